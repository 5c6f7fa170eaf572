"""GPU: the device Douglas-Peucker by the exact rule (predict.simplify_packed_device, csrc/simplify.hip) against simplify_ref, list for
list with np.array_equal and no tolerance: on the device-traced contours of contours_ref.cases(), on hand-built packed inputs that the
tracer would not produce, with the per-vertex state forced into LDS and into the workspace; the refusals; determinism; and the paths
through coastlines_from_mask and CoastlineExtractor with the device simplification on and off."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import contours_ref as CR
import simplify_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = CR.cases()
EPS_FACTORS = (0.002, 0.0, 0.05, 1.0)
HAND = SR.hand_built()
HUGE = 2 ** 31 - 1
_HOST = {}
_REF = {}


def _predict():
    return importlib.import_module("eusipco-2026-robust-unet_amd.predict")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host_contours(name, mask):
    """the host tracer's list (the device tracer's oracle), computed once per mask"""
    if name not in _HOST:
        _HOST[name] = _predict().trace_external_contours(mask)
    return _HOST[name]


def _ref(key, contours, f):
    """simplify_ref on a list of contours, computed once per (key, eps factor) -> ([kept], largest depth)"""
    if (key, f) not in _REF:
        res = [SR.simplify(c, f) for c in contours]
        _REF[(key, f)] = ([k for k, _ in res], max([r["depth"] for _, r in res], default=0))
    return _REF[(key, f)]


def _assert_same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == np.int32 and a.shape == b.shape and np.array_equal(a, b), (what, i, a.tolist()[:8], b.tolist()[:8])


def _run(packed, f, lds=None, sizes=None):
    """-> (host int32 result, head)"""
    out, head = _predict().simplify_packed_device(packed, f, lds_max_vertices=lds, sizes=sizes, with_head=True)
    return out.cpu().numpy(), head


def _check(packed, contours, key, f, lds=None):
    want, depth = _ref(key, contours, f)
    out, head = _run(packed, f, lds)
    n, total = len(contours), sum(len(k) for k in want)
    assert out.size == 3 + n + 2 * total and head == [n, total, 0, depth], (key, f, lds, head, depth)
    assert int(out[0]) == n and int(out[1]) == total and int(out[2]) == 0 and int(out[2 + n]) == total
    _assert_same(SR.unpack(out), want, (key, f, lds))
    return out


@pytest.mark.parametrize("name,mask", CASES, ids=[n for n, _ in CASES])
def test_traced_masks(name, mask):
    P = _predict()
    host = _host_contours(name, mask)
    dm = _dev(mask)
    for min_points in (0, 10):
        contours = [c for c in host if len(c) > min_points]
        packed, sizes = P._trace_packed(dm, min_points, with_sizes=True)
        if packed is None:
            assert not contours
            continue
        assert sizes == (len(contours), sum(len(c) for c in contours))
        for f in EPS_FACTORS:
            out = _check(packed, contours, (name, min_points), f)
            if f == 1.0:                                  # everything collapses to the two anchors (one where all vertices coincide)
                assert all(len(c) <= 2 for c in SR.unpack(out))
            assert np.array_equal(_check(packed, contours, (name, min_points), f, lds=0), out)


def test_short_contours_come_with_min_points_zero():
    by = dict(CASES)
    lens = set()
    for name in ("1x1_set", "corner_nw", "corner_se", "row_full", "col_dashed", "row_dashed"):
        lens |= {len(c) for c in _host_contours(name, by[name])}
    assert {1, 2} <= lens


def test_deep_contours_report_the_reference_depth():
    """the loop over rounds is exercised to the recursion depth, not just survived"""
    P = _predict()
    by = dict(CASES)
    got = []
    for name in ("spiral_64", "spiral_64_complement", "serpentine_128"):
        packed = P._trace_packed(_dev(by[name]), 0)
        contours = _host_contours(name, by[name])
        got.append(_run(packed, 0.002)[1][3])
        assert got[-1] == _ref((name, 0), contours, 0.002)[1]
    assert got == [102, 103, 49]


@pytest.mark.parametrize("f", [0.002, 0.0])
def test_spiral_192_goes_deeper_than_a_workgroup_is_wide(f):
    P = _predict()
    mask = CR.spiral(192)
    contours = _host_contours("spiral_192", mask)
    packed = P._trace_packed(_dev(mask), 0)
    depth = _ref(("spiral_192", 0), contours, f)[1]
    assert depth == {0.002: 172, 0.0: 379}[f]             # 379 rounds: more than the 256 threads of a workgroup
    for lds in (None, 0):
        _check(packed, contours, ("spiral_192", 0), f, lds)


@pytest.mark.parametrize("name,contours,f", HAND, ids=[h[0] for h in HAND])
def test_hand_built_inputs_in_lds_and_in_the_workspace(name, contours, f):
    packed = _dev(SR.pack(contours))
    a = _check(packed, contours, name, f)
    b = _check(packed, contours, name, f, lds=0)
    c = _check(packed, contours, name, f, lds=HUGE)
    d = _check(packed, contours, name, f, lds=12)
    assert a.tobytes() == b.tobytes() == c.tobytes() == d.tobytes()


def test_the_named_mistakes_would_be_seen():
    """the device lists are not the ones `>=` at the threshold and a fused L give, on the two inputs built to tell them apart (the other
    two mistakes change traced contours: test_simplify_ref_cpu.py)"""
    by = {h[0]: h for h in HAND}
    for name, mistake in (("threshold_tie", "ge"), ("fused_L", "fused_L")):
        _, contours, f = by[name]
        wrong = [SR.simplify(c, f, (mistake,))[0].tolist() for c in contours]
        got = [c.tolist() for c in SR.unpack(_run(_dev(SR.pack(contours)), f)[0])]
        assert got == [k.tolist() for k in _ref(name, contours, f)[0]] and got != wrong, (name, mistake)


def test_long_and_short_contours_in_one_call():
    by = {h[0]: h for h in HAND}
    band = _host_contours("coastline_band_256", dict(CASES)["coastline_band_256"])
    contours = by["many_small"][1][:40] + by["long"][1] + list(band) + by["full_range"][1] + by["many_small"][1][40:60]
    packed = _dev(SR.pack(contours))
    outs = [_check(packed, contours, "mixed", 0.002, lds) for lds in (None, 0, 12, 500, HUGE)]
    assert all(o.tobytes() == outs[0].tobytes() for o in outs)


def test_no_contours():
    P = _predict()
    out, head = _run(_dev(np.array([0, 0, 0], np.int32)), 0.002)
    assert out.tolist() == [0, 0, 0] and head == [0, 0, 0, 0]
    assert P.coastlines_from_mask(_dev(np.zeros((9, 13), np.uint8)), rule="exact") == []
    assert P.coastlines_from_mask(torch.zeros((0, 5), device=DEV, dtype=torch.uint8), rule="exact") == []


def _raw_call(packed_np, n, total, f=0.002, lds=-1):
    """the entry point itself on a workspace filled with 0x5A -> (workspace bytes on the host, result offset)"""
    lib_mod = importlib.import_module("eusipco-2026-robust-unet_amd._lib")
    lib = lib_mod.lib
    packed = _dev(packed_np)
    nbytes = lib.runet_contours_simplify_workspace_bytes(n, total)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0x5A, device=DEV, dtype=torch.uint8)
    torch.cuda.synchronize()
    lib_mod.check(lib.runet_contours_simplify(packed.data_ptr(), n, total, f, lds, ws.data_ptr(), nbytes, None))
    torch.cuda.synchronize()
    return ws.cpu().numpy(), lib.runet_contours_simplify_result_offset()


@pytest.mark.parametrize("name", list(SR.BAD_INPUTS))
@pytest.mark.parametrize("lds", [None, 0])
def test_bad_inputs_are_refused(name, lds):
    P = _predict()
    contours = SR.BAD_INPUTS[name]
    packed = SR.pack(contours)
    with pytest.raises(ValueError, match="bad input"):
        P.simplify_packed_device(_dev(packed), 0.002, lds_max_vertices=lds)
    n, total = len(contours), sum(len(c) for c in contours)
    ws, at = _raw_call(packed, n, total, lds=-1 if lds is None else lds)
    head = ws[:16].view(np.int32).tolist()
    assert head[0] == n and head[1] == 0 and head[2] >= 1
    assert np.all(ws[at:at + 4 * (3 + n + 2 * total)] == 0x5A)           # nothing written past the head


@pytest.mark.parametrize("what", ["n", "total", "first_offset", "last_offset", "falling_offsets", "offset_past_the_end"])
def test_a_packed_set_that_does_not_describe_itself_is_refused(what):
    contours = SR.many_small(6)
    packed = SR.pack(contours)
    n, total = len(contours), sum(len(c) for c in contours)
    edit = {"n": (0, n - 1), "total": (1, total + 1), "first_offset": (2, 1), "last_offset": (2 + n, total - 1),
            "falling_offsets": (4, int(packed[3]) - 1), "offset_past_the_end": (4, total + 5)}[what]
    packed[edit[0]] = edit[1]
    ws, at = _raw_call(packed, n, total)
    head = ws[:16].view(np.int32).tolist()
    assert head[1] == 0 and head[2] >= 1 and np.all(ws[at:at + 4 * (3 + n + 2 * total)] == 0x5A)


def test_a_good_call_writes_its_result_and_not_past_it():
    contours = SR.many_small(6)
    n, total = len(contours), sum(len(c) for c in contours)
    ws, at = _raw_call(SR.pack(contours), n, total)
    want = [k for k in _ref("six_small", contours, 0.002)[0]]
    head = ws[:16].view(np.int32).tolist()
    kept = sum(len(k) for k in want)
    assert head[:3] == [n, kept, 0]
    _assert_same(SR.unpack(ws[at:at + 4 * (3 + n + 2 * kept)].view(np.int32)), want, "raw")
    assert np.all(ws[at + 4 * (3 + n + 2 * kept):at + 4 * (3 + n + 2 * total)] == 0x5A)


def test_wrapper_refusals():
    P = _predict()
    packed = _dev(SR.pack(SR.many_small(3)))
    with pytest.raises(ValueError):
        P.simplify_packed_device(packed.cpu(), 0.002)
    with pytest.raises(ValueError):
        P.simplify_packed_device(packed.float(), 0.002)
    for f in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eps_factor"):
            P.simplify_packed_device(packed, f)
    with pytest.raises(ValueError):
        P.simplify_packed_device(packed, 0.002, sizes=(3, 10 ** 6))     # more vertices than the tensor holds
    with pytest.raises(ValueError, match="46341"):
        P.coastlines_from_mask(torch.zeros((1, 46342), device=DEV, dtype=torch.uint8), rule="exact")
    with pytest.raises(ValueError, match="rule"):
        P.coastlines_from_mask(torch.zeros((4, 4), device=DEV, dtype=torch.uint8), rule="exact64")


@pytest.mark.parametrize("lds", [None, 0])
def test_two_runs_give_the_same_bytes(lds):
    P = _predict()
    by = {h[0]: h for h in HAND}
    for packed in (P._trace_packed(_dev(dict(CASES)["noise_130x259_0.55"]), 0), _dev(SR.pack(by["long"][1])),
                   _dev(SR.pack(by["many_small"][1]))):
        a, ha = _run(packed, 0.002, lds)
        b, hb = _run(packed, 0.002, lds)
        assert a.dtype == np.int32 and a.tobytes() == b.tobytes() and ha == hb


# ------------------------------------------------------------------------------------------------ end to end
def _without_device_simplify(fn):
    P = _predict()
    P.DEVICE_SIMPLIFY = False
    try:
        return fn()
    finally:
        P.DEVICE_SIMPLIFY = True


def test_coastlines_from_mask_exact_rule_every_way():
    P = _predict()
    band = dict(CASES)["coastline_band_256"]
    dm = _dev(band)
    want = [k.tolist() for k in _ref(("coastline_band_256", 10), [c for c in _host_contours("coastline_band_256", band) if len(c) > 10],
                                     0.002)[0]]
    assert len(want) >= 3
    assert P.coastlines_from_mask(dm, rule="exact") == want
    assert P.coastlines_from_mask(band, rule="exact") == want
    assert _without_device_simplify(lambda: P.coastlines_from_mask(dm, rule="exact")) == want
    noisy = dict(CASES)["noise_130x259_0.30"]
    for min_points, f in ((0, 0.002), (10, 0.05)):
        a = P.coastlines_from_mask(_dev(noisy), min_points, f, rule="exact")
        assert a == P.coastlines_from_mask(noisy, min_points, f, rule="exact")
        assert a == _without_device_simplify(lambda: P.coastlines_from_mask(_dev(noisy), min_points, f, rule="exact"))


def test_default_rule_is_todays():
    P = _predict()
    band = dict(CASES)["coastline_band_256"]
    want = P._simplify(_host_contours("coastline_band_256", band), 10, 0.002)
    assert P.coastlines_from_mask(_dev(band)) == want == P.coastlines_from_mask(_dev(band), rule="float64")


@pytest.fixture(scope="module")
def extractors(pkg):
    torch.manual_seed(3)
    net = pkg.UNet(3, 2)                                 # untrained: its noisy mask is a good tracer input
    return (pkg.CoastlineExtractor(model=net, device=DEV, input_size=64, simplify_rule="exact"),
            pkg.CoastlineExtractor(model=net, device=DEV, input_size=64))


def test_extract_coastline_contours_exact_both_ways(extractors):
    P = _predict()
    exact, default = extractors
    water = _dev(CR.smooth_field_water(200, seed=5))
    lines, coast = exact.extract_coastline_contours(water, 5)
    lines_host, coast_host = _without_device_simplify(lambda: exact.extract_coastline_contours(water, 5))
    assert len(lines) >= 1 and lines == lines_host and np.array_equal(coast, coast_host)
    assert lines == P.coastlines_from_mask(coast_host, rule="exact")
    lines_default, coast_default = default.extract_coastline_contours(water, 5)
    assert np.array_equal(coast_default, coast) and lines_default == P._simplify(P.trace_external_contours(coast), 10, 0.002)


def test_extract_coastline_from_image_tiled_exact_both_ways(extractors):
    P = _predict()
    exact, default = extractors
    scene = np.random.default_rng(9).integers(0, 256, (96, 80, 3), dtype=np.uint8)
    a = exact.extract_coastline_from_image(scene, tiled=True, tile=64, halo=16)
    b = _without_device_simplify(lambda: exact.extract_coastline_from_image(scene, tiled=True, tile=64, halo=16))
    torch.cuda.synchronize()
    assert set(a) == set(b)
    for key in a:
        if key == "extraction_time":
            continue
        same = np.array_equal(a[key], b[key]) if isinstance(a[key], np.ndarray) else a[key] == b[key]
        assert same, key
    assert a["coastlines"] == P.coastlines_from_mask(a["coastline_mask"], rule="exact") and a["coastline_count"] == len(a["coastlines"])
    d = default.extract_coastline_from_image(scene, tiled=True, tile=64, halo=16)
    assert np.array_equal(d["coastline_mask"], a["coastline_mask"])
    assert d["coastlines"] == P._simplify(P.trace_external_contours(d["coastline_mask"]), 10, 0.002)
