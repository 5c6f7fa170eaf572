"""GPU: the device contour tracer (predict.trace_external_contours_device, csrc/contours.hip) against the unchanged host tracer
predict.trace_external_contours, array for array (exact integer equality, no tolerance), on the masks of contours_ref.cases(); then the
paths through coastlines_from_mask and CoastlineExtractor with the device tracing on and off."""
import importlib

import numpy as np
import pytest
import torch

import contours_ref as CR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = CR.cases()
_WANT = {}


def _predict():
    return importlib.import_module("eusipco-2026-robust-unet_amd.predict")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _want(name, mask):
    """the host tracer's list, computed once per mask"""
    if name not in _WANT:
        _WANT[name] = _predict().trace_external_contours(mask)
    return _WANT[name]


def _assert_same(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == np.int32 and a.shape == b.shape and np.array_equal(a, b), (i, a.tolist()[:8], b.tolist()[:8])


@pytest.mark.parametrize("name,mask", CASES, ids=[n for n, _ in CASES])
def test_device_tracer_equals_the_host_tracer(name, mask):
    P = _predict()
    want = _want(name, mask)
    dm = _dev(mask)
    _assert_same(P.trace_external_contours_device(dm), want)
    _assert_same(P.trace_external_contours_device(dm, min_points=10), [c for c in want if len(c) > 10])


def test_expected_contour_counts():
    P = _predict()
    by = dict(CASES)
    counts = {"empty": 0, "all_ones": 1, "1x1_set": 1, "1x1_clear": 0, "squares_touching_at_a_corner": 1, "diagonal_ring_with_dot": 1,
              "dot_in_ring_in_ring": 1, "two_rings_with_islands": 2, "spiral_64": 1, "serpentine_128": 1}
    for name, n in counts.items():
        got = P.trace_external_contours_device(_dev(by[name]))
        assert len(got) == n, name
    assert P.trace_external_contours_device(_dev(by["all_ones"]))[0].tolist() == [[0, 0], [0, 8], [12, 8], [12, 0]]
    assert P.trace_external_contours_device(_dev(by["1x1_set"]))[0].tolist() == [[0, 0]]


@pytest.mark.parametrize("name", ["37x53", "130x259"])
def test_mask_at_an_address_that_is_not_16_byte_aligned(name):
    P = _predict()
    mask = dict(CASES)[name]
    h, w = mask.shape
    wide = np.zeros((h, w + 9), np.uint8)
    wide[:, 4:4 + w] = mask
    assert np.array_equal(np.ascontiguousarray(wide[:, 4:4 + w]), mask)
    flat = torch.zeros(h * w + 4, device=DEV, dtype=torch.uint8)
    view = flat[4:].view(h, w)                           # dense rows, data pointer 4 bytes past an aligned one
    view.copy_(_dev(wide)[:, 4:4 + w])
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    _assert_same(P.trace_external_contours_device(view), _want(name, mask))
    _assert_same(P.trace_external_contours_device(_dev(wide)[:, 4:4 + w]), _want(name, mask))      # a strided view: made dense by the call


@pytest.mark.parametrize("name", ["noise_130x259_0.55", "serpentine_128_complement", "coastline_band_256"])
def test_two_runs_give_the_same_bytes(name):
    P = _predict()
    dm = _dev(dict(CASES)[name])
    a = P._trace_packed(dm, 0).cpu().numpy()
    b = P._trace_packed(dm, 0).cpu().numpy()
    assert a.dtype == np.int32 and a.tobytes() == b.tobytes()
    n, total = int(a[0]), int(a[1])
    assert a.size == 3 + n + 2 * total and a[2] == 0 and a[2 + n] == total and np.all(np.diff(a[2:3 + n]) >= 1)


def test_coastlines_from_mask_takes_a_device_tensor():
    P = _predict()
    water = CR.smooth_field_water()
    coast, _, _ = P.dilate_diff(_dev(water), 5)
    band = coast.cpu().numpy()
    assert np.array_equal(band, dict(CASES)["coastline_band_256"])       # the product's own dilate_diff gives the CPU test's band
    want = P.coastlines_from_mask(band)
    assert len(want) >= 3
    assert P.coastlines_from_mask(coast) == want
    P.DEVICE_CONTOURS = False
    try:
        assert P.coastlines_from_mask(coast) == want
    finally:
        P.DEVICE_CONTOURS = True


@pytest.fixture(scope="module")
def extractor(pkg):
    torch.manual_seed(3)
    net = pkg.UNet(3, 2)                                 # untrained: its noisy mask is a good tracer input
    return pkg.CoastlineExtractor(model=net, device=DEV, input_size=64)


def test_extract_coastline_contours_both_ways(extractor):
    P = _predict()
    water = _dev(CR.smooth_field_water(200, seed=5))
    lines, coast = extractor.extract_coastline_contours(water, 5)
    P.DEVICE_CONTOURS = False
    try:
        lines_host, coast_host = extractor.extract_coastline_contours(water, 5)
    finally:
        P.DEVICE_CONTOURS = True
    assert len(lines) >= 1 and lines == lines_host and np.array_equal(coast, coast_host)
    assert lines == P.coastlines_from_mask(coast_host)


def test_extract_coastline_from_image_tiled_both_ways(extractor):
    P = _predict()
    scene = np.random.default_rng(9).integers(0, 256, (96, 80, 3), dtype=np.uint8)
    a = extractor.extract_coastline_from_image(scene, tiled=True, tile=64, halo=16)
    P.DEVICE_CONTOURS = False
    try:
        b = extractor.extract_coastline_from_image(scene, tiled=True, tile=64, halo=16)
    finally:
        P.DEVICE_CONTOURS = True
    torch.cuda.synchronize()
    assert a["coastlines"] == b["coastlines"] and a["coastline_count"] == b["coastline_count"]
    assert np.array_equal(a["coastline_mask"], b["coastline_mask"]) and np.array_equal(a["water_mask"], b["water_mask"])
    assert (a["water_pixels"], a["coastline_pixels"]) == (b["water_pixels"], b["coastline_pixels"])
    assert a["coastlines"] == P.coastlines_from_mask(a["coastline_mask"])
    assert a["coastline_mask"].shape == (96, 80) and a["image_size"] == (80, 96)
