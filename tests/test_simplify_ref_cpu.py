"""CPU: the exact Douglas-Peucker rule.  predict.approx_poly_dp_exact (the host restatement the product uses) against simplify_ref (the
independent recursive restatement) on the traced contours of contours_ref.cases() and the hand-built inputs; the property every result
must have, in exact rational arithmetic; where the exact rule and the float64 rule part; and that each named mistake of simplify_ref
changes a list on at least one input the GPU test runs, so that test can see it."""
import importlib
from fractions import Fraction

import numpy as np
import pytest

import contours_ref as CR
import simplify_ref as SR

EPS_FACTORS = (0.002, 0.0, 0.05, 1.0)
_TRACED = {}


def _predict():
    return importlib.import_module("eusipco-2026-robust-unet_amd.predict")


def traced():
    """{mask name: the host tracer's contours}, computed once"""
    if not _TRACED:
        P = _predict()
        for name, mask in CR.cases():
            _TRACED[name] = P.trace_external_contours(mask)
    return _TRACED


def gpu_inputs():
    """every (label, contour, eps_factor) the GPU test simplifies"""
    out = []
    for name, contours in traced().items():
        for f in EPS_FACTORS:
            out += [(f"{name}[{i}]@{f}", c, f) for i, c in enumerate(contours)]
    for name, contours, f in SR.hand_built():
        out += [(f"{name}[{i}]@{f}", c, f) for i, c in enumerate(contours)]
    return out


def test_host_restatement_equals_the_reference_on_traced_contours():
    P = _predict()
    n = 0
    for name, contours in traced().items():
        for f in EPS_FACTORS:
            for i, c in enumerate(contours):
                want, _ = SR.simplify(c, f)
                got = P.approx_poly_dp_exact(c, f)
                assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), (name, i, f)
                n += 1
            for min_points in (0, 10):
                want = [SR.simplify(c, f)[0].tolist() for c in contours if len(c) > min_points]
                assert P._simplify_exact(contours, min_points, f) == want, (name, f, min_points)
    assert n > 4 * 1000


def test_host_restatement_equals_the_reference_on_hand_built_inputs():
    P = _predict()
    for name, contours, f in SR.hand_built():
        for i, c in enumerate(contours):
            want, _ = SR.simplify(c, f)
            assert np.array_equal(P.approx_poly_dp_exact(c, f), want), (name, i)


def test_everything_collapses_to_the_two_anchors_at_eps_factor_one():
    for name, contours in traced().items():
        for c in contours:
            got, rec = SR.simplify(c, 1.0)
            assert len(got) == (2 if rec["far"] else 1), name


def _dist2_to_segment(p, a, b):
    """exact squared distance of p to the clipped segment a-b"""
    abx, aby, apx, apy = b[0] - a[0], b[1] - a[1], p[0] - a[0], p[1] - a[1]
    den = abx * abx + aby * aby
    t = Fraction(0) if den == 0 else min(Fraction(1), max(Fraction(0), Fraction(apx * abx + apy * aby, den)))
    return (apx - t * abx) ** 2 + (apy - t * aby) ** 2


@pytest.mark.parametrize("f", [0.002, 0.05])
def test_property_of_the_result(f):
    """a subsequence of the input that starts at vertex 0 and contains `far`; every dropped vertex lies within eps of the clipped segment
    that replaces it (eps^2 compared as the exact rational value of the rounded thr, which is what the rule compares against)"""
    P = _predict()
    checked = 0
    sets = [(name, cs) for name, cs in traced().items()] + [(name, cs) for name, cs, _ in SR.hand_built()]
    for name, contours in sets:
        for c in contours:
            pts = [tuple(v) for v in c.tolist()]
            n = len(pts)
            got = [tuple(v) for v in P.approx_poly_dp_exact(c, f).tolist()]
            d2 = [(x - pts[0][0]) ** 2 + (y - pts[0][1]) ** 2 for x, y in pts]
            far = d2.index(max(d2))
            assert got[0] == pts[0]
            keep_idx = _kept_positions(c, f)
            assert [pts[i] for i in keep_idx] == got and keep_idx[0] == 0 and (far in keep_idx)
            thr = Fraction(SR.threshold(pts, f).item())
            q = pts + pts[:1]
            bounds = keep_idx + [n]
            for a, b in zip(bounds[:-1], bounds[1:]):
                for i in range(a + 1, b):
                    assert _dist2_to_segment(q[i], q[a], q[b]) <= thr, (name, a, b, i)
                    checked += 1
    assert checked > 1000


def _kept_positions(c, f):
    """the positions simplify_ref keeps (its list gives the vertices; revisited pixels make the positions ambiguous, so redo it on labels)"""
    pts = [tuple(v) for v in np.asarray(c).tolist()]
    n = len(pts)
    thr = SR.threshold(pts, f)
    d2 = [(x - pts[0][0]) ** 2 + (y - pts[0][1]) ** 2 for x, y in pts]
    far = d2.index(max(d2))
    if far == 0:
        return [0]
    q = pts + pts[:1]
    keep = {0, far}
    stack = [(0, far), (far, n)]
    while stack:
        a, b = stack.pop()
        if b - a < 2:
            continue
        nums = [SR.numerator(q[a], q[b], q[i]) for i in range(a + 1, b)]
        best = max(v for v, _ in nums)
        k = a + 1 + [v for v, _ in nums].index(best)
        if np.float64(float(best)) > thr * np.float64(float(nums[0][1])):
            keep.add(k)
            stack += [(a, k), (k, b)]
    return sorted(keep)


def test_the_two_rules_part_only_at_ties():
    """on cases() at 0.002 the exact rule and the float64 rule return equal lists; a contour on which they do not must show a tie or a
    threshold margin below 1e-9 in its record"""
    P = _predict()
    n = 0
    for name, contours in traced().items():
        long_ones = [c for c in contours if len(c) > 10]
        a = P._simplify(long_ones, 10, 0.002)
        b = P._simplify_exact(long_ones, 10, 0.002)
        for c, x, y in zip(long_ones, a, b):
            n += 1
            if x != y:
                rec = SR.simplify(c, 0.002)[1]
                assert rec["ties"] > 0 or rec["far_ties"] > 0 or rec["margin"] < 1e-9, (name, rec)
    assert n == 408


def test_ties_are_common_on_the_traced_contours():
    recs = [SR.simplify(c, 0.002)[1] for c in traced()["noise_130x259_0.30"] if len(c) > 10]
    splits, ties = sum(r["splits"] for r in recs), sum(r["ties"] for r in recs)
    assert splits > 1000 and 0.05 * splits < ties < 0.3 * splits, (splits, ties)


def test_deep_contours_have_the_depths_the_kernel_must_reach():
    t = traced()
    assert [SR.simplify(t[k][0], 0.002)[1]["depth"] for k in ("spiral_64", "spiral_64_complement", "serpentine_128")] == [102, 103, 49]


def test_hand_built_inputs_are_what_they_claim():
    by = {name: (cs, f) for name, cs, f in SR.hand_built()}
    # eps == h == 4 exactly, N == thr * den on the deciding chord
    (c,), f = by["threshold_tie"]
    assert SR.arc_terms(c.tolist()) == (256, 0) and SR.threshold(c.tolist(), f) == 16.0
    assert SR.numerator((0, 0), (124, 0), (40, 4)) == (16 * 124 * 124, 124 * 124)
    assert SR.simplify(c, f)[1]["margin"] == 0.0
    # the fused and the unfused arc length differ in the last bit
    (c,), f = by["fused_L"]
    a, d = SR.arc_terms(c.tolist())
    assert (a, d) == (24, 18) and SR.arc_length(a, d) != SR.arc_length(a, d, fused=True)
    assert SR.threshold(c.tolist(), f) == 3.24 and SR.threshold(c.tolist(), f, fused=True) < 3.24
    # the whole coordinate range: N reaches 46340^4, which is the largest value the rule can produce (for three points in a square of
    # side s, |ap| |ab| with a right or obtuse angle at a, and the cross product, are at most s^2) - above 2^61, far beyond 32 bits
    cs, f = by["full_range"]
    s = SR.COORD_MAX
    assert SR.numerator((0, 0), (s, s), (s, 0))[0] == s ** 4 > 2 ** 61
    assert max(int(c.max()) for c in cs) == s and min(int(c.min()) for c in cs) == 0
    # long and many
    assert len(by["long"][0][0]) >= 2 * 2048 and len(by["many_small"][0]) == 300
    assert {len(c) for c in by["many_small"][0]} == {11, 12, 13}
    assert sum(len(c) for c in by["many_small"][0]) > 2048
    for name, contours, _ in SR.hand_built():
        for c in contours:
            SR.arc_terms(c.tolist())                      # every hand-built contour is a good input


def test_bad_inputs_are_refused_by_the_host_restatement():
    P = _predict()
    for name, contours in SR.BAD_INPUTS.items():
        with pytest.raises(ValueError):
            for c in contours:
                P.approx_poly_dp_exact(c, 0.002)
        with pytest.raises(ValueError):
            for c in contours:
                SR.simplify(c, 0.002)
    for f in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            P.approx_poly_dp_exact([[0, 0], [4, 0], [4, 4]], f)
    with pytest.raises(ValueError):
        P.approx_poly_dp_exact(np.array([[0.5, 0.0], [4.0, 0.0]]), 0.002)


def test_rule_names_and_the_size_bound():
    P = _predict()
    band = dict(CR.cases())["coastline_band_256"]
    assert P.coastlines_from_mask(band, rule="exact") == P._simplify_exact(traced()["coastline_band_256"], 10, 0.002)
    assert P.coastlines_from_mask(band, rule="float64") == P.coastlines_from_mask(band)
    with pytest.raises(ValueError, match="rule"):
        P.coastlines_from_mask(band, rule="cv2")
    with pytest.raises(ValueError, match="46341"):
        P.coastlines_from_mask(np.zeros((1, 46342), np.uint8), rule="exact")
    assert P.coastlines_from_mask(np.zeros((1, 46341), np.uint8), rule="exact") == []
    with pytest.raises(ValueError, match="rule"):
        P.CoastlineExtractor(device="cpu", simplify_rule="nearest")


def test_entry_point_validates_on_the_host_without_a_gpu():
    import ctypes
    lib = importlib.import_module("eusipco-2026-robust-unet_amd._lib").lib
    sizes = lib.runet_contours_simplify_workspace_bytes
    assert sizes(0, 0) > 0 and sizes(3, 40) > sizes(3, 20) > 0
    assert sizes(-1, 4) == -1 and sizes(5, 4) == -1 and sizes(1, 1 << 30) == -1
    assert lib.runet_contours_simplify_result_offset() % 16 == 0
    p, big = ctypes.c_void_p(256), 1 << 40
    call = lib.runet_contours_simplify
    for args, word in (((None, 1, 4, 0.002, -1, p, big, None), b"null pointer"),
                       ((p, 1, 4, 0.002, -1, None, big, None), b"null pointer"),
                       ((p, -1, 4, 0.002, -1, p, big, None), b"n <= total"),
                       ((p, 5, 4, 0.002, -1, p, big, None), b"n <= total"),
                       ((p, 1, 4, -0.5, -1, p, big, None), b"eps_factor"),
                       ((p, 1, 4, float("nan"), -1, p, big, None), b"eps_factor"),
                       ((p, 1, 4, float("inf"), -1, p, big, None), b"eps_factor"),
                       ((ctypes.c_void_p(258), 1, 4, 0.002, -1, p, big, None), b"aligned"),
                       ((p, 1, 4, 0.002, -1, ctypes.c_void_p(264), big, None), b"aligned"),
                       ((p, 1, 4, 0.002, -1, p, sizes(1, 4) - 1, None), b"workspace too small")):
        assert call(*args) != 0 and word in lib.runet_last_error(), (args, lib.runet_last_error())


@pytest.mark.parametrize("mistake", SR.MISTAKES)
def test_every_named_mistake_changes_a_list_the_gpu_test_compares(mistake):
    changed = []
    for label, c, f in gpu_inputs():
        if len(c) > 600:
            continue                                      # the long contour: not needed to show a difference
        if SR.simplify(c, f, (mistake,))[0].tolist() != SR.simplify(c, f)[0].tolist():
            changed.append(label)
            if len(changed) >= 3:
                break
    assert changed, mistake
