"""CPU: the numpy restatement of the exact distance transform (boundary.distance_transform_sq_host) against the brute-force table and
scipy, the named mistakes against the cases, the scores on hand-checkable inputs through the host route, and the host-side refusals of
the three entry points.  No tolerance anywhere: squared pixel distances are integers."""
import ctypes
import importlib
import math

import numpy as np
import pytest

import edt_ref as E


def _boundary():
    return importlib.import_module("eusipco-2026-robust-unet_amd.boundary")


@pytest.fixture
def host_route(monkeypatch):
    monkeypatch.setenv("RUNET_NO_DEVICE_EDT", "1")       # read at call time
    return _boundary()


@pytest.fixture(scope="module")
def truths():
    return {name: E.truth(m, inv) for name, m, inv in E.cases()}


def test_host_restatement_equals_the_brute_force_table(truths):
    B = _boundary()
    for name, m, inv in E.cases():
        got = B.distance_transform_sq_host(m, invert=inv)
        assert got.dtype == np.int32 and got.shape == m.shape and np.array_equal(got, truths[name]), name
    m = E.contents(5, 9, 3)["corner 00"]
    assert truths["3x5 corner 11"][0, 0] == 2 * 2 + 4 * 4 and B.distance_transform_sq_host(m)[4, 8] == 4 * 4 + 8 * 8
    assert (B.distance_transform_sq_host(np.zeros((3, 4), bool)) == B.NONE).all() and B.NONE == E.NONE == 2 ** 31 - 1
    batch = np.stack([E.contents(6, 11, k)[c] for k, c in enumerate(("random 0.5", "no feature", "two ends"))])
    got = B.distance_transform_sq_host(batch)
    assert got.shape == batch.shape and all(np.array_equal(got[i], E.truth(batch[i])) for i in range(3))
    assert np.array_equal(B.distance_transform_sq_host(batch != 0), got)


def test_host_restatement_equals_scipy(truths):
    ndimage = pytest.importorskip("scipy.ndimage")
    B = _boundary()
    for name, m, inv in E.cases():
        feat = E.features(m, inv)
        if not feat.any():
            continue                                     # scipy has no "no feature" value
        want = np.rint(ndimage.distance_transform_edt(~feat) ** 2).astype(np.int64)
        assert np.array_equal(B.distance_transform_sq_host(m, invert=inv), want), name
    for h, w, density in ((96, 130, 0.5), (96, 130, 0.01), (2, 3000, 0.001), (3000, 2, 0.001)):
        feat = np.random.default_rng(h + w).random((h, w)) < density
        feat[h - 1, 0] = True
        want = np.rint(ndimage.distance_transform_edt(~feat) ** 2).astype(np.int64)
        assert np.array_equal(B.distance_transform_sq_host(feat), want), (h, w, density)


def test_integer_range_lines():
    """a single feature at one end of the longest line there is: d2 up to 32767^2 + 1"""
    B = _boundary()
    for shape in ((2, 32768), (32768, 2)):
        m = np.zeros(shape, np.uint8)
        m[0, 0] = 1
        yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
        got = B.distance_transform_sq_host(m)
        assert np.array_equal(got, yy * yy + xx * xx) and got.max() == 32767 ** 2 + 1
    with pytest.raises(ValueError):
        B.distance_transform_sq_host(np.zeros((1, 32769), np.uint8))
    with pytest.raises(ValueError):
        B.distance_transform_sq_host(np.zeros((4, 4), np.float32))


def test_the_cases_see_every_named_mistake(truths):
    cases = E.cases()
    for name, kind, fn in E.mistakes():
        if kind == "d2":
            seen = [c for c, m, inv in cases if not np.array_equal(fn(m, inv), truths[c])]
        else:
            seen = []
            for c, m, inv in cases:
                d2 = truths[c][None]
                if not np.array_equal(fn(d2, None, (1, 4))[0], E.stats(d2, None, (1, 4))[0]):
                    seen.append(c)
        assert seen, f"no case tells '{name}' from the truth"
    # and the separable form without a mistake is the truth, so the two switches are what the cases see
    for c, m, inv in cases:
        assert np.array_equal(E._two_pass(E.features(m, inv)), truths[c]), c


def test_stats_restatements_agree(truths):
    B = _boundary()
    rng = np.random.default_rng(5)
    for c in ("16x17 random 0.05", "65x67 random 0.05", "3x5 no feature", "1x1 all features"):
        d2 = truths[c][None]
        for select in (None, (rng.random(d2.shape) < 0.4).astype(np.uint8)):
            for tol in ((), (0, 1, 4, 9, 16, 25, 36, 10 ** 9)):
                got, want = B._stats_host(d2, select, list(tol)), E.stats(d2, select, tol)
                assert np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes(), (c, tol)
    e = rng.random(70 * 1024 + 5)
    assert B.ordered_sum(e) == E.ordered_sum(e) and abs(E.ordered_sum(e) - math.fsum(e)) < 1e-8


# ------------------------------------------------------------------------------------------------ the kernel's column walk
def _column_walk(col, h, ahead=8):
    """edt_col_kernel (csrc/edt.hip) line by line on one column, IN PLACE: col holds g (-1: the row has no feature), then the stack
    entries row | g << 15, then d2; `start` is the workspace.  The asserts are the two facts the in-place form rests on: an entry is
    written at or behind the row being worked on, and the fill never overwrites a live entry."""
    start = [0] * h
    q, ts, tg, tt = -1, 0, 0, 0
    for u0 in range(0, h, ahead):
        gbuf = [int(col[u0 + j]) if u0 + j < h else -1 for j in range(ahead)]     # read before anything at or behind these rows is written
        for j, g in enumerate(gbuf):
            u = u0 + j
            if g < 0:
                continue
            while q >= 0 and (tt - ts) ** 2 + tg * tg > (tt - u) ** 2 + g * g:
                q -= 1
                if q >= 0:
                    ts, tg, tt = int(col[q]) & 0x7fff, int(col[q]) >> 15, start[q]
            if q < 0:
                push, tt = True, 0
            else:
                sep = (u * u - ts * ts + g * g - tg * tg) // (2 * (u - ts))
                push = sep + 1 < h
                if push:
                    tt = sep + 1
            if push:
                q, ts, tg = q + 1, u, g
                assert q <= u
                col[q], start[q] = ts | (tg << 15), tt
    if q < 0:
        col[:] = E.NONE
        return
    for u in range(h - 1, -1, -1):
        assert q <= u
        col[u] = (u - ts) ** 2 + tg * tg
        if u == tt:
            q -= 1
            if q >= 0:
                ts, tg, tt = int(col[q]) & 0x7fff, int(col[q]) >> 15, start[q]
    assert q == -1


def test_the_in_place_column_walk_is_the_truth(truths):
    for name, m, inv in E.cases():
        feat = E.features(m, inv)
        h, w = feat.shape
        x = np.arange(w)
        d = np.where(feat.any(axis=1)[:, None], np.where(feat[:, None, :], np.abs(x[:, None] - x[None, :])[None], 10 ** 6).min(axis=2), -1)
        for c in range(w):
            col = d[:, c].copy()
            _column_walk(col, h)
            d[:, c] = col
        assert np.array_equal(d, truths[name]), name


# ------------------------------------------------------------------------------------------------ the scores, by hand
def test_two_pixels_three_and_four_apart(host_route):
    B = host_route
    a, b = np.zeros((9, 11), np.uint8), np.zeros((9, 11), bool)
    a[2, 3], b[5, 7] = 1, True
    r = B.coastline_deviation(a, b, tolerances=(1, 4, 5))
    for d in (r["pred_to_true"], r["true_to_pred"]):
        assert (d["count"], d["unreachable"], d["mean"], d["rms"], d["max"]) == (1, 0, 5.0, 5.0, 5.0)
        assert d["within"] == {1: {"count": 0, "fraction": 0.0}, 4: {"count": 0, "fraction": 0.0}, 5: {"count": 1, "fraction": 1.0}}
    assert r["hausdorff"] == 5.0 and r["assd"] == 5.0
    r = B.coastline_deviation(a, b, pixel_size=10.0)
    assert r["pred_to_true"]["mean"] == 50.0 and r["hausdorff"] == 50.0 and r["assd"] == 50.0
    for bad in ((1.5,), (True,), (-1,), tuple(range(9))):
        with pytest.raises(ValueError):
            B.coastline_deviation(a, b, tolerances=bad)
    with pytest.raises(ValueError):
        B.coastline_deviation(a, b[:, :10])


def test_identical_masks(host_route):
    B = host_route
    m = np.zeros((20, 24), np.uint8)
    m[4:15, 6:20] = 1
    coast = m.copy()
    coast[5:14, 7:19] = 0                                # a ring
    r = B.coastline_deviation(coast, coast)
    n = int(coast.sum())
    for d in (r["pred_to_true"], r["true_to_pred"]):
        assert (d["count"], d["unreachable"], d["mean"], d["rms"], d["max"]) == (n, 0, 0.0, 0.0, 0.0)
        assert all(v == {"count": n, "fraction": 1.0} for v in d["within"].values())
    assert r["hausdorff"] == 0.0 and r["assd"] == 0.0
    s = B.boundary_scores(m, m)
    assert s["bf1"] == 1.0 and s["boundary_iou"] == 1.0 and s["boundary_precision"] == 1.0 and s["boundary_recall"] == 1.0
    assert s["pred_boundary_pixels"] == n                # the inner boundary of a rectangle is its ring
    # shifted by one pixel: every boundary pixel is within 2 of the other boundary, the 2-pixel bands overlap in part
    g = np.roll(m, 1, axis=1)
    s = B.boundary_scores(m, g, tolerance=2)
    assert s["bf1"] == 1.0 and 0.0 < s["boundary_iou"] < 1.0
    assert B.boundary_scores(m, g, tolerance=0)["boundary_precision"] == (2 * 13 + 0) / n      # the two long sides stay shared


def test_empty_prediction(host_route):
    B = host_route
    truth = np.zeros((12, 12), np.uint8)
    truth[3:9, 3:9] = 1
    ring = truth.copy()
    ring[4:8, 4:8] = 0
    r = B.coastline_deviation(np.zeros_like(ring), ring)
    a, b = r["pred_to_true"], r["true_to_pred"]
    assert a["count"] == 0 and all(math.isnan(a[k]) for k in ("mean", "rms", "max"))
    assert b["count"] == b["unreachable"] == int(ring.sum()) and b["mean"] == b["rms"] == b["max"] == math.inf
    assert all(v == {"count": 0, "fraction": 0.0} for v in b["within"].values())
    assert r["hausdorff"] == math.inf and r["assd"] == math.inf
    assert r == B.coastline_deviation(np.zeros_like(ring), ring)                  # NaN fields and all
    s = B.boundary_scores(np.zeros_like(truth), truth)
    assert (s["boundary_precision"], s["boundary_recall"], s["bf1"], s["boundary_iou"]) == (1.0, 0.0, 0.0, 0.0)
    both = B.coastline_deviation(np.zeros_like(ring), np.zeros_like(ring))
    assert math.isnan(both["hausdorff"]) and math.isnan(both["assd"])


def test_all_water_has_no_boundary(host_route):
    """the frame is not background: a mask that fills the tile has no boundary at all"""
    B = host_route
    water = np.ones((10, 14), np.uint8)
    s = B.boundary_scores(water, water)
    assert s["pred_boundary_pixels"] == s["true_boundary_pixels"] == 0 and s["bf1"] == 1.0 and s["boundary_iou"] == 1.0
    half = water.copy()
    half[:, 7:] = 0                                      # the only boundary is the column next to the land, not the tile's edge
    assert B.boundary_scores(half, half)["pred_boundary_pixels"] == 10
    batch = B.boundary_scores(np.stack([water, half]), np.stack([water, half]))
    assert [b["pred_boundary_pixels"] for b in batch] == [0, 10]


# ------------------------------------------------------------------------------------------------ the C ABI without a GPU
def test_refusals_return_error_codes_without_a_gpu():
    lib = importlib.import_module("eusipco-2026-robust-unet_amd._lib").lib
    p = ctypes.c_void_p(64)                              # never dereferenced: every call below is refused on the host
    assert lib.runet_edt_workspace_bytes(1, 512, 512) >= 2 * 512 * 512 and lib.runet_edt_workspace_bytes(3, 1, 1) >= 8
    assert lib.runet_edt_workspace_bytes(2, 32768, 32768) > 0
    for n, h, w in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (1, 32769, 4), (1, 4, 32769), (-1, 4, 4)):
        assert lib.runet_edt_workspace_bytes(n, h, w) == -1, (n, h, w)
    big = 1 << 40
    # runet_edt_sq_u8(mask, n, h, w, row_stride, image_stride, invert, d2, workspace, workspace_bytes, stream)
    for args, word in (((None, 1, 4, 4, 4, 16, 0, p, p, big, None), b"null pointer"),
                       ((p, 1, 4, 4, 4, 16, 0, None, p, big, None), b"null pointer"),
                       ((p, 1, 4, 4, 4, 16, 0, p, None, big, None), b"null pointer"),
                       ((p, 0, 4, 4, 4, 16, 0, p, p, big, None), b"bad shape"),
                       ((p, 1, 32769, 4, 4, 16, 0, p, p, big, None), b"32768"),
                       ((p, 1, 4, 32769, 32769, 16, 0, p, p, big, None), b"32768"),
                       ((p, 1, 4, 4, 3, 16, 0, p, p, big, None), b"row stride"),
                       ((p, 2, 4, 4, 4, 15, 0, p, p, big, None), b"image stride"),
                       ((p, 1, 4, 4, 4, 16, 0, p, p, lib.runet_edt_workspace_bytes(1, 4, 4) - 1, None), b"workspace too small")):
        assert lib.runet_edt_sq_u8(*args) != 0 and word in lib.runet_last_error(), (args, lib.runet_last_error())
    # runet_edt_stats(d2, select, n, h, w, tol_sq, n_tol, counts, sums, workspace, workspace_bytes, stream)
    for args, word in (((None, None, 1, 4, 4, None, 0, p, p, p, big, None), b"null pointer"),
                       ((p, None, 1, 4, 4, None, 0, None, p, p, big, None), b"null pointer"),
                       ((p, None, 1, 4, 4, None, 0, p, None, p, big, None), b"null pointer"),
                       ((p, None, 1, 4, 4, None, 2, p, p, p, big, None), b"null pointer"),
                       ((p, None, 1, 32769, 4, None, 0, p, p, p, big, None), b"32768"),
                       ((p, None, 1, 4, 4, p, 9, p, p, p, big, None), b"tolerances"),
                       ((p, None, 1, 4, 4, p, -1, p, p, p, big, None), b"tolerances"),
                       ((p, None, 1, 4, 4, None, 0, p, p, p, 7, None), b"workspace too small")):
        assert lib.runet_edt_stats(*args) != 0 and word in lib.runet_last_error(), (args, lib.runet_last_error())
