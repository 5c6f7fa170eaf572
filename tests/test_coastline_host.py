"""CPU: everything of the prediction path (predict.py, csrc/coastline.hip) that runs without a GPU - the C ABI of the new entry points and
their host-side validation, the ellipse spans, the tile plan, the CPU restatement's own rules, the contour tracer and the result files."""
import ctypes
import importlib
import json
import os

import numpy as np
import pytest
from PIL import Image

import coastline_ref as R
from conftest import ROOT

ENTRIES = ("runet_ellipse_spans", "runet_scene_to_tiles", "runet_argmax_stitch", "runet_resize_nearest_u8", "runet_dilate_diff_u8")
P16 = ctypes.c_void_p(4096)          # a non-null, 16-byte aligned "pointer": validation must fail before anything would touch it


def _predict():
    return importlib.import_module("eusipco-2026-robust-unet_amd.predict")


def _lib():
    return importlib.import_module("eusipco-2026-robust-unet_amd._lib")


def test_new_entry_points_are_declared_exported_and_cite_the_reference():
    lm = _lib()
    protos = lm.parse_header(os.path.join(ROOT, "include", "runet_hip.h"))
    raw = ctypes.CDLL(lm.LIB_PATH)
    for name in ENTRIES:
        assert name in protos, f"{name} not declared in include/runet_hip.h"
        assert hasattr(raw, name), f"{name} not exported by librunet_hip.so"
    assert len(protos["runet_dilate_diff_u8"][1]) == 8 and len(protos["runet_scene_to_tiles"][1]) == 15
    assert "predict_coastline.py:" in open(os.path.join(ROOT, "include", "runet_hip.h")).read()
    pkg = importlib.import_module("eusipco-2026-robust-unet_amd")
    assert "CoastlineExtractor" in pkg.__all__ and pkg.CoastlineExtractor is _predict().CoastlineExtractor


def test_host_side_validation_without_a_gpu():
    lib = _lib().lib
    P = _predict()
    j = (ctypes.c_int * 32)()
    assert lib.runet_ellipse_spans(5, None, j) != 0 and b"null pointer" in lib.runet_last_error()
    assert lib.runet_ellipse_spans(4, j, j) != 0 and b"odd" in lib.runet_last_error()
    assert lib.runet_ellipse_spans(33, j, j) != 0
    assert lib.runet_dilate_diff_u8(None, 8, 8, 5, P16, None, P16, None) != 0 and b"null pointer" in lib.runet_last_error()
    assert lib.runet_dilate_diff_u8(P16, 8, 8, 4, ctypes.c_void_p(8192), None, P16, None) != 0 and b"odd" in lib.runet_last_error()
    assert lib.runet_dilate_diff_u8(P16, 8, 8, 33, ctypes.c_void_p(8192), None, P16, None) != 0
    assert lib.runet_scene_to_tiles(None, 8, 8, 24, P16, 1, 16, 0.5, 0.5, 0.5, 0.2, 0.2, 0.2, P16, None) != 0
    assert lib.runet_scene_to_tiles(P16, 8, 8, 23, P16, 1, 16, 0.5, 0.5, 0.5, 0.2, 0.2, 0.2, P16, None) != 0      # row stride < 3 * w
    assert lib.runet_argmax_stitch(None, 1, 16, 2, P16, 0, P16, 8, 8, None) != 0
    assert lib.runet_argmax_stitch(P16, 1, 16, 2, P16, 8, P16, 8, 8, None) != 0 and b"halo" in lib.runet_last_error()
    assert lib.runet_argmax_stitch(P16, 1, 16, 5, P16, 0, P16, 8, 8, None) != 0 and b"classes" in lib.runet_last_error()
    assert lib.runet_resize_nearest_u8(None, 4, 4, P16, 8, 8, None) != 0
    assert lib.runet_resize_nearest_u8(P16, 4, 4, ctypes.c_void_p(8200), 8, 8, None) != 0 and b"aligned" in lib.runet_last_error()
    for k in (0, 2, 4, 32, 33, -1):
        with pytest.raises(ValueError):
            P.ellipse_spans(k)
    with pytest.raises(ValueError):
        P.tile_plan(100, 100, tile=100, halo=8)          # tile % 16 != 0
    with pytest.raises(ValueError):
        P.tile_plan(100, 100, tile=128, halo=64)         # 2 * halo >= tile
    with pytest.raises(ValueError):
        P.CoastlineExtractor(device="cpu", input_size=500)


def test_ellipse_spans_equal_the_documented_matrices():
    P = _predict()
    want = {1: ["1"], 3: ["010", "111", "010"], 5: ["00100", "11111", "11111", "11111", "00100"]}
    for k, rows in want.items():
        assert ["".join(map(str, r)) for r in P.ellipse_element(k).tolist()] == rows
    assert P.ellipse_element(7).sum(1).tolist() == [1, 5, 7, 7, 7, 5, 1]
    assert P.ellipse_element(9).sum(1).tolist() == [1, 7, 7, 9, 9, 9, 7, 7, 1]
    for k in range(1, 32, 2):
        se = P.ellipse_element(k)
        assert se.shape == (k, k) and se[k // 2, k // 2] == 1
        assert np.array_equal(se, se[::-1]) and np.array_equal(se, se[:, ::-1])
        assert np.array_equal(se, R.ellipse(k))          # the product's C rule and the test's Python restatement agree
        j1, j2 = P.ellipse_spans(k)
        assert np.array_equal(j2 - j1, se.sum(1))


@pytest.mark.parametrize("hw", [(1, 1), (384, 384), (385, 383), (1000, 1531)])
@pytest.mark.parametrize("tile,halo", [(512, 64), (128, 32), (64, 0), (16, 7)])
def test_tile_plan_cores_partition_the_scene(hw, tile, halo):
    h, w = hw
    plan = _predict().tile_plan(h, w, tile, halo)
    assert plan.dtype == np.int32 and plan.ndim == 2 and plan.shape[1] == 2
    cover = np.zeros((h, w), dtype=np.int32)
    for y0, x0 in plan.tolist():
        ya, yb = max(y0 + halo, 0), min(y0 + tile - halo, h)
        xa, xb = max(x0 + halo, 0), min(x0 + tile - halo, w)
        assert ya < yb and xa < xb, "a tile without a core pixel in the scene"
        cover[ya:yb, xa:xb] += 1
    assert cover.min() == 1 and cover.max() == 1         # disjoint, and their union is the scene; every tile is `tile` wide by construction
    core = tile - 2 * halo
    assert len(plan) == -(-h // core) * -(-w // core)
    assert plan[0].tolist() == [-halo, -halo]


def test_reference_restatement_self_checks():
    assert R.nearest_index(10, 4).tolist() == [0, 0, 0, 1, 1, 2, 2, 2, 3, 3]
    assert R.nearest_index(4, 10).tolist() == [0, 2, 5, 7]
    assert R.nearest_index(7, 7).tolist() == list(range(7))
    m = (np.random.default_rng(5).random((37, 53)) < 0.3).astype(np.uint8)
    for k in (1, 3, 5, 15, 31):
        coast, dil, n_water, n_coast = R.dilate_diff(m, k)
        assert coast.max() <= 1 and int((coast == 255).sum()) == 0, "dilated - mask wrapped"
        assert np.array_equal(dil, np.maximum(dil, m)) and n_water == int(m.sum()) and n_coast == int(dil.sum()) - n_water
    assert R.dilate_diff(m, 1)[0].sum() == 0
    one = np.zeros((9, 9), np.uint8)
    one[4, 4] = 1
    assert np.array_equal(R.dilate_diff(one, 5)[1][2:7, 2:7], R.ellipse(5))
    z = np.array([[[[1, 1, 9, 9], [np.nan, 1, 9, 9]], [[1, np.nan, 9, 9], [0, 2, 9, 9]]]], dtype=np.float32)      # one 2 x 2 tile
    assert R.argmax_stitch(z, [(0, 0)], 0, 2, 2, 2).tolist() == [[0, 0], [1, 1]]


def _cyclic_equal(got, want):
    got, want = [tuple(p) for p in got], [tuple(p) for p in want]
    if len(got) != len(want):
        return False
    for seq in (want, want[::-1]):
        for s in range(len(seq)):
            if got == seq[s:] + seq[:s]:
                return True
    return False


@pytest.mark.parametrize("x0,y0,w,h", [(3, 2, 6, 4), (0, 0, 2, 2), (5, 1, 2, 7), (0, 3, 12, 2)])
def test_contour_of_a_filled_rectangle_is_its_four_corners(x0, y0, w, h):
    P = _predict()
    m = np.zeros((10, 12), np.uint8)
    m[y0:y0 + h, x0:x0 + w] = 1
    cs = P.trace_external_contours(m)
    assert len(cs) == 1
    x1, y1 = x0 + w - 1, y0 + h - 1
    assert _cyclic_equal(cs[0].tolist(), [(x0, y0), (x0, y1), (x1, y1), (x1, y0)]), cs[0].tolist()


def test_contour_small_cases():
    P = _predict()
    m = np.zeros((8, 11), np.uint8)
    assert P.trace_external_contours(m) == []
    m[3, 4] = 1
    cs = P.trace_external_contours(m)
    assert len(cs) == 1 and cs[0].tolist() == [[4, 3]]
    m[:] = 0
    m[5, 2:9] = 1
    cs = P.trace_external_contours(m)
    assert len(cs) == 1 and sorted(map(tuple, cs[0].tolist())) == [(2, 5), (8, 5)]
    m[1:3, 1:4] = 1                                      # a second, separate blob
    assert len(P.trace_external_contours(m)) == 2
    m[:] = 0
    m[1:7, 1:9] = 1
    m[3:5, 3:6] = 0                                      # a hole: external borders only
    cs = P.trace_external_contours(m)
    assert len(cs) == 1 and _cyclic_equal(cs[0].tolist(), [(1, 1), (1, 6), (8, 6), (8, 1)])
    m[:] = 1                                             # mask touching every edge of the image
    cs = P.trace_external_contours(m)
    assert len(cs) == 1 and _cyclic_equal(cs[0].tolist(), [(0, 0), (0, 7), (10, 7), (10, 0)])
    ring = np.zeros((30, 30), np.uint8)
    ring[2:28, 2:28] = 1
    ring[3:27, 3:27] = 0                                 # one-pixel wall
    ring[10:14, 10:14] = 1                               # island inside the hole: not a top-level component
    assert len(P.trace_external_contours(ring)) == 1


def _dist_to_polygon(pts, poly):
    pts, poly = np.asarray(pts, float), np.asarray(poly, float)
    best = np.full(len(pts), np.inf)
    for a, b in zip(poly, np.roll(poly, -1, axis=0)):
        ab = b - a
        den = float(ab @ ab)
        t = np.clip(((pts - a) @ ab) / den, 0, 1) if den > 0 else np.zeros(len(pts))
        q = a + t[:, None] * ab
        best = np.minimum(best, np.hypot(*(pts - q).T))
    return best


def test_contour_and_polygon_on_a_digital_disc_ring():
    P = _predict()
    yy, xx = np.mgrid[:100, :100]
    d = np.hypot(yy - 50, xx - 50)
    m = ((d <= 40) & (d >= 34)).astype(np.uint8)
    cs = P.trace_external_contours(m)
    assert len(cs) == 1 and len(cs[0]) > 10
    pad = np.pad(m, 1)
    for x, y in cs[0].tolist():
        assert m[y, x] == 1 and pad[y:y + 3, x:x + 3].min() == 0, (x, y)      # a mask pixel with a background 8-neighbour
    assert np.hypot(cs[0][:, 0] - 50, cs[0][:, 1] - 50).min() > 38.5          # the OUTER border, not the hole's
    per = P.arc_length(cs[0], True)
    assert 2 * np.pi * 38 < per < 2 * np.pi * 40 * 1.12
    eps = 0.002 * per
    poly = P.approx_poly_dp(cs[0], eps, True)
    assert 4 <= len(poly) <= len(cs[0])
    assert {tuple(p) for p in poly.tolist()} <= {tuple(p) for p in cs[0].tolist()}
    assert _dist_to_polygon(cs[0], poly).max() <= eps + 1
    coarse = P.approx_poly_dp(cs[0], 5.0, True)
    assert len(coarse) < len(poly) and _dist_to_polygon(cs[0], coarse).max() <= 5.0 + 1
    line = np.array([[0, 0], [5, 0], [10, 1], [20, 0]])
    assert P.approx_poly_dp(line, 1.5, closed=False).tolist() == [[0, 0], [20, 0]]
    assert P.coastlines_from_mask(m) == [poly.tolist()]
    assert P.coastlines_from_mask(np.pad(np.ones((3, 3), np.uint8), 2)) == []        # 4 points: dropped by the reference's > 10 filter


def test_save_extraction_result_round_trip(tmp_path):
    P = _predict()
    rng = np.random.default_rng(2)
    water = (rng.random((21, 34)) < 0.4).astype(np.uint8)
    coast = R.dilate_diff(water, 5)[0]
    result = {"image_path": "/somewhere/scene_07.tif", "image_size": (34, 21), "water_mask": water, "coastline_mask": coast,
              "coastlines": [[[1, 2], [3, 4], [5, 6]]], "coastline_count": 1, "dilation_size": 5, "extraction_time": "2026-01-01 00:00:00"}
    P.save_extraction_result(result, str(tmp_path / "out"))
    P.CoastlineExtractor.save_extraction_result(result, str(tmp_path / "out"))       # the reference calls it as a method
    assert np.array_equal(np.array(Image.open(tmp_path / "out" / "scene_07_water_mask.png")), water * 255)
    assert np.array_equal(np.array(Image.open(tmp_path / "out" / "scene_07_coastline_mask.png")), coast * 255)
    doc = json.load(open(tmp_path / "out" / "scene_07_coastlines.json", encoding="utf-8"))
    assert set(doc) == {"image_path", "image_size", "coastlines", "coastline_count", "dilation_size", "extraction_time"}
    assert doc["image_size"] == [34, 21] and doc["coastlines"] == result["coastlines"] and doc["coastline_count"] == 1
