"""GPU: connected-component labelling, areas, the table and the area filter (csrc/ccl.hip, components.py) against the flood fill and the
restatements of tests/ccl_ref.py and components.py, and the extractor's cleanup.  np.array_equal everywhere: there is no tolerance.

Shapes at which the kernels change plan, each taken at -1 / 0 / +1 (ccl_ref.PLAN_SHAPES and RAGGED):
  h, w = 64, 128     a block labels a 64 x 64 tile in LDS (a wave per row); from 65 on a border row / column exists and the seam pass runs
  131 x 137          3 x 3 tiles, ragged in both axes: four tile corners, each with both diagonal pairs
  h w = 1024, 4096   the filter's and the table's chunk of consecutive pixels; the areas' 16 rounds of 64 per wave
No launch strides its grid (a block per tile, per chunk, or per 256 border pixels), so there is no grid cap to cross.
"""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ccl_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _components():
    return importlib.import_module("eusipco-2026-robust-unet_amd.components")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ labels
def test_every_case_equals_the_flood_fill_and_the_host_restatement():
    C = _components()
    for name, m, connectivity, invert in R.cases():
        got = C.label_components(m, connectivity=connectivity, invert=invert, device=DEV)
        assert got.dtype == np.int32 and got.shape == m.shape and np.array_equal(got, R.truth(name, m, connectivity, invert)), name
        assert np.array_equal(got, C.label_components_host(m, connectivity=connectivity, invert=invert)), name


def test_two_runs_give_the_same_bytes():
    C = _components()
    m = R.contents(*R.RAGGED, seed=9)["random 0.593"]
    for connectivity in (4, 8):
        assert C.label_components(m, connectivity, device=DEV).tobytes() == C.label_components(m, connectivity, device=DEV).tobytes()


def test_batches_strides_and_tensors():
    C = _components()
    batch = R.batch()
    for connectivity in (4, 8):
        want = np.stack([R.flood_labels(m, connectivity) for m in batch])
        assert np.array_equal(C.label_components(batch, connectivity, device=DEV), want)
        for i in range(3):                               # the batch equals three single calls
            assert np.array_equal(C.label_components(batch[i], connectivity, device=DEV), want[i])
        assert np.array_equal(C.label_components(batch != 0, connectivity, device=DEV), want)                     # bool
        t = C.label_components(_dev(batch), connectivity, as_tensor=True, device=DEV)
        assert t.is_cuda and t.dtype == torch.int32 and np.array_equal(t.cpu().numpy(), want)
        # rows and images strided: a crop of a larger buffer, read where it is
        big = np.random.default_rng(2).integers(0, 2, (3, 80, 96), dtype=np.uint8)
        big[:, 4:74, 9:84] = batch
        crop = _dev(big)[:, 4:74, 9:84]
        assert not crop.is_contiguous() and crop.stride(1) == 96
        assert np.array_equal(C.label_components(crop, connectivity, device=DEV), want)
        assert np.array_equal(C.label_components(crop[1], connectivity, device=DEV), want[1])
        inv = np.stack([R.flood_labels(m, connectivity, invert=True) for m in batch])
        assert np.array_equal(C.label_components(crop, connectivity, invert=True, device=DEV), inv)
    # strides that a row stride cannot express: every second column, a transposed view
    wide = _dev(np.repeat(batch, 2, axis=2))[:, :, ::2]
    assert wide.stride(2) == 2 and np.array_equal(C.label_components(wide, device=DEV), want)
    turned = _dev(np.ascontiguousarray(batch[0].T)).T
    assert not turned.is_contiguous() and np.array_equal(C.label_components(turned, device=DEV), want[0])
    with pytest.raises(ValueError):
        C.label_components(np.zeros((1, 32769), np.uint8), device=DEV)


# ------------------------------------------------------------------------------------------------ areas, frame, table
def _masks_for_tables():
    big = R.contents(*R.RAGGED, seed=3)
    return {"specks": R.specks(), "ragged random 0.407": big["random 0.407"], "ragged ring": big["ring and island"], "ragged u": big["u"],
            "ragged empty": big["empty"], "row 1 x 300": R.contents(1, 300, seed=1)["random 0.5"], "64 x 64": R.contents(64, 64)["random 0.05"]}


@pytest.mark.parametrize("connectivity", (4, 8))
def test_areas_frame_and_table_equal_numpy(connectivity):
    C = _components()
    for name, m in _masks_for_tables().items():
        labels_host = R.flood_labels(m, connectivity)
        labels = _dev(labels_host[None])
        areas, frame = C._areas_device(labels)
        # numpy on the restated labels: bincount for the areas, min and max of the coordinates for the frame bits and the boxes
        h, w = m.shape
        ys, xs = np.nonzero(labels_host)
        roots = labels_host[ys, xs].astype(np.int64) - 1
        want_areas = np.bincount(roots, minlength=h * w).astype(np.int32).reshape(h, w)
        assert np.array_equal(areas.cpu().numpy()[0], want_areas), name
        lo_x, lo_y = np.full(h * w, w), np.full(h * w, h)
        hi_x, hi_y = np.full(h * w, -1), np.full(h * w, -1)
        np.minimum.at(lo_x, roots, xs), np.minimum.at(lo_y, roots, ys), np.maximum.at(hi_x, roots, xs), np.maximum.at(hi_y, roots, ys)
        live = want_areas.reshape(-1) != 0
        want_frame = (live * ((lo_y == 0) * 1 + (hi_y == h - 1) * 2 + (lo_x == 0) * 4 + (hi_x == w - 1) * 8)).astype(np.uint8).reshape(h, w)
        assert np.array_equal(frame.cpu().numpy()[0], want_frame), name
        assert np.array_equal(want_areas, R.areas_frame(labels_host)[0]) and np.array_equal(want_frame, R.areas_frame(labels_host)[1]), name
        idx = np.flatnonzero(live)
        rows = np.stack([idx + 1, want_areas.reshape(-1)[idx], lo_x[idx], lo_y[idx], hi_x[idx], hi_y[idx], want_frame.reshape(-1)[idx],
                         np.zeros_like(idx)], axis=1).astype(np.int32)
        assert np.array_equal(rows, R.table(labels_host)), name
        ws = C._workspace(1, h, w, DEV)
        k = len(rows)
        L, ops = (importlib.import_module("eusipco-2026-robust-unet_amd." + mod) for mod in ("_lib", "ops"))
        for capacity in sorted({max(k - 1, 0), k, k + 1}):
            count = torch.full((1,), -5, device=DEV, dtype=torch.int64)
            table = torch.full((1, capacity + 2, 8), -77, device=DEV, dtype=torch.int32)       # a sentinel, and two rows past the capacity
            L.check(L.lib.runet_ccl_table(labels.data_ptr(), areas.data_ptr(), frame.data_ptr(), 1, h, w, capacity, count.data_ptr(),
                                          table.data_ptr() if capacity else None, ws.data_ptr(), ws.numel(), ops.stream()))
            got = table.cpu().numpy()[0]
            kept = min(k, capacity)
            assert int(count.item()) == k and np.array_equal(got[:kept], rows[:kept]) and (got[kept:] == -77).all(), (name, capacity)


def test_water_bodies_of_a_batch():
    C = _components()
    batch = R.batch()
    for connectivity in (4, 8):
        got = C.water_bodies(batch, connectivity=connectivity, pixel_size=10.0, device=DEV)
        assert len(got) == 3
        for i in range(3):
            rows = R.table(R.flood_labels(batch[i], connectivity)).tolist()
            assert [(b["label"], b["area"]) + b["bbox"] for b in got[i]] == [tuple(r[:6]) for r in rows]
            assert [sum(on << bit for bit, on in enumerate(b["touches_frame"].values())) for b in got[i]] == [r[6] for r in rows]
            assert all(b["area_units"] == 100.0 * b["area"] for b in got[i])
    assert C.water_bodies(np.zeros((5, 7), np.uint8), device=DEV) == []
    one = C.water_bodies(R.specks(), device=DEV)
    assert [b["area"] for b in one] == [5, 1, 2, 393, 6, 45] and one[0]["touches_frame"] == {"top": True, "bottom": False, "left": False, "right": False}


# ------------------------------------------------------------------------------------------------ the filter
def test_filter_and_clean_water_mask_equal_the_restatement():
    C = _components()
    for case, m, min_water, min_land, connectivity, keep in R.clean_cases():
        got, info = C.clean_water_mask(m, min_water, min_land, connectivity=connectivity, keep_frame=keep, device=DEV)
        want, counts = R.clean(m, min_water, min_land, connectivity, keep)
        assert got.dtype == np.uint8 and np.array_equal(got, want) and [info[k] for k in C.INFO_KEYS] == counts.tolist(), case


def test_clean_water_mask_batches_tensors_and_untouched_bytes():
    C = _components()
    batch = R.batch()
    got, info = C.clean_water_mask(batch, 9, 6, connectivity=4, device=DEV)
    for i in range(3):
        want, counts = R.clean(batch[i], 9, 6, 4, True)
        assert np.array_equal(got[i], want) and [info[i][k] for k in C.INFO_KEYS] == counts.tolist()
    assert sum(d["removed_water_pixels"] + d["filled_land_pixels"] for d in info) > 0
    src = _dev(batch)
    t, info_t = C.clean_water_mask(src, 9, 6, connectivity=4, as_tensor=True, device=DEV)
    assert t.is_cuda and t.data_ptr() != src.data_ptr() and np.array_equal(src.cpu().numpy(), batch) and np.array_equal(t.cpu().numpy(), got)
    assert info_t == info
    # the bytes of what is kept stay as they came: 7 stays 7, removed water becomes 0, filled land 1
    m = R.specks() * 7
    got, _ = C.clean_water_mask(m, 7, 5, device=DEV)
    want, _ = R.clean(m, 7, 5, 8, True)
    assert np.array_equal(got, want) and set(np.unique(got)) == {0, 1, 7}
    # the low-level call leaves mask_out alone outside the selected components
    labels = _dev(R.flood_labels(R.specks(), 8)[None])
    areas, frame = C._areas_device(labels)
    out = torch.full((1, 40, 44), 9, device=DEV, dtype=torch.uint8)
    counts = torch.full((1, 2), -1, device=DEV, dtype=torch.int64)
    C._filter_device(labels, areas, frame, 6, True, 200, out, counts)
    assert counts.cpu().tolist() == [[2, 3]]
    want = np.full((40, 44), 9, np.uint8)
    want[3, 3] = want[5, 20] = want[6, 21] = 200
    assert np.array_equal(out.cpu().numpy()[0], want)


def test_host_route_in_a_child_process_gives_the_same_outputs(tmp_path):
    C = _components()
    masks = np.stack([np.pad(R.specks(), ((0, 30), (0, 31))), R.batch()[0], R.batch()[2]])
    np.save(str(tmp_path / "masks.npy"), masks)
    code = ("import importlib, json, sys, numpy as np\n"
            "C = importlib.import_module('eusipco-2026-robust-unet_amd.components')\n"
            "m = np.load(sys.argv[1])\n"
            "clean, info = C.clean_water_mask(m, 7, 5, connectivity=8)\n"
            "np.savez(sys.argv[2], l8=C.label_components(m), l4=C.label_components(m, connectivity=4, invert=True), clean=clean)\n"
            "json.dump({'info': info, 'bodies': C.water_bodies(m, connectivity=4)}, open(sys.argv[3], 'w'))\n"
            "import torch\n"
            "assert not torch.cuda.is_initialized()\n")
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path / "masks.npy"), str(tmp_path / "host.npz"), str(tmp_path / "host.json")], cwd=ROOT,
                       env=dict(os.environ, RUNET_NO_DEVICE_CCL="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    host = np.load(str(tmp_path / "host.npz"))
    doc = json.load(open(str(tmp_path / "host.json")))
    assert np.array_equal(C.label_components(masks, device=DEV), host["l8"])
    assert np.array_equal(C.label_components(masks, connectivity=4, invert=True, device=DEV), host["l4"])
    clean, info = C.clean_water_mask(masks, 7, 5, connectivity=8, device=DEV)
    assert np.array_equal(clean, host["clean"])
    assert json.loads(json.dumps({"info": info, "bodies": C.water_bodies(masks, connectivity=4, device=DEV)})) == doc


# ------------------------------------------------------------------------------------------------ the extractor
SIZE = 128


def _sea():
    """the right half of the image behind a wavy shore: it runs off the frame, so a hole in it is not enclosed by its shore's contour"""
    yy, xx = np.mgrid[0:SIZE, 0:SIZE]
    return xx >= 64 + np.rint(6 * np.sin(yy / 6.0))


def _scene_probabilities():
    """float32 [128, 128]: the sea with two holes of land (plus signs of 20 pixels), and three specks of 4 x 4 water on the land.  The
    extractor keeps contours of more than 10 vertices: the shore has 114, a plus 16, the band around a speck 12."""
    p = np.where(_sea(), 0.9, 0.1).astype(np.float32)
    for y, x in ((50, 95), (80, 105)):
        p[y - 1:y + 1, x - 3:x + 3] = 0.2
        p[y - 3:y + 3, x - 1:x + 1] = 0.2
    for y, x in ((6, 8), (10, 30), (112, 30)):
        p[y:y + 4, x:x + 4] = 0.8
    return p


@pytest.fixture(scope="module")
def extractor(pkg):
    """a probability model whose answer is replaced by the scene above: the extractor's own threshold, stitch and everything after it run"""
    ex = pkg.CoastlineExtractor(model=pkg.RobustUNet(3, 1, 16), device=DEV, input_size=SIZE)
    prob = _dev(_scene_probabilities())[None, None].contiguous()
    ex._prob = lambda tiles: prob
    return ex


def _same(a, b, skip=("extraction_time",)):
    assert set(a) == set(b)
    for k in a:
        if k in skip:
            continue
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def _count_syncs(monkeypatch, fn):
    """-> (fn's result, the number of host synchronisations it made: synchronize, and .cpu(), .item(), .tolist() of a device tensor)"""
    calls = []
    with monkeypatch.context() as mp:
        real_sync = torch.cuda.synchronize
        mp.setattr(torch.cuda, "synchronize", lambda *a, **k: (calls.append("synchronize"), real_sync(*a, **k))[1])
        for name in ("cpu", "item", "tolist"):
            real = getattr(torch.Tensor, name)
            mp.setattr(torch.Tensor, name, lambda self, *a, _real=real, _name=name, **k: (calls.append(_name) if self.is_cuda else None,
                                                                                        _real(self, *a, **k))[1])
        out = fn()
    return out, len(calls)


def test_extractor_defaults_change_nothing(extractor, monkeypatch):
    image = np.zeros((SIZE, SIZE, 3), np.uint8)
    plain, syncs_plain = _count_syncs(monkeypatch, lambda: extractor.extract_coastline_from_image(image, dilation_size=5))
    named, syncs_named = _count_syncs(monkeypatch, lambda: extractor.extract_coastline_from_image(image, dilation_size=5, min_water_area=0,
                                                                                                 min_land_area=0, connectivity=8))
    _same(plain, named)
    assert "cleanup" not in plain and syncs_plain == syncs_named
    assert np.array_equal(plain["water_mask"], (_scene_probabilities() > 0.5).astype(np.uint8))
    assert plain["coastline_count"] == 1 + 2 + 3           # the shore, the two holes, the three specks


@pytest.mark.parametrize("rule", ("float64", "exact"))
def test_extractor_cleanup_equals_the_host_route(pkg, extractor, monkeypatch, tmp_path, rule):
    C = _components()
    image = np.zeros((SIZE, SIZE, 3), np.uint8)
    monkeypatch.setattr(extractor, "simplify_rule", rule)
    plain, syncs_plain = _count_syncs(monkeypatch, lambda: extractor.extract_coastline_from_image(image, dilation_size=5))
    clean, syncs_clean = _count_syncs(monkeypatch, lambda: extractor.extract_coastline_from_image(image, dilation_size=5, min_water_area=20,
                                                                                                 min_land_area=40, connectivity=8))
    assert syncs_clean <= syncs_plain                       # the four counts ride in the one download
    want_mask, counts = R.clean(plain["water_mask"], 20, 40, 8, True)
    assert np.array_equal(clean["water_mask"], want_mask) and clean["water_pixels"] == int(want_mask.sum())
    assert np.array_equal(want_mask, _sea())             # the sea, whole, and nothing else
    assert clean["cleanup"] == {"removed_water_components": 3, "removed_water_pixels": 48, "filled_land_components": 2, "filled_land_pixels": 40,
                                "min_water_area": 20, "min_land_area": 40, "connectivity": 8}
    assert [clean["cleanup"][k] for k in C.INFO_KEYS] == counts.tolist()
    assert clean["coastline_count"] == 1 and plain["coastline_count"] == 6
    # the band and the contours are those of the cleaned mask, by the extractor's own unchanged steps
    coastlines, band = extractor.extract_coastline_contours(want_mask, 5)
    assert np.array_equal(clean["coastline_mask"], band) and clean["coastlines"] == coastlines
    assert clean["coastline_pixels"] == int(band.sum())
    again, band_again = extractor.extract_coastline_contours(plain["water_mask"], 5, min_water_area=20, min_land_area=40)
    assert again == coastlines and np.array_equal(band_again, band)
    # the numpy route of the filter inside the extractor: the same result
    monkeypatch.setenv("RUNET_NO_DEVICE_CCL", "1")
    _same(extractor.extract_coastline_from_image(image, dilation_size=5, min_water_area=20, min_land_area=40), clean)
    monkeypatch.delenv("RUNET_NO_DEVICE_CCL")
    # thresholds at the areas and one above: 16 and 20 are not < 16 and < 20
    kept = extractor.extract_coastline_from_image(image, dilation_size=5, min_water_area=16, min_land_area=20)
    assert kept["cleanup"]["removed_water_components"] == 0 and kept["cleanup"]["filled_land_components"] == 0
    assert np.array_equal(kept["water_mask"], plain["water_mask"]) and kept["coastlines"] == plain["coastlines"]
    gone = extractor.extract_coastline_from_image(image, dilation_size=5, min_water_area=17, min_land_area=21, output_dir=str(tmp_path))
    assert np.array_equal(gone["water_mask"], want_mask)
    doc = json.load(open(str(tmp_path / "image_coastlines.json")))
    assert doc["cleanup"] == gone["cleanup"] and doc["coastline_count"] == 1
    with pytest.raises(ValueError):
        extractor.extract_coastline_from_image(image, min_water_area=-1)
    with pytest.raises(ValueError):
        extractor.extract_coastline_from_image(image, min_land_area=3, connectivity=6)
