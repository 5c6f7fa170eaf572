"""GPU: the exact distance transform and its statistics (csrc/edt.hip, boundary.py) against the brute-force table and the numpy
restatements of tests/edt_ref.py and boundary.py.  np.array_equal everywhere, bit-equal float64 sums: there is no tolerance.

Shapes at which the kernels change plan, each taken at -1 / 0 / +1 (PLAN_SHAPES):
  w = 64, 128        the row pass scans a row in chunks of 64 lanes and carries the nearest feature from chunk to chunk
  h = 8, 16          the column pass reads 8 rows of g ahead of the row it works on
  n w = 129          a wave of the column pass takes 64 adjacent columns, across the images of a batch
  n h > 65536        the row pass strides its grid (4 rows per block, at most 16384 blocks)
  h w = 1024         the statistics' chunk;  h w = 63 / 64 / 65 x 1024: the 64 lanes over the chunk sums
"""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import coastline_ref as CR
import edt_ref as E
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

PLAN_SHAPES = [(5, w) for w in (63, 64, 65, 127, 128, 129)] + [(h, 3) for h in (7, 8, 9, 15, 16, 17)]
STATS_SHAPES = ((1, 1023), (32, 32), (25, 41), (252, 256), (256, 256), (257, 256))


def _boundary():
    return importlib.import_module("eusipco-2026-robust-unet_amd.boundary")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ the transform
def test_every_case_equals_the_brute_force_table():
    B = _boundary()
    for name, m, inv in E.cases():
        got = B.distance_transform_sq(m, invert=inv, device=DEV)
        assert got.dtype == np.int32 and got.shape == m.shape and np.array_equal(got, E.truth(m, inv)), name
    far = B.distance_transform_sq(E.contents(65, 67)["corner 00"], device=DEV)
    assert far[64, 66] == 64 * 64 + 66 * 66
    assert (B.distance_transform_sq(np.zeros((65, 67), np.uint8), device=DEV) == E.NONE).all()
    assert (B.distance_transform_sq(np.zeros((65, 67), np.uint8), invert=True, device=DEV) == 0).all()


@pytest.mark.parametrize("h,w", [(1, 300), (300, 1), (64, 64), (65, 67)] + PLAN_SHAPES)
def test_contents_on_lines_and_plan_shapes(h, w):
    B = _boundary()
    for name, m in E.contents(h, w, seed=h * 7 + w).items():
        for inv in (False, True):
            got = B.distance_transform_sq(m, invert=inv, device=DEV)
            assert np.array_equal(got, B.distance_transform_sq_host(m, invert=inv)), (name, inv)


@pytest.mark.parametrize("density", (0.5, 0.01, 0.001))
def test_random_96x130(density):
    B = _boundary()
    m = (np.random.default_rng(int(density * 1000)).random((96, 130)) < density).astype(np.uint8)
    m[95, 0] |= density < 0.01                           # the sparsest mask keeps at least one feature
    want = B.distance_transform_sq_host(m)
    got = B.distance_transform_sq(m, device=DEV)
    assert np.array_equal(got, want)
    if density < 0.1:                                    # the brute-force table is [h w, features]
        assert np.array_equal(got, E.truth(m))
    assert np.array_equal(B.distance_transform_sq(m, invert=True, device=DEV), B.distance_transform_sq_host(m, invert=True))
    again = B.distance_transform_sq(m, device=DEV)
    assert got.tobytes() == again.tobytes()              # two runs, the same bytes


def test_batches_strides_and_tensors():
    B = _boundary()
    c = E.contents(37, 43, seed=11)
    batch = np.stack([c["random 0.5"], c["no feature"], c["random 0.05"]])         # 3 x 43 = 129 columns: waves that span two images
    want = np.stack([E.truth(m) for m in batch])
    assert (want[1] == E.NONE).all()
    assert np.array_equal(B.distance_transform_sq(batch, device=DEV), want)
    assert np.array_equal(B.distance_transform_sq(batch != 0, device=DEV), want)                          # bool
    t = B.distance_transform_sq(_dev(batch), as_tensor=True, device=DEV)
    assert t.is_cuda and t.dtype == torch.int32 and np.array_equal(t.cpu().numpy(), want)
    # rows and images strided: a crop of a larger buffer, read where it is
    big = np.random.default_rng(2).integers(0, 2, (3, 50, 64), dtype=np.uint8)
    big[:, 4:41, 9:52] = batch
    crop = _dev(big)[:, 4:41, 9:52]
    assert not crop.is_contiguous() and crop.stride(1) == 64
    assert np.array_equal(B.distance_transform_sq(crop, device=DEV), want)
    assert np.array_equal(B.distance_transform_sq(crop[0], device=DEV), want[0])
    # strides that a row stride cannot express: every second column, a transposed view
    wide = _dev(np.repeat(batch, 2, axis=2))[:, :, ::2]
    assert wide.stride(2) == 2 and np.array_equal(B.distance_transform_sq(wide, device=DEV), want)
    turned = _dev(np.ascontiguousarray(batch[0].T)).T
    assert not turned.is_contiguous() and np.array_equal(B.distance_transform_sq(turned, device=DEV), want[0])
    assert np.array_equal(B.distance_transform_sq(_dev(batch[0] != 0), device=DEV), want[0])              # bool tensor


@pytest.mark.parametrize("shape", ((2, 32768), (32768, 2)))
def test_integer_range(shape):
    """a single feature at one end of the longest line: d2 up to 32767^2 + 1"""
    B = _boundary()
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    for corner in ((0, 0), (shape[0] - 1, shape[1] - 1)):
        m = np.zeros(shape, np.uint8)
        m[corner] = 1
        got = B.distance_transform_sq(m, device=DEV)
        assert np.array_equal(got, (yy - corner[0]) ** 2 + (xx - corner[1]) ** 2) and got.max() == 32767 ** 2 + 1
    with pytest.raises(ValueError):
        B.distance_transform_sq(np.zeros((1, 32769), np.uint8), device=DEV)


def test_more_rows_than_one_grid_pass():
    B = _boundary()
    m = (np.random.default_rng(4).random((3, 21846, 1)) < 0.001).astype(np.uint8)                       # 65538 rows
    m[1] = 0
    got = B.distance_transform_sq(m, device=DEV)
    assert np.array_equal(got, B.distance_transform_sq_host(m)) and (got[1] == E.NONE).all() and got[0].max() > 0


def test_host_route_in_a_child_process_gives_the_same_arrays(tmp_path):
    B = _boundary()
    c = E.contents(65, 67, seed=1)
    masks = np.stack([c["random 0.5"], c["random 0.05"], c["no feature"], c["two ends"]])
    path = str(tmp_path / "host.npz")
    np.save(str(tmp_path / "masks.npy"), masks)
    code = ("import importlib, sys, numpy as np\n"
            "B = importlib.import_module('eusipco-2026-robust-unet_amd.boundary')\n"
            "m = np.load(sys.argv[1])\n"
            "dev = B.coastline_deviation(m[0], m[1])\n"
            "np.savez(sys.argv[2], d2=B.distance_transform_sq(m), inv=B.distance_transform_sq(m, invert=True), mean=dev['pred_to_true']['mean'],\n"
            "         assd=dev['assd'], bf1=B.boundary_scores(m[0], m[1])['bf1'])\n")
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path / "masks.npy"), path], cwd=ROOT, env=dict(os.environ, RUNET_NO_DEVICE_EDT="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    host = np.load(path)
    assert np.array_equal(B.distance_transform_sq(masks, device=DEV), host["d2"])
    assert np.array_equal(B.distance_transform_sq(masks, invert=True, device=DEV), host["inv"])
    dev = B.coastline_deviation(masks[0], masks[1], device=DEV)
    assert dev["pred_to_true"]["mean"] == float(host["mean"]) and dev["assd"] == float(host["assd"])
    assert B.boundary_scores(masks[0], masks[1], device=DEV)["bf1"] == float(host["bf1"])


# ------------------------------------------------------------------------------------------------ the statistics
@pytest.mark.parametrize("h,w", STATS_SHAPES + ((65, 67),))
def test_stats_equal_the_restatement(h, w):
    B = _boundary()
    rng = np.random.default_rng(h * w)
    masks = np.stack([(rng.random((h, w)) < 0.02).astype(np.uint8), np.zeros((h, w), np.uint8), (rng.random((h, w)) < 0.3).astype(np.uint8)])
    masks[0, h - 1, w - 1] = 1
    d2 = B.distance_transform_sq(masks, as_tensor=True, device=DEV)
    d2_host = d2.cpu().numpy()
    assert (d2_host[1] == E.NONE).all()                  # an image of NONE pixels among the three
    select = (rng.random((3, h, w)) < 0.5).astype(np.uint8) * 3
    worst = int(d2_host[0].max())
    for sel in (None, select):
        for tol in ([], [0, 1, 4, worst - 1, worst, worst + 1, 25, 2 ** 31 - 2]):
            counts, sums = B._stats_device(d2, None if sel is None else _dev(sel), tol)
            want_counts, want_sums = E.stats(d2_host, sel, tol)
            assert counts.dtype == np.int64 and np.array_equal(counts, want_counts), (sel is None, tol)
            assert sums.tobytes() == want_sums.tobytes(), (sel is None, tol, sums, want_sums)
            host_counts, host_sums = B._stats_host(d2_host, sel, tol)
            assert np.array_equal(host_counts, want_counts) and host_sums.tobytes() == want_sums.tobytes()
    assert want_counts[1, 1] == want_counts[1, 0] > 0 and want_counts[1, 2] == 0 and want_sums[1] == 0.0
    at = B._stats_device(d2, None, [worst - 1, worst])[0][0]
    assert at[5] == at[0] == h * w and at[4] < at[0]     # <= at the tolerance, not <


# ------------------------------------------------------------------------------------------------ the product
@pytest.fixture(scope="module")
def extraction(pkg):
    """an untrained UNet calls a whole scene one class; its head's bias is moved so that the median pixel of this scene is a tie, which
    makes the predicted water mask a noisy half of the scene - a coastline everywhere, a few pixels from the true one in places"""
    torch.manual_seed(3)
    net = pkg.UNet(3, 2).to(DEV).eval()
    scene, water = CR.synthetic_scene(128, 128, seed=6)
    with torch.no_grad():
        z = net(CR.normalize_u8(scene)[None].to(DEV))
        net.final.bias[1] += (z[:, 0] - z[:, 1]).median()
    ex = pkg.CoastlineExtractor(model=net, device=DEV, input_size=128)
    return ex.extract_coastline_from_image(scene, dilation_size=5), water


def _on_the_host(fn):
    os.environ["RUNET_NO_DEVICE_EDT"] = "1"              # read at call time
    try:
        return fn()
    finally:
        del os.environ["RUNET_NO_DEVICE_EDT"]


def test_scores_of_an_extraction_equal_the_host_route(pkg, extraction):
    B, P = _boundary(), importlib.import_module("eusipco-2026-robust-unet_amd.predict")
    result, water = extraction
    true_band = P.dilate_diff(_dev((water != 0).astype(np.uint8)), 5)[0].cpu().numpy()
    assert result["coastline_mask"].any() and true_band.any()
    dev = pkg.coastline_deviation(result["coastline_mask"], true_band, tolerances=(1, 2, 5), pixel_size=10.0, device=DEV)
    assert dev == _on_the_host(lambda: B.coastline_deviation(result["coastline_mask"], true_band, tolerances=(1, 2, 5), pixel_size=10.0))
    assert dev["pred_to_true"]["count"] == int(result["coastline_mask"].sum()) and dev["hausdorff"] >= dev["assd"] > 0.0
    # and from the transform's definition: the mean over the predicted band of the root of the brute-force distance to the true band
    d2 = B.distance_transform_sq_host(true_band)[result["coastline_mask"] != 0]
    assert dev["pred_to_true"]["max"] == 10.0 * np.sqrt(d2.max()) and dev["pred_to_true"]["within"][2]["count"] == int((d2 <= 4).sum())
    assert dev["pred_to_true"]["rms"] == 10.0 * np.sqrt(int(d2.sum()) / d2.size)
    for tol in (0, 2, 5):
        got = pkg.boundary_scores(result["water_mask"], water, tolerance=tol, device=DEV)
        assert got == _on_the_host(lambda: B.boundary_scores(result["water_mask"], water, tolerance=tol)), tol
        assert got == pkg.boundary_scores(_dev(result["water_mask"]), _dev(water) != 0, tolerance=tol, device=DEV)
    whole = pkg.evaluate_coastline(result, water, tolerances=(1, 2, 5), boundary_tolerance=2, pixel_size=10.0, device=DEV)
    assert whole == {"deviation": dev, "boundary": pkg.boundary_scores(result["water_mask"], water, 2, device=DEV), "dilation_size": 5}
    assert whole == _on_the_host(lambda: B.evaluate_coastline(result, water, pixel_size=10.0, device=DEV))
    on_device = dict(result, water_mask=_dev(result["water_mask"]), coastline_mask=_dev(result["coastline_mask"]))
    assert whole == pkg.evaluate_coastline(on_device, _dev(water), pixel_size=10.0, device=DEV)
    with pytest.raises(ValueError):
        pkg.evaluate_coastline(result, water[:64], device=DEV)


def test_evaluate_model_with_a_boundary_tolerance(pkg, oracle):
    B = _boundary()
    net = pkg.RobustUNet(3, 1, 16)
    net.load_state_dict(oracle.init_state(3, 1, 16, seed=7, perturb_bn=True))
    net.to(DEV)
    x, y = pkg.synthetic_batch(4, 64, seed=2)
    data = [(x[:2], y[:2]), (x[2:], y[2:])]
    ev = pkg.ModelEvaluator(torch.device(DEV))
    plain = ev.evaluate_model(net, data)
    scored = ev.evaluate_model(net, data, boundary_tolerance=2)
    assert set(scored) == set(plain) | {"mean_boundary_iou", "mean_bf1"}
    assert all(scored[k] == plain[k] for k in plain if k != "avg_inference_time")
    with torch.no_grad():
        pred = torch.cat([net(xi.to(DEV)) for xi, _ in data]).cpu().numpy()[:, 0] > 0.5
    per_image = _on_the_host(lambda: [B.boundary_scores(p, t, tolerance=2) for p, t in zip(pred, y.numpy()[:, 0] > 0.5)])
    assert scored["mean_boundary_iou"] == np.mean([s["boundary_iou"] for s in per_image])
    assert scored["mean_bf1"] == np.mean([s["bf1"] for s in per_image])
    with pytest.raises(ValueError):
        ev.evaluate_model(net, data, boundary_tolerance=1.5)
