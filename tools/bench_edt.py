"""The exact distance transform and the coastline scores (boundary.py, csrc/edt.hip) on one MI355X, beside scipy on the same machine's host.

Per size (512, 4096, 10980: a tile, a large crop, a Sentinel-2 scene) and per input (the coastline band of a smooth synthetic water mask;
a 50 % random mask):
  * runet_edt_sq_u8 and runet_edt_stats with device events around back-to-back calls on buffers allocated before, each with the bytes it
    must move over its time.  Bytes from the shapes (include/runet_hip.h): the transform reads 1 mask byte, writes d2 twice and reads it
    once in the row pass, reads and writes it once in the column pass = 21 bytes per pixel, not counting the envelope's stack, which
    depends on the data; the statistics read 4 bytes of d2 and 1 of select per pixel;
  * distance_transform_sq end to end, numpy in -> numpy out: upload of the mask, the transform, download of d2 (host clock, synchronised);
  * scipy.ndimage.distance_transform_edt on the same mask on the host, where scipy is installed, and the device result compared with
    rint(scipy^2) at the size that is timed;
  * evaluate_coastline end to end on host masks (a true water mask, a prediction a few pixels off): uploads, the true band, six
    transforms in three batched calls, the statistics, the downloads.

Not a bench line of the contract (bench.py measures the Robust U-Net training metric).
  python tools/bench_edt.py [--sizes 512,4096,10980] [--reps 5] [--scipy-max 10980] [--out FILE]
"""
import argparse
import ctypes
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B = importlib.import_module("eusipco-2026-robust-unet_amd.boundary")
P = importlib.import_module("eusipco-2026-robust-unet_amd.predict")
L = importlib.import_module("eusipco-2026-robust-unet_amd._lib")
ops = importlib.import_module("eusipco-2026-robust-unet_amd.ops")
DEV = torch.device("cuda:0")
LINES = []


def say(s):
    LINES.append(s)
    print(s, flush=True)


def smooth_water(size, seed=0, shift=0):
    """uint8 [size, size]: a sum of a few long waves above its mean = water; shift moves the field by that many pixels"""
    rng = np.random.default_rng(seed)
    y = (np.arange(size, dtype=np.float32) + shift)[:, None]
    x = (np.arange(size, dtype=np.float32) + shift)[None, :]
    f = np.zeros((size, size), np.float32)
    for _ in range(6):
        ky, kx = rng.uniform(-1, 1, 2) * (2 * np.pi * rng.integers(1, 6) / size)
        f += np.float32(rng.uniform(0.3, 1.0)) * np.sin(np.float32(ky) * y + np.float32(kx) * x + np.float32(rng.uniform(0, 6.28)))
    return (f > 0).astype(np.uint8)


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    fn()
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def one_input(name, mask, other, reps, with_scipy, row):
    """mask: the features; other: the pixels the statistics select"""
    h, w = mask.shape
    px = h * w
    m, sel = torch.from_numpy(mask).to(DEV), torch.from_numpy(other).to(DEV)
    d2 = torch.empty((1, h, w), device=DEV, dtype=torch.int32)
    ws = B._workspace(1, h, w, DEV)
    counts = torch.empty((1, 7), device=DEV, dtype=torch.int64)
    sums = torch.empty(1, device=DEV, dtype=torch.float64)
    tol = (ctypes.c_int * 3)(1, 4, 25)

    def edt():
        L.check(L.lib.runet_edt_sq_u8(m.data_ptr(), 1, h, w, w, px, 0, d2.data_ptr(), ws.data_ptr(), ws.numel(), ops.stream()))

    def stats():
        L.check(L.lib.runet_edt_stats(d2.data_ptr(), sel.data_ptr(), 1, h, w, tol, 3, counts.data_ptr(), sums.data_ptr(), ws.data_ptr(), ws.numel(),
                                      ops.stream()))

    t_edt = timed(edt, reps)
    t_stats = timed(stats, reps)
    t_e2e = wall(lambda: B.distance_transform_sq(mask, device=DEV), max(1, reps // 2))
    r = {"edt_ms": t_edt, "edt_gbs": 21 * px / t_edt / 1e6, "stats_ms": t_stats, "stats_gbs": 5 * px / t_stats / 1e6, "edt_end_to_end_ms": t_e2e,
         "features": int(mask.sum())}
    line = (f"  {name:14s} runet_edt_sq_u8 {t_edt:9.3f} ms ({r['edt_gbs']:7.1f} GB/s of 21 B/px)   runet_edt_stats {t_stats:8.3f} ms "
            f"({r['stats_gbs']:7.1f} GB/s of 5 B/px)   numpy -> numpy {t_e2e:9.2f} ms")
    if with_scipy:
        from scipy import ndimage
        t0 = time.perf_counter()
        ref = ndimage.distance_transform_edt(mask == 0)
        r["scipy_ms"] = (time.perf_counter() - t0) * 1e3
        got = B.distance_transform_sq(mask, device=DEV)
        r["equals_scipy"] = bool(np.array_equal(got, np.rint(ref * ref).astype(np.int64)))
        line += f"   scipy {r['scipy_ms']:10.1f} ms (x{r['scipy_ms'] / t_e2e:6.1f} of numpy -> numpy; equal: {r['equals_scipy']})"
    say(line)
    row[name] = r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,4096,10980")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scipy-max", type=int, default=10980, help="largest size at which scipy is run beside the device")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    try:
        import scipy  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    say(f"device {torch.cuda.get_device_name(0)}; scipy {'present' if have_scipy else 'absent'}; reps {a.reps}")
    res = {}
    for size in (int(s) for s in a.sizes.split(",")):
        say(f"{size} x {size}")
        row = res[size] = {}
        water, pred = smooth_water(size, 0), smooth_water(size, 0, shift=3)
        band = P.dilate_diff(torch.from_numpy(water).to(DEV), 5)[0].cpu().numpy()
        pred_band = P.dilate_diff(torch.from_numpy(pred).to(DEV), 5)[0].cpu().numpy()
        scipy_here = have_scipy and size <= a.scipy_max
        one_input("coastline band", band, pred_band, a.reps, scipy_here, row)
        rnd = (np.random.default_rng(1).random((size, size)) < 0.5).astype(np.uint8)
        one_input("random 50 %", rnd, pred_band, a.reps, scipy_here, row)
        result = {"water_mask": pred, "coastline_mask": pred_band, "dilation_size": 5}
        t = wall(lambda: B.evaluate_coastline(result, water, device=DEV), max(1, a.reps // 2))
        score = B.evaluate_coastline(result, water, device=DEV)
        row["evaluate_coastline_ms"] = t
        say(f"  evaluate_coastline end to end {t:9.2f} ms   (assd {score['deviation']['assd']:.3f} px, hausdorff {score['deviation']['hausdorff']:.3f} px, "
            f"bf1 {score['boundary']['bf1']:.4f}, boundary IoU {score['boundary']['boundary_iou']:.4f})")
        if "scipy_ms" in row["coastline band"]:
            say(f"  six scipy transforms of the band's cost: {6 * row['coastline band']['scipy_ms']:10.1f} ms (derived: 6 x the one measured)")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"lines": LINES, "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
