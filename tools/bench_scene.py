"""Scene ingestion (scene.py, csrc/scene_bands.hip) on one MI355X against numpy on the same machine's host, at the size of a Sentinel-2 tile:
a seeded synthetic 6 x 10980 x 10980 scene, uint16 and float32, "water" mode (bands 4, 3, 2).

  * the upload of the raw bands (pageable host memory -> device);
  * every selection pass of runet_band_percentiles (one counting launch + one scan launch), timed with device events inside one call
    (runet_band_percentiles_timed), and runet_band_stretch_u8 with device events around back-to-back calls; each with the bytes it must move
    (from the shapes: a pass reads the three selected planes once; the stretch reads them once and writes 3 bytes per pixel) over its time;
  * the same work in numpy on the host: np.percentile per band, then the reference's stretch expression, then the upload of the uint8 image
    - the path a caller had to take before;
  * the device result is compared with numpy's first, bit for bit, at the size that is timed.

Not a bench line of the contract (bench.py measures the Robust U-Net training metric).
  python tools/bench_scene.py [--size 10980] [--dtypes uint16,float32] [--reps 5] [--out FILE]
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
S = importlib.import_module("eusipco-2026-robust-unet_amd.scene")
L = importlib.import_module("eusipco-2026-robust-unet_amd._lib")
ops = importlib.import_module("eusipco-2026-robust-unet_amd.ops")
DEV = torch.device("cuda:0")
LINES = []


def say(s):
    LINES.append(s)
    print(s, flush=True)


def synthetic(size, dtype, seed=0):
    """6 planes of reflectance-like counts with a nodata block of zeros (a tie run of 8 % of the pixels: p2 sits inside it)"""
    rng = np.random.default_rng(seed)
    a = np.empty((6, size, size), dtype)
    for b in range(6):
        v = rng.integers(200, 9000, (size, size), dtype=np.uint16)
        v[: size * 8 // 100] = 0
        a[b] = v if dtype == np.uint16 else v.astype(np.float32) * np.float32(1e-4)
    return a


def numpy_enhance(a, sel):
    """the reference's "water" enhancement of the selected planes -> (uint8 [H, W, 3], seconds in np.percentile, seconds in the stretch)"""
    out = np.zeros(a.shape[1:] + (3,), a.dtype)
    t_pct = t_str = 0.0
    pcts = []
    for i, b in enumerate(sel):
        band = a[b]
        t0 = time.perf_counter()
        p2, p98 = np.percentile(band, [2, 98])
        t1 = time.perf_counter()
        s = np.clip((band - p2) / (p98 - p2) * 255, 0, 255)
        if i == 0:
            low = s < 100
            s[low] = s[low] * 0.7
        out[:, :, i] = s
        t_str += time.perf_counter() - t1
        t_pct += t1 - t0
        pcts.append((p2, p98))
    t0 = time.perf_counter()
    img = out.astype(np.uint8)
    t_str += time.perf_counter() - t0
    return img, np.array(pcts), t_pct, t_str


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    fn()
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e-3 / reps


def host_timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def one(size, dtype, reps):
    name = np.dtype(dtype).name
    a = synthetic(size, dtype)
    sel = S.select_bands(6, "water")
    n, es = size * size, a.dtype.itemsize
    say(f"{name} 6 x {size} x {size} ({a.nbytes / 1e9:.2f} GB), bands {sel}:")
    # ---- host: numpy, then the upload of its uint8 image
    img_np, pct_np, t_pct, t_str = numpy_enhance(a, sel)
    t_up8 = host_timed(lambda: torch.from_numpy(img_np).to(DEV), 3)
    # ---- device
    t_up = host_timed(lambda: S.load_raster(a, DEV), 3)
    t_up3 = host_timed(lambda: S.load_raster(a[2:5], DEV), 3)
    r = S.load_raster(a, DEV)
    img_dev, nonfinite = S._enhance(r, "water")
    pct_dev, _ = S._percentiles(r, sel)
    same = bool(np.array_equal(pct_dev.cpu().numpy(), pct_np)) and bool(np.array_equal(img_dev.cpu().numpy(), img_np))
    assert same and int(nonfinite.item()) == 0, "the device result differs from numpy's: no timing of a different computation"
    (k_lo, g_lo), (k_hi, g_hi) = S.percentile_ranks(n)
    ws = torch.empty(L.lib.runet_band_percentiles_workspace(3), device=DEV, dtype=torch.uint8)
    pct = torch.empty((3, 2), device=DEV, dtype=torch.float64)
    nf = torch.empty(1, device=DEV, dtype=torch.int32)
    ms = (ctypes.c_float * 4)()
    passes = []
    for i in range(reps + 1):                            # the first call is the warm-up
        L.check(L.lib.runet_band_percentiles_timed(*r.args, *sel, 3, k_lo, g_lo, k_hi, g_hi, 0, pct.data_ptr(), nf.data_ptr(), ws.data_ptr(),
                                                   ws.numel(), ops.stream(), ms))
        if i:
            passes.append(list(ms))
    passes = np.array(passes)
    n_pass = int((passes[0] > 0).sum())
    pass_s = np.median(passes, axis=0)[:n_pass] * 1e-3
    t_sel = timed(lambda: S._percentiles(r, sel), reps)
    out = torch.empty((size, size, 3), device=DEV, dtype=torch.uint8)
    t_stretch = timed(lambda: L.check(L.lib.runet_band_stretch_u8(*r.args, *sel, pct.data_ptr(), 0, out.data_ptr(), out.stride(0), ops.stream())),
                      reps)
    pass_bytes, stretch_bytes = 3 * n * es, 3 * n * es + 3 * n
    say(f"  upload of the raw bands (pageable): 6 bands {t_up * 1e3:9.1f} ms = {a.nbytes / t_up * 1e-9:6.2f} GB/s;   the 3 selected bands "
        f"{t_up3 * 1e3:9.1f} ms")
    for p, t in enumerate(pass_s):
        say(f"  selection pass {p}: {t * 1e3:9.3f} ms  {pass_bytes / t * 1e-9:8.1f} GB/s of the {pass_bytes / 1e9:.2f} GB it reads "
            f"(min / max over {reps} calls {passes[:, p].min():.3f} / {passes[:, p].max():.3f} ms)")
    say(f"  runet_band_percentiles, whole call ({n_pass} passes, memset included): {t_sel * 1e3:9.3f} ms")
    say(f"  runet_band_stretch_u8: {t_stretch * 1e3:9.3f} ms  {stretch_bytes / t_stretch * 1e-9:8.1f} GB/s of the {stretch_bytes / 1e9:.2f} GB it moves")
    dev_total, dev_total3 = t_up + t_sel + t_stretch, t_up3 + t_sel + t_stretch
    host_total = t_pct + t_str + t_up8
    say(f"  numpy on the host: np.percentile x 3 {t_pct:7.2f} s, stretch + casts {t_str:7.2f} s, upload of the uint8 image {t_up8 * 1e3:7.1f} ms")
    say(f"  end to end to a uint8 scene on the device: host numpy + upload {host_total:7.2f} s;  upload of 6 raw bands + device "
        f"{dev_total:7.3f} s ({host_total / dev_total:5.1f} x);  upload of 3 bands + device {dev_total3:7.3f} s ({host_total / dev_total3:5.1f} x)")
    return {"dtype": name, "size": size, "equal_to_numpy": same, "upload6_ms": round(t_up * 1e3, 1), "upload3_ms": round(t_up3 * 1e3, 1),
            "pass_ms": [round(float(t) * 1e3, 3) for t in pass_s], "pass_GBps": [round(pass_bytes / float(t) * 1e-9, 1) for t in pass_s],
            "percentiles_ms": round(t_sel * 1e3, 3), "stretch_ms": round(t_stretch * 1e3, 3),
            "stretch_GBps": round(stretch_bytes / t_stretch * 1e-9, 1), "numpy_percentile_s": round(t_pct, 2), "numpy_stretch_s": round(t_str, 2),
            "upload_u8_ms": round(t_up8 * 1e3, 1), "host_total_s": round(host_total, 2), "device_total6_s": round(dev_total, 3),
            "device_total3_s": round(dev_total3, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=10980)
    ap.add_argument("--dtypes", default="uint16,float32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", help="also write the text report here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene.py needs the GPU: there is no CPU path to time")
    say(f"scene ingestion on {torch.cuda.get_device_name(0)}, host numpy {np.__version__} with {os.cpu_count()} CPUs visible; device events, "
        f"{a.reps} calls after a warm-up")
    res = [one(a.size, np.dtype(d).type, a.reps) for d in a.dtypes.split(",")]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")
    print(json.dumps({"scene_bench": res}))


if __name__ == "__main__":
    main()
