"""Connected-component labelling and the water-mask cleanup (components.py, csrc/ccl.hip) on one MI355X, beside scipy on the same machine's host.

Per size (512, 4096, 10980: a tile, a large crop, a Sentinel-2 scene) and per input (a smooth synthetic water mask, built as bench_edt.py
builds the source of its band, with specks of water on land and of land in the water; a 50 % random mask; a 59.3 % random mask, the
4-connected percolation threshold, where components are largest and most tortuous and the union chains longest):
  * runet_ccl_label_u8, runet_ccl_areas, runet_ccl_filter_u8 and runet_ccl_table (count only, and with a table of the exact capacity) with
    device events around back-to-back calls on buffers allocated before.  The labelling is given in GB/s against its floor of 1 byte read
    and 4 written per pixel;
  * label_components end to end, numpy in -> numpy out: upload of the mask, the three launches, download of the labels (host clock);
  * scipy.ndimage.label on the same mask on the host, where scipy is installed, and dense_labels of the device result compared with it for
    equality at the size that is timed;
  * CoastlineExtractor.extract_coastline_from_image, tiled, simplify_rule "exact", with and without min_water_area / min_land_area, on a
    scene painted from the blob mask.  The network is replaced by a sigmoid of the first channel, so that the figure is the extraction path
    (tiles, threshold and stitch, cleanup, band, contours, simplification, the one download, the host's unpacking) and not the model.

Not a bench line of the contract (bench.py measures the Robust U-Net training metric).
  python tools/bench_ccl.py [--sizes 512,4096,10980] [--reps 5] [--scipy-max 10980] [--scipy-max-random 4096] [--out FILE]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PKG = importlib.import_module("eusipco-2026-robust-unet_amd")
C = importlib.import_module("eusipco-2026-robust-unet_amd.components")
L = importlib.import_module("eusipco-2026-robust-unet_amd._lib")
ops = importlib.import_module("eusipco-2026-robust-unet_amd.ops")
from bench_edt import smooth_water, timed, wall  # noqa: E402  (the same mask source and timers)

DEV = torch.device("cuda:0")
LINES = []


def say(s):
    LINES.append(s)
    print(s, flush=True)


def blob_with_specks(size, seed=0):
    """the smooth water mask with one 3 x 3 speck of the other class per 64 x 64 pixels on average"""
    m = smooth_water(size, seed)
    rng = np.random.default_rng(seed + 1)
    k = max(4, size * size // 4096)
    ys, xs = rng.integers(1, size - 1, k), rng.integers(1, size - 1, k)
    flip = m[ys, xs] ^ 1
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            m[ys + dy, xs + dx] = flip
    return m


def one_input(name, mask, reps, with_scipy, row):
    h, w = mask.shape
    px = h * w
    m = torch.from_numpy(mask).to(DEV)
    out = m.clone()
    ws = C._workspace(1, h, w, DEV)
    labels = torch.empty((1, h, w), device=DEV, dtype=torch.int32)
    areas = torch.empty((1, h, w), device=DEV, dtype=torch.int32)
    frame = torch.empty((1, h, w), device=DEV, dtype=torch.uint8)
    counts = torch.empty((1, 2), device=DEV, dtype=torch.int64)
    count = torch.empty(1, device=DEV, dtype=torch.int64)

    def label():
        L.check(L.lib.runet_ccl_label_u8(m.data_ptr(), 1, h, w, w, px, 0, 8, labels.data_ptr(), ws.data_ptr(), ws.numel(), ops.stream()))

    def area():
        L.check(L.lib.runet_ccl_areas(labels.data_ptr(), 1, h, w, areas.data_ptr(), frame.data_ptr(), ops.stream()))

    def filt():
        L.check(L.lib.runet_ccl_filter_u8(labels.data_ptr(), areas.data_ptr(), frame.data_ptr(), 1, h, w, 50, 1, 0, out.data_ptr(), counts.data_ptr(),
                                          ops.stream()))

    def tab(capacity, table):
        L.check(L.lib.runet_ccl_table(labels.data_ptr(), areas.data_ptr(), frame.data_ptr(), 1, h, w, capacity, count.data_ptr(),
                                      None if table is None else table.data_ptr(), ws.data_ptr(), ws.numel(), ops.stream()))

    t_label = timed(label, reps)
    t_area = timed(area, reps)
    t_filter = timed(filt, reps)
    t_count = timed(lambda: tab(0, None), reps)
    k = int(count.item())
    table = torch.empty((1, max(k, 1), 8), device=DEV, dtype=torch.int32)
    t_table = timed(lambda: tab(k, table), reps) if k else 0.0
    t_e2e = wall(lambda: C.label_components(mask, device=DEV), max(1, reps // 2))
    r = {"label_ms": t_label, "label_gbs": 5 * px / t_label / 1e6, "areas_ms": t_area, "filter_ms": t_filter, "table_count_ms": t_count,
         "table_ms": t_table, "label_end_to_end_ms": t_e2e, "components": k, "features": int(mask.sum())}
    line = (f"  {name:14s} {k:9d} components   label {t_label:9.3f} ms ({r['label_gbs']:7.1f} GB/s of 5 B/px)   areas {t_area:8.3f} ms   "
            f"filter {t_filter:8.3f} ms   table: count {t_count:8.3f} ms, rows {t_table:8.3f} ms   numpy -> numpy {t_e2e:9.2f} ms")
    if with_scipy:
        from scipy import ndimage
        t0 = time.perf_counter()
        ref, n_ref = ndimage.label(mask, structure=np.ones((3, 3), bool))
        r["scipy_ms"] = (time.perf_counter() - t0) * 1e3
        r["equals_scipy"] = bool(n_ref == k and np.array_equal(C.dense_labels(labels[0]), ref))
        line += f"   scipy {r['scipy_ms']:10.1f} ms (x{r['scipy_ms'] / t_e2e:6.1f} of numpy -> numpy; equal: {r['equals_scipy']})"
    say(line)
    row[name] = r


def extractor_times(mask, reps, row):
    size = mask.shape[0]
    ex = PKG.CoastlineExtractor(model=PKG.RobustUNet(3, 1, 16), device=DEV, simplify_rule="exact")
    ex._prob = lambda tiles: tiles[:, 0:1].sigmoid().contiguous()
    image = np.repeat((mask * 255)[:, :, None], 3, axis=2)   # water is white: above the mean in every channel, so sigmoid > 0.5

    def run(**kw):
        return ex.extract_coastline_from_image(image, tiled=True, tile=512, halo=64, batch=8, **kw)

    t_plain = wall(run, reps)
    t_clean = wall(lambda: run(min_water_area=50, min_land_area=50), reps)
    plain, clean = run(), run(min_water_area=50, min_land_area=50)
    row["extractor"] = {"plain_ms": t_plain, "cleanup_ms": t_clean, "plain_coastlines": plain["coastline_count"],
                        "cleanup_coastlines": clean["coastline_count"], "cleanup": clean["cleanup"]}
    say(f"  extractor {size} x {size} (tiled, no network): {t_plain:9.1f} ms and {plain['coastline_count']} coastlines without cleanup, "
        f"{t_clean:9.1f} ms and {clean['coastline_count']} with min_water_area = min_land_area = 50 ({clean['cleanup']['removed_water_components']} "
        f"specks removed, {clean['cleanup']['filled_land_components']} holes filled)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,4096,10980")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scipy-max", type=int, default=10980, help="largest size at which scipy labels the blob mask beside the device")
    ap.add_argument("--scipy-max-random", type=int, default=4096, help="the same for the two random masks")
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
        blob = blob_with_specks(size)
        one_input("blob + specks", blob, a.reps, have_scipy and size <= a.scipy_max, row)
        for name, density in (("random 50 %", 0.5), ("random 59.3 %", 0.593)):
            rnd = (np.random.default_rng(1).random((size, size)) < density).astype(np.uint8)
            one_input(name, rnd, a.reps, have_scipy and size <= a.scipy_max_random, row)
            del rnd
        torch.cuda.empty_cache()
        extractor_times(blob, max(1, a.reps // 2), row)
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"lines": LINES, "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
