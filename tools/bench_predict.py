"""Prediction path (predict.py, csrc/coastline.hip) on one MI355X:

  * images/s of the reference-size path (predict_coastline.py:387-396, 595-602) on a 512 x 512 image: upload, network, arg-max, dilation
    difference, one download - without the host-side contour tracing, which is reported on its own;
  * Mpixel/s of predict_scene on a seeded 4096 x 4096 scene (tile 512, halo 64, batch 8);
  * each of the four new kernels at 512^2 and 4096^2 against the same step composed from stock torch device ops on the same data, the two
    alternated in windows of back-to-back calls timed with device events (>= 1 s per variant after a warm-up), with the bytes each kernel
    must move (from the shapes) over its time;
  * the post-processing share of one 512^2 prediction;
  * --model {unet,runet,<baseline>}: the whole-prediction lines above for that model (default unet, the reference's; every other one is a
    probability model, binarised as `prob > 0.5`), and for those the two kernels of the probability route against their torch composition:
    planar tiles against the NHWC-4 tiles + `[..., :3].permute(0, 3, 1, 2).contiguous()`, threshold_stitch against `(prob > thr)` plus the
    copies into the scene maps, with and without the soft map (figures kept in profiles/predict_models.txt);
  * contour tracing (csrc/contours.hip) against the host tracer on the same coastline band, on this box, in interleaved rounds: the band
    of the 512^2 scene above, and the bands of a seeded smooth random field at 2048^2 and 10980^2; device time by device events and by the
    wall clock including its three downloads, the workspace bytes at each size.  Where the host tracer would exceed --host-budget seconds
    it is timed on the top-left 2048^2 crop instead, and the report says so;
  * polygon simplification by the exact rule (csrc/simplify.hip) on the traced contours of those bands, interleaved the same way: the
    device kernels by events, device trace + simplify + downloads by the wall clock, the default path (trace, download, host float64
    Douglas-Peucker) by the wall clock, and the two host rules alone on the same contours (on the first contours only where all of them
    would exceed --host-budget, and the report says so); vertices in and out, the largest round count, download and workspace bytes
    (figures kept in profiles/contours_simplify.txt).

  * --what report: the kernels behind the report figures (csrc/report.hip: combined overlay, NDWI pass 1 and pass 2, RGB histogram,
    error overlays) at 512^2, 2048^2 and 10980^2: device-event time and GB/s over the bytes each must move, beside numpy on this host
    running the restatement tests/report_ref.py on the same data (results checked equal first); and the public functions end to end by
    the wall clock, upload, synchronisation and download included, against the same numpy (figures kept in profiles/report.txt).

Not a bench line of the contract (bench.py measures the Robust U-Net training metric); the figures are kept in profiles/predict_postprocess.txt.
  python tools/bench_predict.py [--what all|path|kernels|contours|simplify|report] [--model unet] [--window 0.5] [--host-budget 20] [--out FILE]
"""
import argparse
import importlib
import json
import math
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("eusipco-2026-robust-unet_amd")
P = importlib.import_module("eusipco-2026-robust-unet_amd.predict")
data = importlib.import_module("eusipco-2026-robust-unet_amd.data")
DEV = torch.device("cuda:0")
LINES = []


def say(s):
    LINES.append(s)
    print(s, flush=True)


def scene_u8(h, w, seed):
    """smooth seeded blobs (a darker region on a brighter one) so that masks look like coastlines, not like noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w].astype(np.float32)
    f = np.zeros((h, w), np.float32)
    for _ in range(6):
        cy, cx, s = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0.08, 0.25) * min(h, w)
        f += np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    water = f > np.median(f)
    img = np.where(water[..., None], 60, 150) + rng.integers(-20, 21, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8), water.astype(np.uint8)


def windows(fns, window_s):
    """fns: the variants to alternate.  -> seconds per call of each (two windows per variant, each about window_s of back-to-back calls)."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    reps = []
    for f in fns:
        f(); f()
        ev[0].record(); f(); ev[1].record(); ev[1].synchronize()
        reps.append(max(3, math.ceil(window_s / max(ev[0].elapsed_time(ev[1]) * 1e-3, 1e-6))))
    tot = [0.0] * len(fns)
    for _ in range(2):
        for j, f in enumerate(fns):
            ev[0].record()
            for _ in range(reps[j]):
                f()
            ev[1].record()
            ev[1].synchronize()
            tot[j] += ev[0].elapsed_time(ev[1]) * 1e-3
    return [t / (2 * r) for t, r in zip(tot, reps)], [2 * r for r in reps]


MODELS = {"unet": "UNet", "runet": "RobustUNet", **{k.lower(): k for k in P.PROB_MODELS if k != "RobustUNet"}}


def timed_cases(size, cases, window_s):
    rows = []
    for name, hip, stock, nbytes in cases:
        (t_hip, t_stock), (r_hip, r_stock) = windows((hip, stock), window_s)
        rows.append({"size": size, "kernel": name, "hip_us": round(t_hip * 1e6, 2), "torch_us": round(t_stock * 1e6, 2),
                     "torch_over_hip": round(t_stock / t_hip, 2), "bytes_min": nbytes, "hip_GBps": round(nbytes / t_hip * 1e-9, 1),
                     "calls": [r_hip, r_stock]})
        say(f"  {size:5d}^2  {name:34s} HIP {t_hip * 1e6:9.2f} us  {nbytes / t_hip * 1e-9:8.1f} GB/s   torch ops {t_stock * 1e6:9.2f} us"
            f"   torch / HIP = {t_stock / t_hip:6.2f}   ({r_hip} / {r_stock} calls)")
    return rows


def prob_kernel_rows(size, window_s):
    """the two kernels of the probability route on one size x size tile (halo 0), as kernel_rows does for the other four"""
    h = w = size
    scene, _ = scene_u8(h, w, size)
    sd = torch.from_numpy(scene).to(DEV)
    origin = torch.zeros((1, 2), device=DEV, dtype=torch.int32)
    thr = 0.5
    prob = torch.rand((1, 1, h, w), device=DEV)
    prob[0, 0, ::7, ::5] = float("nan")
    prob[0, 0, 1::7, ::5] = thr
    mask, soft = torch.empty((h, w), device=DEV, dtype=torch.uint8), torch.empty((h, w), device=DEV)
    t_mask, t_soft = torch.empty_like(mask), torch.empty_like(soft)

    def t_planar():
        return P.scene_to_tiles(sd, origin, size)[..., :3].permute(0, 3, 1, 2).contiguous()

    def t_threshold():
        return t_mask.copy_(prob[0, 0] > thr)

    def t_threshold_soft():
        t_soft.copy_(prob[0, 0])
        return t_mask.copy_(prob[0, 0] > thr)

    assert torch.equal(P.scene_to_tiles(sd, origin, size, "nchw").view(torch.int32), t_planar().view(torch.int32))
    assert torch.equal(P.threshold_stitch(prob, origin, 0, mask, thr, soft=soft), t_threshold_soft())
    assert torch.equal(soft.view(torch.int32), t_soft.view(torch.int32))
    return timed_cases(size, [
        ("scene_to_tiles nchw", lambda: P.scene_to_tiles(sd, origin, size, "nchw"), t_planar, 3 * h * w + 12 * h * w),
        ("threshold_stitch", lambda: P.threshold_stitch(prob, origin, 0, mask, thr), t_threshold, 4 * h * w + h * w),
        ("threshold_stitch + soft map", lambda: P.threshold_stitch(prob, origin, 0, mask, thr, soft=soft), t_threshold_soft,
         4 * h * w + h * w + 4 * h * w),
    ], window_s)


def kernel_rows(size, window_s):
    h = w = size
    scene, water = scene_u8(h, w, size)
    sd, wd = torch.from_numpy(scene).to(DEV), torch.from_numpy(water).to(DEV)
    origin = torch.zeros((1, 2), device=DEV, dtype=torch.int32)
    mean = torch.tensor(data.IMAGENET_MEAN, device=DEV)
    std = torch.tensor(data.IMAGENET_STD, device=DEV)
    z4 = torch.randn((1, h, w, 4), device=DEV)
    mask = torch.empty((h, w), device=DEV, dtype=torch.uint8)
    small = wd[::max(1, h // 512), ::max(1, w // 512)].contiguous() if size > 512 else wd
    dh, dw = (h, w) if size > 512 else (1000, 1531)
    out = torch.empty((dh, dw), device=DEV, dtype=torch.uint8)
    inv_x, inv_y = 1.0 / (dw / small.shape[1]), 1.0 / (dh / small.shape[0])
    ix = torch.clamp(torch.floor(torch.arange(dw, dtype=torch.float64) * inv_x).long(), max=small.shape[1] - 1).to(DEV)
    iy = torch.clamp(torch.floor(torch.arange(dh, dtype=torch.float64) * inv_y).long(), max=small.shape[0] - 1).to(DEV)
    k = 5
    se = torch.from_numpy(P.ellipse_element(k).astype(np.float32)).to(DEV)[None, None]
    coast, counts = torch.empty_like(wd), torch.empty(2, device=DEV, dtype=torch.int32)

    def t_norm():
        return F.pad((sd.float().div(255.0) - mean) / std, (0, 1))

    def t_argmax():
        return z4[0, :, :, :2].argmax(-1).to(torch.uint8)

    def t_resize():
        return small[iy[:, None], ix[None, :]]

    def t_dilate():
        d = (F.conv2d(wd[None, None].float(), se, padding=k // 2) > 0).to(torch.uint8)[0, 0]
        c = d - wd
        return c, torch.stack([wd.sum(), c.sum()])

    cases = [
        ("scene_to_tiles", lambda: P.scene_to_tiles(sd, origin, size), t_norm, 3 * h * w + 16 * h * w),
        ("argmax_stitch", lambda: P.argmax_stitch(z4, origin, 0, mask, 2), t_argmax, 16 * h * w + h * w),
        (f"resize_nearest {small.shape[0]}^2->{dh}x{dw}", lambda: P.resize_nearest(small, (dh, dw), out=out), t_resize,
         small.numel() + dh * dw),
        ("dilate_diff k=5", lambda: P.dilate_diff(wd, k, coast=coast, counts=counts), t_dilate, 2 * h * w),
    ]
    # same results first: a faster kernel that computes something else is not faster
    # (stock device division by a scalar may multiply by the reciprocal: last-bit differences allowed for this one only)
    assert torch.allclose(P.scene_to_tiles(sd, origin, size)[0], t_norm(), rtol=0, atol=2e-6)
    assert torch.equal(P.argmax_stitch(z4, origin, 0, mask, 2), t_argmax())
    assert torch.equal(P.resize_nearest(small, (dh, dw), out=out), t_resize())
    c_ref, n_ref = t_dilate()
    c_got, n_got, _ = P.dilate_diff(wd, k, coast=coast, counts=counts)
    assert torch.equal(c_got, c_ref) and n_got.tolist() == n_ref.tolist()
    return timed_cases(size, cases, window_s)


def path_rows(window_s, model="unet"):
    torch.manual_seed(0)
    ex = pkg.CoastlineExtractor(model=pkg.UNet(3, 2) if model == "unet" else getattr(pkg, MODELS[model])(), device="cuda:0", input_size=512)
    scene, _ = scene_u8(512, 512, 1)
    from PIL import Image
    pil = Image.fromarray(scene)
    out = {}

    def device_path():
        buf = torch.empty(2 * 512 * 512 + 16, device=DEV, dtype=torch.uint8)
        water, coast = buf[:512 * 512].view(512, 512), buf[512 * 512:2 * 512 * 512].view(512, 512)
        ex._predict_resized(pil, out=water)
        P.dilate_diff(water, 5, coast=coast, counts=buf[2 * 512 * 512:2 * 512 * 512 + 8].view(torch.int32))
        return buf.cpu()

    for _ in range(3):
        device_path()
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < max(1.0, 2 * window_s):
        device_path()
        n += 1
    dt = (time.perf_counter() - t0) / n
    out["reference_size_512"] = {"images_per_s": round(1 / dt, 1), "ms_per_image": round(dt * 1e3, 3), "images": n}
    say(f"  reference-size path, 512 x 512 image, upload -> masks + counts on the host: {1 / dt:7.1f} images/s ({dt * 1e3:.3f} ms, {n} images)")
    # the four post-processing kernels of that prediction, back to back on the device
    sd = torch.from_numpy(scene).to(DEV)
    origin = torch.zeros((1, 2), device=DEV, dtype=torch.int32)
    tiles = P.scene_to_tiles(sd, origin, 512, "nchw" if ex.prob else "nhwc4")
    net = ex._prob if ex.prob else ex._z4
    z4 = net(tiles)
    water, coast = torch.empty((512, 512), device=DEV, dtype=torch.uint8), torch.empty((512, 512), device=DEV, dtype=torch.uint8)
    counts = torch.empty(2, device=DEV, dtype=torch.int32)

    def post():
        if ex.prob:
            P.scene_to_tiles(sd, origin, 512, "nchw")
            P.threshold_stitch(z4, origin, 0, water, ex.threshold)
        else:
            P.scene_to_tiles(sd, origin, 512)
            P.argmax_stitch(z4, origin, 0, water, 2)
        P.dilate_diff(water, 5, coast=coast, counts=counts)

    (t_post, t_net), _ = windows((post, lambda: net(tiles)), window_s)
    out["post_us_512"], out["network_us_512"] = round(t_post * 1e6, 2), round(t_net * 1e6, 2)
    out["post_share_of_prediction"] = round(t_post / dt, 5)
    say(f"  of which on the device: network {t_net * 1e3:.3f} ms, normalise + {'threshold' if ex.prob else 'arg-max'} + dilation difference {t_post * 1e6:.1f} us "
        f"= {100 * t_post / dt:.2f} % of the prediction")
    res = ex.extract_coastline_from_image(scene)
    t0 = time.perf_counter()
    lines = P.coastlines_from_mask(res["coastline_mask"])
    out["contours_host_ms_512"] = round((time.perf_counter() - t0) * 1e3, 2)
    say(f"  host contour tracing + polygon simplification of that coastline mask: {out['contours_host_ms_512']} ms ({len(lines)} coastlines; "
        f"untrained weights, so the mask is whatever the random network draws)")
    big, _ = scene_u8(4096, 4096, 2)
    ex.predict_scene(big[:1024, :1024], as_tensor=True)
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < max(1.0, 2 * window_s):
        ex.predict_scene(big, tile=512, halo=64, batch=8, as_tensor=True)
        torch.cuda.synchronize()
        n += 1
    dt = (time.perf_counter() - t0) / n
    out["predict_scene_4096"] = {"mpixel_per_s": round(4096 * 4096 / dt * 1e-6, 2), "s_per_scene": round(dt, 3), "tiles": len(P.tile_plan(4096, 4096)),
                                 "scenes": n}
    say(f"  predict_scene, 4096 x 4096, tile 512 / halo 64 / batch 8 ({out['predict_scene_4096']['tiles']} tiles): "
        f"{out['predict_scene_4096']['mpixel_per_s']} Mpixel/s ({dt:.3f} s per scene incl. upload, {n} scenes)")
    return out


def field_water(size, seed, cell=48):
    """a seeded smooth random field (bicubic interpolation of a coarse normal grid, one cell = `cell` pixels) thresholded at 0: winding
    shores at every size, built on the device"""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randn((1, 1, size // cell + 3, size // cell + 3), generator=g).to(DEV)
    return (F.interpolate(coarse, size=(size, size), mode="bicubic", align_corners=True)[0, 0] > 0).to(torch.uint8)


def contour_rows(sizes, host_budget):
    lib = importlib.import_module("eusipco-2026-robust-unet_amd._lib").lib
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    rows = []
    host_px_per_s = None
    for size in sizes:
        water = torch.from_numpy(scene_u8(512, 512, 1)[1]).to(DEV) if size == 512 else field_water(size, size)
        band = P.dilate_diff(water, 5)[0]
        del water
        h, w = band.shape
        n_set = int(band.sum(dtype=torch.int64))
        # the host side of the comparison: the whole band, or a crop when the whole band would not fit the budget
        crop = size
        if host_px_per_s is not None and n_set / host_px_per_s > host_budget:
            crop = 2048
        band_np = band[:crop, :crop].cpu().numpy()
        rounds = 5 if size <= 512 else 3
        t_dev, t_wall, t_host = [], [], []
        got = P.trace_external_contours_device(band)     # warm-up: code objects, allocator
        for _ in range(rounds):                          # interleaved: device, host, device, host, ...
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev[0].record()
            got = P.trace_external_contours_device(band)
            ev[1].record()
            ev[1].synchronize()
            t_wall.append(time.perf_counter() - t0)
            t_dev.append(ev[0].elapsed_time(ev[1]) * 1e-3)
            t0 = time.perf_counter()
            want = P.trace_external_contours(band_np)
            t_host.append(time.perf_counter() - t0)
        check = got if crop == size else P.trace_external_contours_device(band[:crop, :crop].contiguous())
        assert len(check) == len(want) and all(np.array_equal(a, b) for a, b in zip(check, want)), "device and host contours differ"
        host_px_per_s = int(np.count_nonzero(band_np)) / float(np.median(t_host))
        # workspace bytes: the pixel stage from the shape, the state stage from the state count
        ws_bytes = lib.runet_contours_workspace_bytes(h, w)
        ws = torch.empty(ws_bytes, device=DEV, dtype=torch.uint8)
        cnt = torch.empty(1, device=DEV, dtype=torch.int64)
        assert lib.runet_contours_count(band.data_ptr(), h, w, ws.data_ptr(), ws_bytes, cnt.data_ptr(), None) == 0
        torch.cuda.synchronize()
        n_states = int(cnt.cpu()[0])
        sws_bytes = lib.runet_contours_state_workspace_bytes(n_states)
        del ws
        row = {"size": size, "set_pixels": n_set, "states": n_states, "contours": len(got), "vertices": int(sum(len(c) for c in got)),
               "device_ms_events": round(float(np.median(t_dev)) * 1e3, 3), "device_ms_wall_with_downloads": round(float(np.median(t_wall)) * 1e3, 3),
               "host_ms": round(float(np.median(t_host)) * 1e3, 1), "host_on": f"{crop}^2" + ("" if crop == size else " crop"),
               "host_set_pixels": int(np.count_nonzero(band_np)), "rounds": rounds, "workspace_bytes": ws_bytes,
               "state_workspace_bytes": sws_bytes, "device_ms_all": [round(t * 1e3, 3) for t in t_wall],
               "host_ms_all": [round(t * 1e3, 1) for t in t_host]}
        rows.append(row)
        say(f"  {size:5d}^2 band: {n_set} set pixels, {n_states} states, {row['contours']} contours, {row['vertices']} vertices | device "
            f"{row['device_ms_events']:.3f} ms (events) {row['device_ms_wall_with_downloads']:.3f} ms (wall, 3 downloads) | host tracer on "
            f"{row['host_on']} ({row['host_set_pixels']} set pixels) {row['host_ms']:.1f} ms | medians of {rounds} interleaved rounds | "
            f"workspace {ws_bytes / 2**20:.1f} MiB + states {sws_bytes / 2**20:.1f} MiB")
        del band
    return rows


def simplify_rows(sizes, host_budget):
    """polygon simplification by the exact rule on the device (csrc/simplify.hip) against the host: the float64 rule (predict._simplify,
    what the default path runs after the trace) and the exact rule's host restatement, on the traced contours of the bands of
    contour_rows; the host side on the first contours only where all of them would exceed the budget"""
    lib = importlib.import_module("eusipco-2026-robust-unet_amd._lib").lib
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    rows = []
    host_v_per_s = {}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    for size in sizes:
        water = torch.from_numpy(scene_u8(512, 512, 1)[1]).to(DEV) if size == 512 else field_water(size, size)
        band = P.dilate_diff(water, 5)[0]
        del water
        packed, (n, total) = P._trace_packed(band, 10, with_sizes=True)
        contours = P._unpack_contours(packed.cpu().numpy())
        # the host side: all contours, or the first ones whose vertices fit the budget at the speed measured on the size before
        n_host = n
        slowest = min(host_v_per_s.values()) if host_v_per_s else None
        if slowest is not None and total / slowest > host_budget:
            lens = np.cumsum([len(c) for c in contours])
            n_host = max(1, int(np.searchsorted(lens, slowest * host_budget)))
        host_contours = contours[:n_host]
        host_vertices = int(sum(len(c) for c in host_contours))
        ws_bytes = lib.runet_contours_simplify_workspace_bytes(n, total)
        ws = torch.empty(ws_bytes, device=DEV, dtype=torch.uint8)

        def kernels():
            assert lib.runet_contours_simplify(packed.data_ptr(), n, total, 0.002, -1, ws.data_ptr(), ws_bytes, None) == 0

        rounds = 5 if size <= 512 else 3
        t_dev, t_wall_exact, t_wall_default, t_f64, t_exact = [], [], [], [], []
        kernels()
        got = P.coastlines_from_mask(band, rule="exact")     # warm-up: code objects, allocator
        for _ in range(rounds):                              # interleaved: device, host, device, host, ...
            torch.cuda.synchronize()
            ev[0].record()
            kernels()
            ev[1].record()
            ev[1].synchronize()
            t_dev.append(ev[0].elapsed_time(ev[1]) * 1e-3)
            t, got = wall(lambda: P.coastlines_from_mask(band, rule="exact"))
            t_wall_exact.append(t)
            t, lines_f64 = wall(lambda: P._simplify(host_contours, 10, 0.002))
            t_f64.append(t)
            t, lines_exact = wall(lambda: P._simplify_exact(host_contours, 10, 0.002))
            t_exact.append(t)
            if n_host == n:
                t, default = wall(lambda: P.coastlines_from_mask(band))
                t_wall_default.append(t)
        assert got[:n_host] == lines_exact, "device and host lists of the exact rule differ"
        head = ws[:16].view(torch.int32).cpu().tolist()
        assert head[0] == n and head[2] == 0 and head[1] == sum(len(c) for c in got)
        host_v_per_s = {"f64": host_vertices / float(np.median(t_f64)), "exact": host_vertices / float(np.median(t_exact))}
        differ = sum(a != b for a, b in zip(lines_f64, lines_exact))
        med = lambda v: round(float(np.median(v)) * 1e3, 3) if v else None
        row = {"size": size, "contours": n, "vertices_in": total, "vertices_out": head[1], "largest_round_count": head[3],
               "device_simplify_ms_events": med(t_dev), "device_trace_simplify_downloads_ms_wall": med(t_wall_exact),
               "default_trace_download_host_float64_ms_wall": med(t_wall_default), "host_float64_ms": med(t_f64), "host_exact_ms": med(t_exact),
               "host_on_contours": n_host, "host_on_vertices": host_vertices, "float64_and_exact_lists_differ_on": differ,
               "download_bytes_before": 4 * (3 + n + 2 * total), "download_bytes_after": 4 * (3 + n + 2 * head[1]), "workspace_bytes": ws_bytes,
               "rounds": rounds}
        rows.append(row)
        scale = total / max(1, host_vertices)
        say(f"  {size:5d}^2 band: {n} contours, {total} -> {head[1]} vertices, largest round count {head[3]} | device simplify "
            f"{row['device_simplify_ms_events']:.3f} ms (events) | device trace + simplify + downloads {row['device_trace_simplify_downloads_ms_wall']:.3f} ms (wall)"
            + (f" | default path (trace, download, host float64) {row['default_trace_download_host_float64_ms_wall']:.3f} ms (wall)" if t_wall_default else "")
            + f" | host float64 _simplify {row['host_float64_ms']:.1f} ms, host exact rule {row['host_exact_ms']:.1f} ms on "
            + (f"all contours" if n_host == n else f"the first {n_host} contours ({host_vertices} vertices, x {scale:.1f} for all)")
            + f"; the two rules differ on {differ} of them | download {row['download_bytes_before']} -> {row['download_bytes_after']} bytes | "
            f"workspace {ws_bytes / 2**20:.1f} MiB | medians of {rounds} interleaved rounds")
        del band, ws, packed
    return rows


def report_rows(sizes, window_s, end_to_end_sizes=(128, 256, 512, 2048, 10980)):
    """the report kernels against numpy running tests/report_ref.py on this host"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import report_ref as R
    M = importlib.import_module("eusipco-2026-robust-unet_amd.report")
    S = importlib.import_module("eusipco-2026-robust-unet_amd.scene")
    lib = importlib.import_module("eusipco-2026-robust-unet_amd._lib").lib

    def host(fn):
        t0 = time.perf_counter()
        r = fn()
        return time.perf_counter() - t0, r

    def wall(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts))

    def inputs(size):
        rng = np.random.default_rng(size)
        img, water = scene_u8(size, size, size)
        coast = P.dilate_diff(torch.from_numpy(water).to(DEV), 5)[0].cpu().numpy()
        bands = rng.integers(1, 4096, (4, size, size)).astype(np.uint16)
        bands[3][water == 1] //= 4                       # water is dark in the near infrared: two separated NDWI populations
        x = (rng.standard_normal((1, 3, size, size)) * 1.5).astype(np.float32)
        prob = rng.random((1, 1, size, size)).astype(np.float32)
        gt = water.astype(np.float32)[None, None]
        return img, water, coast, bands, x, prob, gt

    rows, e2e = [], []
    for size in sorted(set(sizes) | set(end_to_end_sizes)):
        n = size * size
        img, water, coast, bands, x, prob, gt = inputs(size)
        t_np = {}
        t_np["combined_overlay"], want_overlay = host(lambda: R.combined_overlay(img, water, coast))
        t_np["ndwi pass 1 (index, min, max)"], sel = host(lambda: [(v, v.min(), v.max()) for x_ in (R.ndwi(bands),) for v in (x_[water == 1], x_[water == 0])])
        t_np["ndwi pass 2 (binning)"], want_hist = host(lambda: [np.histogram(v[0], bins=50) for v in sel])
        t_np["rgb histogram"], want_rgb = host(lambda: [np.histogram(img[:, :, c].flatten(), bins=50, density=True) for c in range(3)])   # :828, once per channel
        t_np["error_overlays"], want_err = host(lambda: R.error_overlays(x, prob, gt))
        del sel
        # end to end: numpy in, numpy out, by the wall clock
        t_dev = {"combined_overlay": wall(lambda: M.combined_overlay(img, water, coast)),
                 "ndwi_histograms": wall(lambda: M.ndwi_histograms(bands, water)),
                 "rgb_histograms": wall(lambda: M.rgb_histograms(img)),
                 "error_overlays": wall(lambda: M.error_overlays(x, prob, gt))}
        t_host = {"combined_overlay": t_np["combined_overlay"], "ndwi_histograms": t_np["ndwi pass 1 (index, min, max)"] + t_np["ndwi pass 2 (binning)"],
                  "rgb_histograms": t_np["rgb histogram"], "error_overlays": t_np["error_overlays"]}
        e2e.append({"size": size, **{k: {"device_ms_wall": round(t_dev[k] * 1e3, 3), "numpy_ms": round(t_host[k] * 1e3, 3)} for k in t_dev}})
        say(f"  {size:5d}^2  end to end (upload, kernels, syncs, download | numpy): " + "; ".join(
            f"{k} {t_dev[k] * 1e3:.2f} | {t_host[k] * 1e3:.2f} ms" for k in t_dev))
        if size not in sizes:
            continue
        # the kernels alone, inputs and outputs on the device
        d_img, d_water, d_coast = (torch.from_numpy(a).to(DEV) for a in (img, water, coast))
        r = S.load_raster(bands, DEV)
        got = M.ndwi_histograms(r, d_water)
        assert np.array_equal(M.combined_overlay(d_img, d_water, d_coast), want_overlay)
        assert all(np.array_equal(got[k]["counts"], w[0]) and np.array_equal(got[k]["edges"], w[1]) for k, w in zip(("water", "other"), want_hist))
        got = M.rgb_histograms(d_img)
        assert all(np.array_equal(got[k]["density"], w[0]) and np.array_equal(got[k]["edges"], w[1]) for k, w in zip(("red", "green", "blue"), want_rgb))
        got = M.error_overlays(x, prob, gt)
        assert all(np.array_equal(got[k], want_err[k], equal_nan=True) for k in want_err)
        del got, want_err, want_overlay
        table = torch.from_numpy(M.overlay_table()).to(DEV)
        out = torch.empty_like(d_img)
        stats = torch.empty(8, device=DEV, dtype=torch.int64)
        edges = torch.from_numpy(np.stack([w[1] for w in want_hist])).to(DEV)
        counts = torch.empty((2, 50), device=DEV, dtype=torch.int64)
        hist = torch.empty((3, 256), device=DEV, dtype=torch.int64)
        d_x, d_prob, d_gt = (torch.from_numpy(a).to(DEV) for a in (x, prob, gt))
        colours = torch.from_numpy(M.class_colour_terms()).to(DEV)
        vis, ov = torch.empty((1, size, size, 3), device=DEV), torch.empty((1, size, size, 3), device=DEV, dtype=torch.float64)
        err, cls, sums = torch.empty((1, size, size), device=DEV), torch.empty((1, 5), device=DEV, dtype=torch.int64), torch.empty(1, device=DEV, dtype=torch.float64)
        nws = lib.runet_error_overlays_workspace_bytes(1, size, size)
        ws = torch.empty(nws // 8, device=DEV, dtype=torch.float64)
        m, sd = data.IMAGENET_MEAN, data.IMAGENET_STD
        st = None
        kernels = [
            ("combined_overlay", "combined_overlay", 8 * n,
             lambda: lib.runet_report_overlay_u8(d_img.data_ptr(), d_water.data_ptr(), d_coast.data_ptr(), size, size, table.data_ptr(), out.data_ptr(), st)),
            ("ndwi pass 1 (index, min, max)", "ndwi pass 1 (index, min, max)", 5 * n,
             lambda: lib.runet_ndwi_stats(*r.args, d_water.data_ptr(), stats.data_ptr(), st)),
            ("ndwi pass 2 (binning)", "ndwi pass 2 (binning)", 5 * n,
             lambda: lib.runet_ndwi_hist(*r.args, d_water.data_ptr(), edges.data_ptr(), 50, counts.data_ptr(), st)),
            ("rgb histogram", "rgb histogram", 3 * n, lambda: lib.runet_rgb_hist_u8(d_img.data_ptr(), size, size, hist.data_ptr(), st)),
            ("error_overlays", "error_overlays", 60 * n,
             lambda: lib.runet_error_overlays(d_x.data_ptr(), d_prob.data_ptr(), d_gt.data_ptr(), 1, size, size, 0.5, m[0], m[1], m[2], sd[0], sd[1], sd[2],
                                              colours.data_ptr(), vis.data_ptr(), ov.data_ptr(), err.data_ptr(), cls.data_ptr(), sums.data_ptr(),
                                              ws.data_ptr(), nws, st)),
        ]
        for name, key, nbytes, fn in kernels:
            (t,), (calls,) = windows((fn,), window_s)
            rows.append({"size": size, "kernel": name, "hip_us": round(t * 1e6, 2), "bytes_min": nbytes, "hip_GBps": round(nbytes / t * 1e-9, 1),
                         "numpy_ms": round(t_np[key] * 1e3, 3), "numpy_over_hip": round(t_np[key] / t, 1), "calls": calls})
            say(f"  {size:5d}^2  {name:32s} HIP {t * 1e6:10.2f} us  {nbytes / t * 1e-9:8.1f} GB/s ({nbytes / n} B/pixel)   numpy {t_np[key] * 1e3:10.2f} ms"
                f"   numpy / HIP = {t_np[key] / t:8.1f}   ({calls} calls)")
        del d_x, d_prob, d_gt, vis, ov, err, ws
    return {"kernels": rows, "end_to_end": e2e}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="all", choices=("all", "path", "kernels", "contours", "simplify", "report"),
                    help="report is not part of all: its numpy side takes minutes at 10980^2")
    ap.add_argument("--model", default="unet", choices=sorted(MODELS), help="the model of the whole-prediction lines; any but unet also "
                    "times the two kernels of the probability route")
    ap.add_argument("--host-budget", type=float, default=20.0, help="seconds one host tracing run may take before it moves to a 2048^2 crop")
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window (two windows per variant)")
    ap.add_argument("--out", help="also write the text report here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_predict.py needs the GPU: there is no CPU path to time")
    res = {}
    say(f"prediction path on {torch.cuda.get_device_name(0)}; device-event windows of >= {2 * a.window:.1f} s per variant, alternated")
    if a.what in ("all", "kernels"):
        say("kernels (HIP = csrc/coastline.hip; torch ops = the same step composed from stock device ops, results checked equal first):")
        res["kernels"] = (kernel_rows(512, a.window) + kernel_rows(4096, a.window) if a.model == "unet" else
                          prob_kernel_rows(512, a.window) + prob_kernel_rows(4096, a.window))
    if a.what in ("all", "path"):
        say(f"prediction (fp32, seeded untrained {MODELS[a.model]}):")
        res["path"] = path_rows(a.window, a.model)
    if a.what in ("all", "contours"):
        say("contour tracing (csrc/contours.hip against predict.trace_external_contours on the same band, results checked equal):")
        res["contours"] = contour_rows((512, 2048, 10980), a.host_budget)
    if a.what in ("all", "simplify"):
        say("polygon simplification (csrc/simplify.hip, the exact rule, against the host float64 rule and the exact rule's host restatement on "
            "the same traced contours; eps factor 0.002, contours of more than 10 vertices; device and host lists of the exact rule checked equal):")
        res["simplify"] = simplify_rows((512, 2048, 10980), a.host_budget)
    if a.what == "report":
        say("report arrays (HIP = csrc/report.hip, device events; numpy = the operations of tests/report_ref.py on this host, np.histogram once per selection or channel, one run; results checked equal first):")
        res["report"] = report_rows((512, 2048, 10980), a.window)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")
    print(json.dumps({"predict_bench": res}))


if __name__ == "__main__":
    main()
