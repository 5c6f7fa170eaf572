"""Prediction: the reference's `CoastlineExtractor` (predict_coastline.py:336-652) on the gfx950 kernels, for the plain 2-class U-Net it was
written for and for every 1-channel probability model of the project (RobustUNet, DeepLabV3Plus and the ten baselines).

Reference pipeline, one image at a time (line numbers of predict_coastline.py):
  1. :358-363, :387  PIL bilinear Resize((512, 512)) -> ToTensor -> Normalize(ImageNet)      host resize, then runet_scene_to_tiles
  2. :390-392        UNet(3, 2).eval(), argmax(logits, dim=1)                                 unet_forward(nhwc=True), runet_argmax_stitch
  3. :395-396        cv2.resize(pred, (W, H), INTER_NEAREST)                                  runet_resize_nearest_u8
  4. :595-602        MORPH_ELLIPSE k x k, cv2.dilate, dilated - mask                          runet_dilate_diff_u8 (+ the two pixel counts)
  5. :605-616        cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE), > 10 points,       runet_contours_count / runet_contours_trace (device
                     approxPolyDP(0.002 * arcLength)                                          masks; host: trace_external_contours), host approx_poly_dp
                                                                                              (rule "float64") or runet_contours_simplify (rule "exact")
  6. :404-413, :620-652  result dict, two PNG masks (* 255), <base>_coastlines.json           save_extraction_result

A probability model (PROB_MODELS) differs in steps 1-2 only, the two kernels on either side of the network: its tiles are planar NCHW
(runet_scene_to_tiles_nchw, the input its forward takes) and its mask is the reference's `pred > threshold`, threshold 0.5 (Main_Final.py:521,
comne.py:622, Extended_Baseline_Comparison.py:758, :920), taken by runet_threshold_stitch; NaN is land.  The same launch can fill a soft
water map (predict_scene(return_prob=True)).  Which sizes a model takes is asked of the model (`_check_input`), not tabulated here.

Between the upload of the uint8 image and the single download of (water mask, coastline mask, counts, packed contours) nothing returns to
the host but the two size words the contour tracing needs to allocate (its state count, then its contour and vertex counts) and, under
simplify_rule="exact", the simplifier's head (its kept-vertex count).
`predict_scene` is the addition for scenes larger than one network input: the scene is cut into overlapping tiles at its own resolution and
every output pixel is taken from exactly one tile's core (tile_plan), so there is no blending and the result is bit-deterministic.

OpenCV is not a dependency.  Steps 3-5 restate OpenCV's rules (index rule, ellipse spans, Suzuki-Abe border following); vertex-for-vertex
equality of the contours with cv2 is not claimed.  The analysis report (:659-846) is report.py: its arrays come from the device, matplotlib
only draws them (`report=True` below).  The GUI and the CLI are out of scope.

Multi-band rasters (load_tif_image, :425-581) come in through scene.py: `extract_coastline_from_image` and `predict_scene` take the raw
bands - a [B, H, W] array or device tensor with B <= 6, a .npy path, or anything through `bands=` (a .tif path there is read with GDAL where
it is installed; as `image` a .tif path stays what it was, an RGB file for PIL) - and run the reference's band selection, 2-98 % stretch
and darkening on the device (runet_band_percentiles, runet_band_stretch_u8).  On the tiled path the enhanced scene never leaves the device:
one upload (the raw bands), one download (the results).  On the resized path it is downloaded once, because the reference resizes the
ENHANCED image with PIL's bilinear filter (:467, :387) and that order is kept.  GDAL itself is not a dependency.
"""
from __future__ import annotations

import ctypes
import json
import os
from datetime import datetime

import numpy as np
import torch
from PIL import Image

from . import data, ops, scene as _scene
from ._lib import check, lib

MAX_DILATION = 31
# RUNET_NO_DEVICE_CONTOURS=1: masks that live on the device are downloaded and traced by the host loop (trace_external_contours) as before.
# Consulted at every call; the results are identical either way.
DEVICE_CONTOURS = os.environ.get("RUNET_NO_DEVICE_CONTOURS", "0") != "1"
# RUNET_NO_DEVICE_SIMPLIFY=1: under rule "exact" the device-traced contours are downloaded whole and simplified by the host restatement
# (approx_poly_dp_exact) instead of runet_contours_simplify.  Consulted at every call; the lists are identical either way.
DEVICE_SIMPLIFY = os.environ.get("RUNET_NO_DEVICE_SIMPLIFY", "0") != "1"
SIMPLIFY_RULES = ("float64", "exact")
EXACT_COORD_MAX = 46340                                  # rule "exact": 2 * 46340^2 < 2^32, so every distance numerator stays below 2^64
_SQRT2 = float.fromhex("0x1.6a09e667f3bcdp+0")


# ------------------------------------------------------------------------------------------------ host-side plans
def ellipse_spans(k):
    """-> (j1, j2): row i of cv2.getStructuringElement(MORPH_ELLIPSE, (k, k)) is set on columns [j1[i], j2[i])."""
    k = int(k)
    if k < 1 or k > MAX_DILATION or k % 2 == 0:
        raise ValueError(f"dilation size must be odd and in 1..{MAX_DILATION} (got {k})")
    j1, j2 = (ctypes.c_int * k)(), (ctypes.c_int * k)()
    check(lib.runet_ellipse_spans(k, j1, j2))
    return np.array(j1, dtype=np.int64), np.array(j2, dtype=np.int64)


def ellipse_element(k):
    j1, j2 = ellipse_spans(k)
    cols = np.arange(k)[None, :]
    return ((cols >= j1[:, None]) & (cols < j2[:, None])).astype(np.uint8)


def tile_plan(h, w, tile=512, halo=64, multiple=16):
    """-> int32 [n, 2] tile origins (y0, x0).  Cores of side tile - 2 * halo partition the scene from (0, 0): tile t owns the pixels
    [y0 + halo, y0 + tile - halo) x [x0 + halo, x0 + tile - halo) clipped to the scene and reads halo pixels of context around them, so
    origins start at -halo and the last row / column of tiles may overhang.  multiple: what the tile must be a multiple of (16: the U-Nets;
    the extractor has asked its model by then and passes 1)."""
    if tile <= 0 or tile % multiple:
        raise ValueError(f"tile must be a positive multiple of {multiple}" + (" (four 2x2 poolings)" if multiple == 16 else ""))
    if halo < 0 or 2 * halo >= tile:
        raise ValueError("2 * halo must be smaller than the tile")
    if h <= 0 or w <= 0:
        raise ValueError("empty scene")
    core = tile - 2 * halo
    ys = np.arange(0, h, core, dtype=np.int32) - halo
    xs = np.arange(0, w, core, dtype=np.int32) - halo
    return np.stack(np.meshgrid(ys, xs, indexing="ij"), axis=-1).reshape(-1, 2).astype(np.int32)


# ------------------------------------------------------------------------------------------------ device steps
def _dev_u8(a, device):
    if isinstance(a, torch.Tensor):
        if a.dtype != torch.uint8:
            raise ValueError("expected a uint8 tensor")
        return a.to(device).contiguous()
    a = np.ascontiguousarray(a)
    if a.dtype != np.uint8:
        raise ValueError("expected a uint8 array")
    return torch.from_numpy(a).to(device)


def scene_to_tiles(scene, origins, tile, layout="nhwc4"):
    """scene: device uint8 [H, W, 3]; origins: device int32 [n, 2] -> float32 [n, tile, tile, 4] (ToTensor + Normalize, outside = 0), the
    plain U-Net's stem input; layout="nchw": the same values as planar [n, 3, tile, tile], the input of every other model's forward."""
    if layout not in ("nhwc4", "nchw"):
        raise ValueError("layout must be 'nhwc4' or 'nchw'")
    h, w, _ = scene.shape
    n = origins.shape[0]
    out = torch.empty((n, tile, tile, 4) if layout == "nhwc4" else (n, 3, tile, tile), device=scene.device, dtype=torch.float32)
    m, s = data.IMAGENET_MEAN, data.IMAGENET_STD
    fn = lib.runet_scene_to_tiles if layout == "nhwc4" else lib.runet_scene_to_tiles_nchw
    check(fn(scene.data_ptr(), h, w, scene.stride(0), origins.data_ptr(), n, tile, m[0], m[1], m[2], s[0], s[1], s[2], out.data_ptr(),
             ops.stream()))
    return out


def argmax_stitch(z4, origins, halo, mask, n_classes=2):
    """z4: the head's NHWC output [n, T, T, 4]; writes the class index of every tile's core into mask (device uint8 [H, W])."""
    n, tile = z4.shape[0], z4.shape[1]
    check(lib.runet_argmax_stitch(z4.data_ptr(), n, tile, n_classes, origins.data_ptr(), halo, mask.data_ptr(), mask.shape[0], mask.shape[1],
                                  ops.stream()))
    return mask


def threshold_stitch(prob, origins, halo, mask, threshold=0.5, soft=None):
    """prob: a model's output [n, 1, T, T] (or [n, T, T]), contiguous float32; writes `prob > threshold` (torch's rule on an fp32 tensor: NaN
    is 0, the threshold itself is 0) of every tile's core into mask (device uint8 [H, W]) and, if given, the cores' probabilities bit for bit
    into soft (device float32 [H, W])."""
    if prob.dim() == 4 and prob.shape[1] == 1:
        prob = prob[:, 0]
    if prob.dim() != 3 or prob.shape[1] != prob.shape[2] or prob.dtype != torch.float32 or not prob.is_contiguous():
        raise ValueError("prob must be a contiguous float32 [n, 1, T, T] tensor")
    if origins.dtype != torch.int32 or tuple(origins.shape) != (prob.shape[0], 2) or not origins.is_contiguous():
        raise ValueError("origins must be a contiguous int32 [n, 2] tensor, one row per tile")
    if mask.dtype != torch.uint8 or mask.dim() != 2 or not mask.is_contiguous():
        raise ValueError("mask must be a contiguous uint8 [H, W] tensor")
    if soft is not None and (soft.dtype != torch.float32 or soft.shape != mask.shape or not soft.is_contiguous()):
        raise ValueError("soft must be a contiguous float32 tensor of the mask's shape")
    if any(t.device != prob.device for t in (origins, mask) + (() if soft is None else (soft,))):
        raise ValueError("prob, origins, mask and soft must live on one device")
    check(lib.runet_threshold_stitch(prob.data_ptr(), prob.shape[0], prob.shape[1], origins.data_ptr(), int(halo), float(threshold),
                                     mask.data_ptr(), None if soft is None else soft.data_ptr(), mask.shape[0], mask.shape[1], ops.stream()))
    return mask


def resize_nearest(src, size, out=None):
    """cv2.resize(src, (W, H), interpolation=INTER_NEAREST) of a device uint8 mask; size = (H, W).  The same size returns src itself."""
    dh, dw = size
    if (dh, dw) == tuple(src.shape) and out is None:
        return src
    if out is None:
        out = torch.empty((dh, dw), device=src.device, dtype=torch.uint8)
    if (dh, dw) == tuple(src.shape):
        return out.copy_(src)
    check(lib.runet_resize_nearest_u8(src.data_ptr(), src.shape[0], src.shape[1], out.data_ptr(), dh, dw, ops.stream()))
    return out


def dilate_diff(mask, k=5, coast=None, counts=None, want_dilated=False):
    """-> (coastline = dilate(mask, ellipse k) - mask, counts int32 [2] = (water, coastline pixels), dilated or None), all on the device."""
    ellipse_spans(k)                                     # ValueError for an even / too large k, before anything is allocated
    h, w = mask.shape
    if coast is None:
        coast = torch.empty((h, w), device=mask.device, dtype=torch.uint8)
    if counts is None:
        counts = torch.empty(2, device=mask.device, dtype=torch.int32)
    dil = torch.empty((h, w), device=mask.device, dtype=torch.uint8) if want_dilated else None
    if dil is not None and (dil.data_ptr() - coast.data_ptr()) % 16:
        raise RuntimeError("allocator returned masks of different 16-byte phase")
    check(lib.runet_dilate_diff_u8(mask.data_ptr(), h, w, int(k), coast.data_ptr(), dil.data_ptr() if want_dilated else None, counts.data_ptr(),
                                   ops.stream()))
    return coast, counts, dil


# ------------------------------------------------------------------------------------------------ contours (host)
# the 8 neighbours in counter-clockwise order as seen on the image (y grows downwards): E, NE, N, NW, W, SW, S, SE
_DI = (0, -1, -1, -1, 0, 1, 1, 1)
_DJ = (1, 1, 0, -1, -1, -1, 0, 1)


def trace_external_contours(mask):
    """cv2.findContours(mask, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) by Suzuki-Abe border following (8-connected): the outer border of every
    top-level component, in raster order of their start pixels, each an int32 [n, 2] array of (x, y) with collinear runs reduced to their end
    points.  Border pixels are marked +id (the pixel to the right not seen to be background) or -id (right neighbour is background), and a
    start candidate whose last marked pixel to the left is positive lies inside a traced border and is skipped - which is how holes and what is
    inside them stay out.  Only candidates (pixel set, left neighbour clear: found with numpy) and border pixels are visited from Python."""
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError("mask must be 2-D")
    h, w = m.shape
    img = np.zeros((h + 2, w + 2), dtype=np.int32)
    img[1:-1, 1:-1] = m != 0
    cand_i, cand_j = np.nonzero((img[:, 1:] == 1) & (img[:, :-1] == 0))
    cand_j = cand_j + 1
    W = w + 2
    flat = img.reshape(-1)
    f = memoryview(flat)
    off = [_DI[d] * W + _DJ[d] for d in range(8)]
    contours = []
    nbd = 1
    for i, j in zip(cand_i.tolist(), cand_j.tolist()):
        p0 = i * W + j
        if f[p0] != 1:
            continue                                     # already on a traced border
        left = img[i, :j]
        marked = np.flatnonzero((left > 1) | (left < 0))
        if marked.size and left[marked[-1]] > 0:
            continue                                     # inside an outer border: a hole's far side, or an island in a hole
        nbd += 1
        # first neighbour clockwise from the west one
        d1 = -1
        for s in range(8):
            d = (4 - s) % 8
            if f[p0 + off[d]] != 0:
                d1 = d
                break
        if d1 < 0:
            f[p0] = -nbd
            contours.append(np.array([[j - 1, i - 1]], dtype=np.int32))
            continue
        p1 = p0 + off[d1]
        pts, dirs = [], []                               # visited pixels and the direction each was LEFT in
        p3, d_from = p0, d1                              # d_from: direction from p3 to the previous pixel p2
        while True:
            east_clear = False
            d = d_from
            for _ in range(8):
                d = (d + 1) % 8
                if f[p3 + off[d]] != 0:
                    break
                if d == 0:
                    east_clear = True
            p4 = p3 + off[d]
            if east_clear:
                f[p3] = -nbd
            elif f[p3] == 1:
                f[p3] = nbd
            pts.append(p3)
            dirs.append(d)
            if p4 == p0 and p3 == p1:
                break
            p3, d_from = p4, (d + 4) % 8
        n = len(pts)
        keep = [t for t in range(n) if dirs[t] != dirs[t - 1]] if n > 1 else [0]
        pa = np.array([pts[t] for t in keep], dtype=np.int64)
        contours.append(np.stack([pa % W - 1, pa // W - 1], axis=1).astype(np.int32))
    return contours


# ------------------------------------------------------------------------------------------------ contours (device)
def _trace_packed(mask, min_points=0, with_sizes=False):
    """mask: device uint8 [h, w] -> device int32 tensor {n, total, offsets [n + 1], points [total][2]} (csrc/contours.hip), or None for a
    mask without a set pixel.  Two small downloads: the state count, then (n, total) to cut the packed result to its length.
    with_sizes: -> (packed, (n, total)), so that a caller that goes on working on the device need not read them again."""
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or mask.ndim != 2 or not mask.is_cuda:
        raise ValueError("expected a 2-D uint8 device tensor")
    if min_points < 0:
        raise ValueError("min_points must not be negative")
    mask = mask.contiguous()
    h, w = mask.shape
    if h == 0 or w == 0:
        return (None, (0, 0)) if with_sizes else None
    nbytes = lib.runet_contours_workspace_bytes(h, w)
    if nbytes < 0:
        raise ValueError(f"a {h} x {w} mask is too large for the device tracer (h * w must stay below 2^31)")
    ws = torch.empty(nbytes, device=mask.device, dtype=torch.uint8)
    count = torch.empty(1, device=mask.device, dtype=torch.int64)
    check(lib.runet_contours_count(mask.data_ptr(), h, w, ws.data_ptr(), nbytes, count.data_ptr(), ops.stream()))
    n_states = int(count.cpu()[0])                                                     # download 1
    if n_states == 0:
        return (None, (0, 0)) if with_sizes else None
    sbytes = lib.runet_contours_state_workspace_bytes(n_states)
    if sbytes < 0:
        raise ValueError(f"{n_states} border states do not fit int32")
    sws = torch.empty(sbytes, device=mask.device, dtype=torch.uint8)
    check(lib.runet_contours_trace(h, w, ws.data_ptr(), nbytes, n_states, int(min_points), sws.data_ptr(), sbytes, ops.stream()))
    n, total = (int(v) for v in sws[:8].view(torch.int32).cpu())                       # download 2
    packed = sws[:4 * (3 + n + 2 * total)].view(torch.int32)
    return (packed, (n, total)) if with_sizes else packed


def _unpack_contours(packed):
    """host int32 {n, total, offsets [n + 1], points [total][2]} -> list of int32 [k, 2] arrays"""
    packed = np.asarray(packed, dtype=np.int32)
    n, total = int(packed[0]), int(packed[1])
    off = packed[2:3 + n]
    pts = packed[3 + n:3 + n + 2 * total].reshape(total, 2)
    return [pts[off[i]:off[i + 1]].copy() for i in range(n)]


def trace_external_contours_device(mask, min_points=0):
    """trace_external_contours(mask.cpu().numpy()) computed on the device (runet_contours_count / runet_contours_trace), the same arrays in the
    same order; min_points > 0 also drops the contours with <= min_points vertices there (the reference's filter is 10).  The mask stays on
    the device: three downloads, two size words and the packed vertices."""
    packed = _trace_packed(mask, min_points)
    return [] if packed is None else _unpack_contours(packed.cpu().numpy())            # download 3


def arc_length(points, closed=True):
    p = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    if len(p) < 2:
        return 0.0
    d = np.diff(np.vstack([p, p[:1]]) if closed else p, axis=0)
    return float(np.hypot(d[:, 0], d[:, 1]).sum())


def _seg_dist(p, a, b):
    ab = b - a
    den = float(ab @ ab)
    t = np.clip(((p - a) @ ab) / den, 0.0, 1.0) if den > 0 else np.zeros(len(p))
    q = a + t[:, None] * ab
    return np.hypot(p[:, 0] - q[:, 0], p[:, 1] - q[:, 1])


def _dp_chain(p, eps):
    """Douglas-Peucker on an open chain: indices of the kept points (both ends kept)."""
    keep = np.zeros(len(p), dtype=bool)
    keep[0] = keep[-1] = True
    stack = [(0, len(p) - 1)]
    while stack:
        a, b = stack.pop()
        if b - a < 2:
            continue
        d = _seg_dist(p[a + 1:b], p[a], p[b])
        k = int(d.argmax())
        if d[k] > eps:
            k += a + 1
            keep[k] = True
            stack += [(a, k), (k, b)]
    return np.flatnonzero(keep)


def approx_poly_dp(points, eps, closed=True):
    """cv2.approxPolyDP: Douglas-Peucker with tolerance eps (every dropped vertex within eps of the segment that replaces it).  A closed curve
    is split at its first vertex and the vertex farthest from it.  -> int32 [n, 2]"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    n = len(p)
    if n <= 2:
        return np.asarray(points, dtype=np.int32).reshape(-1, 2)
    if not closed:
        idx = _dp_chain(p, eps)
    else:
        far = int(np.hypot(*(p - p[0]).T).argmax())
        if far == 0:
            return np.asarray(points, dtype=np.int32).reshape(-1, 2)[:1]
        a = _dp_chain(p[:far + 1], eps)
        b = _dp_chain(np.vstack([p[far:], p[:1]]), eps) + far
        idx = np.concatenate([a, b[1:-1]])
    return np.asarray(points, dtype=np.int32).reshape(-1, 2)[idx]


def _simplify(contours, min_points, eps_factor):
    return [approx_poly_dp(c, eps_factor * arc_length(c, True), True).tolist() for c in contours if len(c) > min_points]


# ------------------------------------------------------------------------------------------------ the exact rule (include/runet_hip.h)
def _check_rule(rule):
    if rule not in SIMPLIFY_RULES:
        raise ValueError(f"rule must be one of {SIMPLIFY_RULES} (got {rule!r})")


def _check_eps_factor(eps_factor):
    eps_factor = float(eps_factor)
    if not (0.0 <= eps_factor < float("inf")):
        raise ValueError("eps_factor must be finite and not negative")
    return eps_factor


def _exact_numerator(a, b, p):
    """-> (N, den): den * the squared distance of p to the clipped segment a-b, in Python ints; 1 stands in for den == 0"""
    abx, aby, apx, apy = b[0] - a[0], b[1] - a[1], p[0] - a[0], p[1] - a[1]
    den, dot, ap2 = abx * abx + aby * aby, apx * abx + apy * aby, apx * apx + apy * apy
    if den == 0:
        return ap2, 1
    if dot <= 0:
        return ap2 * den, den
    if dot >= den:
        return ((p[0] - b[0]) ** 2 + (p[1] - b[1]) ** 2) * den, den
    return (apx * aby - apy * abx) ** 2, den


def approx_poly_dp_exact(points, eps_factor):
    """Douglas-Peucker on one closed integer contour by the exact rule stated in include/runet_hip.h (the host restatement of
    runet_contours_simplify: Python ints, and float64 operations that are each rounded once), tolerance eps_factor * arc length.
    -> int32 [k, 2].  ValueError on a bad input: a coordinate outside [0, 46340] or an edge that is not horizontal, vertical or 45 degrees."""
    eps_factor = _check_eps_factor(eps_factor)
    arr = np.asarray(points)
    if arr.size and not np.issubdtype(arr.dtype, np.integer):
        raise ValueError("the exact rule takes integer vertices")
    p = [(int(x), int(y)) for x, y in arr.reshape(-1, 2)]
    n = len(p)
    if n == 0:
        return np.zeros((0, 2), dtype=np.int32)
    axis = diag = 0
    for i, (x, y) in enumerate(p):
        if not (0 <= x <= EXACT_COORD_MAX and 0 <= y <= EXACT_COORD_MAX):
            raise ValueError(f"vertex {i} = ({x}, {y}) is outside [0, {EXACT_COORD_MAX}]")
    for i, (x, y) in enumerate(p):
        xn, yn = p[(i + 1) % n]
        dx, dy = abs(xn - x), abs(yn - y)
        if dx == 0 or dy == 0:
            axis += dx + dy
        elif dx == dy:
            diag += dx
        else:
            raise ValueError(f"edge {i} = ({xn - x}, {yn - y}) is not a horizontal, vertical or 45 degree run")
    length = np.float64(axis) + np.float64(diag) * np.float64(_SQRT2)
    eps = np.float64(eps_factor) * length
    thr = eps * eps
    d2 = [(x - p[0][0]) ** 2 + (y - p[0][1]) ** 2 for x, y in p]
    far = d2.index(max(d2))
    if far == 0:
        return np.array(p[:1], dtype=np.int32)
    q = p + p[:1]
    keep = {0, far}
    stack = [(0, far), (far, n)]
    while stack:
        a, b = stack.pop()
        if b - a < 2:
            continue
        best, k, den = -1, -1, 1
        for i in range(a + 1, b):
            num, den = _exact_numerator(q[a], q[b], q[i])
            if num > best:
                best, k = num, i
        if np.float64(float(best)) > thr * np.float64(float(den)):
            keep.add(k)
            stack += [(a, k), (k, b)]
    return np.array([p[i] for i in sorted(keep)], dtype=np.int32)


def _simplify_exact(contours, min_points, eps_factor):
    return [approx_poly_dp_exact(c, eps_factor).tolist() for c in contours if len(c) > min_points]


def simplify_packed_device(packed, eps_factor=0.002, lds_max_vertices=None, sizes=None, with_head=False):
    """packed: the tracer's device int32 tensor {n, total, offsets [n + 1], points [total][2]} -> the same format with every contour
    simplified by the exact rule on the device (runet_contours_simplify).  sizes = (n, total) where the caller has read them already;
    otherwise they are one small download.  One more small download follows, the head {n, kept vertices, bad inputs, largest round count},
    to cut the result to its length.  lds_max_vertices: the contour length up to which the per-vertex state stays in LDS (None: the
    library's default), same bytes for every value.  ValueError when an input is bad (see approx_poly_dp_exact); with_head: -> (result, head)."""
    if not isinstance(packed, torch.Tensor) or packed.dtype != torch.int32 or packed.ndim != 1 or not packed.is_cuda:
        raise ValueError("expected a 1-D int32 device tensor")
    eps_factor = _check_eps_factor(eps_factor)
    packed = packed.contiguous()
    if sizes is None:
        if packed.numel() < 3:
            raise ValueError("a packed contour set has at least three words")
        sizes = packed[:2].cpu().tolist()
    n, total = int(sizes[0]), int(sizes[1])
    nbytes = lib.runet_contours_simplify_workspace_bytes(n, total)
    if nbytes < 0 or packed.numel() < 3 + n + 2 * total:
        raise ValueError(f"n = {n}, total = {total} do not describe a packed contour set of {packed.numel()} words")
    ws = torch.empty(nbytes, device=packed.device, dtype=torch.uint8)
    lds = -1 if lds_max_vertices is None else max(0, min(int(lds_max_vertices), 2 ** 31 - 1))
    check(lib.runet_contours_simplify(packed.data_ptr(), n, total, eps_factor, lds, ws.data_ptr(), nbytes, ops.stream()))
    head = [int(v) for v in ws[:16].view(torch.int32).cpu()]
    if head[2]:
        raise ValueError(f"{head[2]} bad inputs: the exact rule takes coordinates in [0, {EXACT_COORD_MAX}] and horizontal, vertical or "
                         "45 degree edges, in a packed set whose offsets rise from 0 to its vertex count")
    at = lib.runet_contours_simplify_result_offset()
    out = ws[at:at + 4 * (3 + n + 2 * head[1])].view(torch.int32)
    return (out, head) if with_head else out


def _check_exact_shape(h, w):
    if max(h, w) > EXACT_COORD_MAX + 1:
        raise ValueError(f"rule 'exact' takes masks of at most {EXACT_COORD_MAX + 1} pixels a side (coordinates up to {EXACT_COORD_MAX}); "
                         f"got {h} x {w}")


def _coastlines_packed(coast, min_points, eps_factor, rule):
    """device mask -> (device packed contours or None, simplified): traced on the device and, under rule "exact" with DEVICE_SIMPLIFY on,
    simplified there too, so that only the kept vertices are downloaded"""
    if rule == "exact" and DEVICE_SIMPLIFY:
        packed, sizes = _trace_packed(coast, min_points, with_sizes=True)
        return (None if packed is None else simplify_packed_device(packed, eps_factor, sizes=sizes)), True
    return _trace_packed(coast, min_points), False


def _finish_contours(contours, simplified, min_points, eps_factor, rule):
    """downloaded contours -> coastlines: whatever of the rule has not run on the device"""
    if simplified:
        return [c.tolist() for c in contours]
    return (_simplify_exact if rule == "exact" else _simplify)(contours, min_points, eps_factor)


def coastlines_from_mask(coastline_mask, min_points=10, eps_factor=0.002, rule="float64"):
    """predict_coastline.py:605-616 -> list of [[x, y], ...].  A device tensor is traced and length-filtered on the device and its packed
    vertices downloaded once (DEVICE_CONTOURS off: the mask is downloaded and traced on the host).
    rule "float64" (the default): arc length and Douglas-Peucker on the host in float64 (approx_poly_dp) either way, so the lists are the same.
    rule "exact": the project's exact integer rule (include/runet_hip.h), which parts from the float64 rule at ties and near-ties only.  A
    device mask is traced AND simplified on the device and only the kept vertices are downloaded (DEVICE_SIMPLIFY off: the traced contours
    are downloaded and simplified by approx_poly_dp_exact); a host mask goes through the host tracer and approx_poly_dp_exact.  The lists
    are identical whichever way.  Masks of more than 46341 pixels a side are refused under "exact"."""
    _check_rule(rule)
    if rule == "exact":
        if getattr(coastline_mask, "ndim", 2) == 2:
            _check_exact_shape(*coastline_mask.shape)
        _check_eps_factor(eps_factor)
    if isinstance(coastline_mask, torch.Tensor):
        if coastline_mask.is_cuda and DEVICE_CONTOURS:
            if rule == "float64":
                return _simplify(trace_external_contours_device(coastline_mask, min_points), min_points, eps_factor)
            packed, simplified = _coastlines_packed(coastline_mask, min_points, eps_factor, rule)
            contours = [] if packed is None else _unpack_contours(packed.cpu().numpy())
            return _finish_contours(contours, simplified, min_points, eps_factor, rule)
        coastline_mask = coastline_mask.cpu().numpy()
    return (_simplify_exact if rule == "exact" else _simplify)(trace_external_contours(coastline_mask), min_points, eps_factor)


# ------------------------------------------------------------------------------------------------ the extractor
def _load_rgb(image):
    """-> (PIL RGB image, path or None)"""
    if isinstance(image, (str, os.PathLike)):
        return Image.open(image).convert("RGB"), os.fspath(image)
    if isinstance(image, Image.Image):
        return image.convert("RGB"), None
    a = np.asarray(image)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("image must be a path, a PIL image or a uint8 [H, W, 3] array")
    return Image.fromarray(np.ascontiguousarray(a)), None


def _as_bands(image, bands):
    """The rule that tells a band raster from an RGB image.  -> the raster input, or None for an image.  A raster is: whatever comes through
    `bands=`; a .npy path; a numpy array or tensor with ndim == 3 and shape[0] <= 6 that is not a uint8 [H, W, 3] image (a uint8 array whose
    last axis is 3 stays an image, as before: pass such a raster through `bands=`).  Every other path, .tif included, is an image file for
    PIL, as before: a multi-band .tif goes through `bands=` (and needs GDAL)."""
    if bands is not None:
        if image is not None:
            raise ValueError("pass either an image or bands=, not both")
        return bands
    if isinstance(image, (str, os.PathLike)):
        return image if os.path.splitext(os.fspath(image))[1].lower() == ".npy" else None
    if isinstance(image, (np.ndarray, torch.Tensor)) and image.ndim == 3 and image.shape[0] <= _scene.MAX_BANDS:
        is_u8 = image.dtype == (torch.uint8 if isinstance(image, torch.Tensor) else np.uint8)
        return None if is_u8 and image.shape[2] == 3 else image
    return None


def save_extraction_result(result, output_dir, report=False):
    """predict_coastline.py:620-652: <base>_water_mask.png, <base>_coastline_mask.png (* 255) and <base>_coastlines.json with the
    reference's keys.  report=True: also the reference's fourth product, <base>_coastsat_analysis.png (report.py), drawn from
    result["report"] (computed from the result where it is missing, and stored there); that alone needs matplotlib."""
    os.makedirs(output_dir, exist_ok=True)
    base = os.path.splitext(os.path.basename(str(result["image_path"])))[0]
    Image.fromarray(result["water_mask"] * 255).save(os.path.join(output_dir, f"{base}_water_mask.png"))
    Image.fromarray(result["coastline_mask"] * 255).save(os.path.join(output_dir, f"{base}_coastline_mask.png"))
    doc = {"image_path": result["image_path"], "image_size": result["image_size"], "coastlines": result["coastlines"],
           "coastline_count": result["coastline_count"], "dilation_size": result.get("dilation_size", 5),
           "extraction_time": result["extraction_time"]}
    if "cleanup" in result:
        doc["cleanup"] = result["cleanup"]
    with open(os.path.join(output_dir, f"{base}_coastlines.json"), "w", encoding="utf-8") as fh:
        json.dump(doc, fh, indent=2, ensure_ascii=False)
    if report:
        from . import report as _report
        if "report" not in result:
            result["report"] = _report.analysis_report(result)
        _report.create_coastsat_style_visualization(result, output_dir, report=result["report"])


def _check_cleanup(min_water_area, min_land_area, connectivity):
    """-> (min_water, min_land, connectivity) as clean_water_mask takes them; ValueError otherwise"""
    from . import components as _cc
    return (_cc._check_area(min_water_area, "min_water_area"), _cc._check_area(min_land_area, "min_land_area"),
            _cc._check_connectivity(connectivity))


def _clean_in_place(water, min_water, min_land, connectivity, counts):
    """water: dense device uint8 [h, w], cleaned where it lies (components.clean_water_mask's two steps, frame components exempt);
    counts: device int64 [1, 4], the four figures of its info.  Nothing is read back on the device route."""
    from . import components as _cc
    if _cc._host_route():
        out, c = _cc._clean_host(water.cpu().numpy()[None], min_water, min_land, connectivity, True)
        water.copy_(torch.from_numpy(out[0]))
        counts.copy_(torch.from_numpy(c))
    else:
        _cc._clean_device(water[None], min_water, min_land, connectivity, True, counts)


def _raise_nonfinite(count):
    if count:
        raise ValueError(f"the selected bands hold {count} non-finite values: mask them (nodata) before the stretch")


PROB_MODELS = {"RobustUNet": "model", "DeepLabV3Plus": "deeplab", "SegNet": "segnet", "YOLOSeg": "yolo", "SegFormerLite": "segformer",
               "HRNetWater": "hrnet", "WaterNet": "waternet", "MSWNet": "mswnet", "FastSCNN": "fastscnn", "ENet": "enet", "PSPNet": "pspnet"}


def _is_prob_model(model):
    """one of the project's models whose forward(x [N, 3, H, W]) returns sigmoid probabilities [N, 1, H, W] (class name -> its module)"""
    import importlib
    return any(isinstance(model, getattr(importlib.import_module(f"{__package__}.{mod}"), name)) for name, mod in PROB_MODELS.items())


class CoastlineExtractor:
    """Drop-in for the reference's class (predict_coastline.py:336): same constructor and method names, results as described above.
    model: a UNet (2-class logits, arg-max) or one of PROB_MODELS (1-channel probabilities, `> threshold`) with its weights loaded.
    simplify_rule: "float64" (the default: host Douglas-Peucker in float64, as before) or "exact" (coastlines_from_mask): the contours are
    then simplified on the device too, the simplified packed contours ride in the one result download in place of the raw ones, and one
    more small size word (the simplifier's head) is read before it.  The result dict and save_extraction_result are the same."""

    def __init__(self, model_path=None, device="cuda", model=None, input_size=512, threshold=0.5, simplify_rule="float64"):
        from .unet import UNet
        _check_rule(simplify_rule)
        self.simplify_rule = simplify_rule
        self.device = torch.device(device)
        self.input_size = int(input_size)
        self.threshold = float(threshold)
        if model is None:
            model = UNet(n_channels=3, n_classes=2)
            if model_path and os.path.exists(model_path):
                model.load_state_dict(torch.load(model_path, map_location="cpu", weights_only=True))
        self.prob = not isinstance(model, UNet)
        if self.prob and not _is_prob_model(model):
            raise TypeError("model must be a UNet (2-class logits) or one of the project's probability models: " + ", ".join(PROB_MODELS))
        self.model = model.eval()
        self._check_size(self.input_size, "input_size")          # before the parameters move: a refused size allocates nothing
        self.model = model.to(self.device)

    def _check_size(self, size, what):
        """ValueError unless the model takes size x size inputs: the model's own rule (_check_input), asked on a shape-only tensor"""
        if size <= 0:
            raise ValueError(f"{what} must be positive (got {size})")
        try:
            self.model._check_input(torch.empty((1, 3, size, size), device="meta"))
        except ValueError as e:
            raise ValueError(f"{what} = {size} is not a size {type(self.model).__name__} takes: {e}") from None

    # -- network ---------------------------------------------------------------------------------
    def _z4(self, tiles):
        from .unet import unet_forward
        with torch.no_grad(), ops.precision(self.model.precision):
            return unet_forward(self.model, tiles, save=False, nhwc=True)[0]

    def _prob(self, tiles):
        with torch.no_grad():
            p = self.model(tiles)                                # the models apply their own ops.precision
        n, t = tiles.shape[0], tiles.shape[-1]
        if not isinstance(p, torch.Tensor) or p.dtype != torch.float32 or tuple(p.shape) != (n, 1, t, t) or not p.is_contiguous():
            raise ValueError(f"{type(self.model).__name__} must return a contiguous float32 [{n}, 1, {t}, {t}] tensor")
        return p

    def _stitch_tiles(self, scene, origins, tile, halo, mask, soft=None):
        """tiles -> network -> cores into mask: the one place where the two model families part (tile layout and stitch rule)"""
        if self.prob:
            threshold_stitch(self._prob(scene_to_tiles(scene, origins, tile, "nchw")), origins, halo, mask, self.threshold, soft)
        else:
            argmax_stitch(self._z4(scene_to_tiles(scene, origins, tile)), origins, halo, mask, self.model.n_classes)

    def _predict_resized(self, pil, out=None):
        """steps 1-3: -> device uint8 [H, W] water mask at the image's own size"""
        s = self.input_size
        scene = torch.from_numpy(np.array(data.Resize((s, s))(pil), dtype=np.uint8)).to(self.device)
        origin = torch.zeros((1, 2), device=self.device, dtype=torch.int32)
        w, h = pil.size
        same = (h, w) == (s, s)
        pred = out if same and out is not None else torch.empty((s, s), device=self.device, dtype=torch.uint8)
        self._stitch_tiles(scene, origin, s, 0, pred)
        return pred if same else resize_nearest(pred, (h, w), out=out)

    def _predict_tiled(self, scene, tile, halo, batch, out=None, soft=None):
        h, w, _ = scene.shape
        plan = tile_plan(h, w, tile, halo, multiple=1)           # the model has been asked about the tile (_check_size)
        if batch < 1:
            raise ValueError("batch must be at least 1")
        origins = torch.from_numpy(plan).to(self.device)
        mask = out if out is not None else torch.empty((h, w), device=self.device, dtype=torch.uint8)
        for i in range(0, len(plan), batch):
            o = origins[i:i + batch]
            self._stitch_tiles(scene, o, tile, halo, mask, soft)
        return mask

    def predict_scene(self, image=None, tile=512, halo=64, batch=8, as_tensor=False, bands=None, mode="water", return_prob=False):
        """Water mask at the scene's own resolution, no resize: tiles of side `tile` whose cores (tile - 2 * halo) partition the scene, `batch`
        tiles per network call.  Each pixel comes from exactly one core.  Beyond the scene the tiles read 0.0 (normalised units).
        A band raster (_as_bands) is enhanced on the device first (scene.py, `mode`) and goes straight into the tiles.
        return_prob (probability models only): -> (mask, prob_map), the float32 [h, w] probabilities of the same cores from the same stitch
        launch (Extended_Baseline_Comparison.py:954 draws its error maps from it); a device tensor with as_tensor, numpy otherwise."""
        self._check_size(tile, "tile")
        if return_prob and not self.prob:
            raise ValueError("return_prob needs a probability model: a UNet's outputs are logits")

        def soft_map(h, w):
            return torch.empty((h, w), device=self.device, dtype=torch.float32) if return_prob else None

        raster = _as_bands(image, bands)
        if raster is not None:
            r = _scene.load_raster(raster, self.device)
            scene, nonfinite = _scene._enhance(r, mode)
            soft = soft_map(r.h, r.w)
            if as_tensor:
                mask = self._predict_tiled(scene, tile, halo, batch, soft=soft)
                return (mask, soft) if return_prob else mask
            # water mask | non-finite count: one download
            seg = (r.h * r.w + 15) // 16 * 16
            buf = torch.empty(seg + 16, device=self.device, dtype=torch.uint8)
            self._predict_tiled(scene, tile, halo, batch, out=buf[:r.h * r.w].view(r.h, r.w), soft=soft)
            buf[seg:seg + 4].view(torch.int32).copy_(nonfinite)
            host = buf.cpu().numpy()
            _raise_nonfinite(int(host[seg:seg + 4].view(np.int32)[0]))
            mask = host[:r.h * r.w].reshape(r.h, r.w).copy()
            return (mask, soft.cpu().numpy()) if return_prob else mask
        pil, _ = _load_rgb(image)
        scene = _dev_u8(np.array(pil, dtype=np.uint8), self.device)
        soft = soft_map(scene.shape[0], scene.shape[1])
        mask = self._predict_tiled(scene, tile, halo, batch, soft=soft)
        if not as_tensor:
            mask, soft = mask.cpu().numpy(), None if soft is None else soft.cpu().numpy()
        return (mask, soft) if return_prob else mask

    # -- reference surface -----------------------------------------------------------------------
    def extract_coastline_contours(self, water_mask, dilation_kernel_size=5, min_water_area=0, min_land_area=0, connectivity=8):
        """-> (coastlines, coastline_mask) as predict_coastline.py:583-618; water_mask: numpy array or device tensor, uint8.
        min_water_area / min_land_area > 0: a copy of the mask is cleaned first (components.clean_water_mask), on the device."""
        min_water, min_land, connectivity = _check_cleanup(min_water_area, min_land_area, connectivity)
        mask = _dev_u8(water_mask, self.device)
        if min_water or min_land:
            if isinstance(water_mask, torch.Tensor) and mask.data_ptr() == water_mask.data_ptr():
                mask = mask.clone()
            _clean_in_place(mask, min_water, min_land, connectivity, torch.empty((1, 4), device=mask.device, dtype=torch.int64))
        coast, _, _ = dilate_diff(mask, dilation_kernel_size)
        rule = self.simplify_rule
        if rule == "exact":
            _check_exact_shape(*coast.shape)
        if not (coast.is_cuda and DEVICE_CONTOURS):
            coast = coast.cpu().numpy()
            return coastlines_from_mask(coast, rule=rule), coast
        # trace (rule "exact": and simplify) before the download; packed contours | coastline mask -> one download
        packed, simplified = _coastlines_packed(coast, 10, 0.002, rule)
        head = 0 if packed is None else 4 * packed.numel()
        host = (coast.view(-1) if packed is None else torch.cat([packed.view(torch.uint8), coast.view(-1)])).cpu().numpy()
        contours = [] if packed is None else _unpack_contours(host[:head].view(np.int32))
        return _finish_contours(contours, simplified, 10, 0.002, rule), host[head:].reshape(coast.shape).copy()

    def extract_coastline_from_image(self, image=None, output_dir=None, dilation_size=5, tiled=False, tile=512, halo=64, batch=8, bands=None,
                                     mode="water", report=False, min_water_area=0, min_land_area=0, connectivity=8):
        """predict_coastline.py:366-423.  `image`: a path, a PIL image or a uint8 [H, W, 3] array as before, or a band raster (_as_bands),
        which is enhanced on the device (scene.py, `mode`): tiled, the enhanced scene feeds the tiles directly; resized, it is downloaded
        once for the PIL bilinear resize, the reference's order.
        report=True: the result gains "report" (report.analysis_report's arrays), computed from the masks and the scene while they are on
        the device, before the download; a raster's background is its "display"-mode image, its histograms are NDWI from four bands on.
        With output_dir the analysis PNG is written too (matplotlib).
        min_water_area / min_land_area > 0: the predicted water mask is cleaned on the device before the band is made
        (components.clean_water_mask with `connectivity`; components that touch the image frame stay), so that water_mask, water_pixels,
        the band, the contours and the report all describe the cleaned mask; the result gains "cleanup", the filter's four counts and
        the three parameters.  The counts ride in the one download.  With both at 0 (the default) nothing is launched or added."""
        ellipse_spans(dilation_size)
        min_water, min_land, connectivity = _check_cleanup(min_water_area, min_land_area, connectivity)
        cleanup = bool(min_water or min_land)
        rule = self.simplify_rule
        if tiled:
            self._check_size(tile, "tile")
        raster = _as_bands(image, bands)
        scene = nonfinite = None
        if raster is not None:
            r = _scene.load_raster(raster, self.device)
            path = r.meta.get("path")
            if tiled:
                scene, nonfinite = _scene._enhance(r, mode)
                pil, (w, h) = None, (r.w, r.h)
            else:
                pil = Image.fromarray(_scene.enhance_scene(r, mode))
                w, h = pil.size
        else:
            pil, path = _load_rgb(image)
            w, h = pil.size
        if rule == "exact":
            _check_exact_shape(h, w)
        # one device buffer for everything that goes back: water mask | coastline mask | the two counts -> one download
        # (with a cleanup: | its four 64-bit counts)
        seg = (h * w + 15) // 16 * 16
        tail = 2 * seg + 16 + (32 if cleanup else 0)
        buf = torch.empty(tail, device=self.device, dtype=torch.uint8)
        water, coast = buf[:h * w].view(h, w), buf[seg:seg + h * w].view(h, w)
        counts = buf[2 * seg:2 * seg + 8].view(torch.int32)
        if scene is not None:
            self._predict_tiled(scene, tile, halo, batch, out=water)
            buf[2 * seg + 8:2 * seg + 12].view(torch.int32).copy_(nonfinite)
        elif tiled:
            self._predict_tiled(_dev_u8(np.array(pil, dtype=np.uint8), self.device), tile, halo, batch, out=water)
        else:
            self._predict_resized(pil, out=water)
        if cleanup:
            _clean_in_place(water, min_water, min_land, connectivity, buf[2 * seg + 16:tail].view(torch.int64).view(1, 4))
        dilate_diff(water, dilation_size, coast=coast, counts=counts)
        on_device = coast.is_cuda and DEVICE_CONTOURS
        packed, simplified = _coastlines_packed(coast, 10, 0.002, rule) if on_device else (None, False)
        arrays = None
        if report:
            from . import report as _report
            if raster is not None:
                display, bad = _scene._enhance(r, "display")
                _raise_nonfinite(int(bad.item()))
            else:
                display = _dev_u8(np.array(pil, dtype=np.uint8), self.device)
            arrays = _report._device_arrays(display, water, coast, r if raster is not None else None, 50)
        if packed is not None:                           # the packed contours ride along in the one download
            buf = torch.cat([buf, packed.view(torch.uint8)])
        host = buf.cpu().numpy()
        if scene is not None:
            _raise_nonfinite(int(host[2 * seg + 8:2 * seg + 12].view(np.int32)[0]))
        water_np = host[:h * w].reshape(h, w).copy()
        coast_np = host[seg:seg + h * w].reshape(h, w).copy()
        n_water, n_coast = (int(v) for v in host[2 * seg:2 * seg + 8].view(np.int32))
        if on_device:
            contours = [] if packed is None else _unpack_contours(host[tail:].view(np.int32))
            coastlines = _finish_contours(contours, simplified, 10, 0.002, rule)
        else:
            coastlines = coastlines_from_mask(coast_np, rule=rule)
        result = {"image_path": path if path is not None else "image", "image_size": (w, h), "water_mask": water_np,
                  "coastline_mask": coast_np, "coastlines": coastlines, "coastline_count": len(coastlines), "dilation_size": int(dilation_size),
                  "extraction_time": str(datetime.now()), "water_pixels": n_water, "coastline_pixels": n_coast}
        if cleanup:
            from .components import INFO_KEYS
            result["cleanup"] = dict(zip(INFO_KEYS, (int(v) for v in host[2 * seg + 16:tail].view(np.int64))), min_water_area=min_water,
                                     min_land_area=min_land, connectivity=connectivity)
        if arrays is not None:
            result["report"] = _report._with_statistics(arrays, h * w, n_water, n_coast, coastlines)
        if output_dir:
            save_extraction_result(result, output_dir, report=report)
        return result

    save_extraction_result = staticmethod(save_extraction_result)
