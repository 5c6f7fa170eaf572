"""How good is a coastline?  The exact Euclidean distance transform (EDT) on the device and the scores that rest on it.

The reference measures regions only (Main_Final.py:527-547: IoU / precision / recall / F1 / accuracy), and at scene scale those hardly
move when the coastline does.  The questions one asks of a coastline - how far is it from the labelled one (mean, RMS, worst case), what
share lies within t pixels, boundary F-score, Boundary IoU - all reduce to one primitive: for every pixel the squared distance to the
nearest feature pixel, which is an integer and therefore exact (csrc/edt.hip; the rules are stated in include/runet_hip.h).

  distance_transform_sq        d2 = min over feature pixels of dx^2 + dy^2, int32; RUNET_EDT_NONE in an image without features
                                                                                                       runet_edt_sq_u8
  distance_transform_sq_host   the same in numpy: two passes, integers only, no scipy
  coastline_deviation          both directions between two coastline masks: count, unreachable, mean, rms, max, share within t pixels;
                               hausdorff and assd                                                      runet_edt_sq_u8, runet_edt_stats
  boundary_scores              boundary precision / recall / F-score and Boundary IoU of two region masks    (the same two)
  evaluate_coastline           both for a CoastlineExtractor result against a true water mask               + runet_dilate_diff_u8

Only pixels inside the image are features: the frame around a tile is neither water nor land, because a tile edge is not a coast.

Counts, maxima and the sum of d2 are integers from the device; the sum of the distances is a float64 sum in a fixed order; ratios and
roots are taken on the host in float64.  RUNET_NO_DEVICE_EDT=1 (read at every call) sends the transform and its statistics through the
numpy restatement instead: the outputs are identical, bit for bit.  The restatement costs O(h w min(h, w)) in the worst case - it is the
second witness and the route for a machine without the device, not a fast path.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np
import torch

NONE = 2 ** 31 - 1                                       # RUNET_EDT_NONE
MAX_SIDE = 32768
MAX_TOL = 8
NAN = math.nan                                           # one object, so that two result dicts with the same NaNs compare equal


def _host_route():
    return os.environ.get("RUNET_NO_DEVICE_EDT", "") not in ("", "0")


# ------------------------------------------------------------------------------------------------ inputs
def _as_u8(mask):
    """bool / uint8 array or tensor -> the same bytes as uint8, no copy"""
    if isinstance(mask, torch.Tensor):
        if mask.dtype == torch.bool:
            return mask.view(torch.uint8)
        if mask.dtype != torch.uint8:
            raise ValueError(f"expected a bool or uint8 mask (got {mask.dtype})")
        return mask
    a = np.asarray(mask)
    if a.dtype == np.bool_:
        return a.view(np.uint8)
    if a.dtype != np.uint8:
        raise ValueError(f"expected a bool or uint8 mask (got {a.dtype})")
    return a


def _as_batch(mask):
    """-> ([n, h, w] uint8 view, batched)"""
    m = _as_u8(mask)
    if m.ndim not in (2, 3):
        raise ValueError(f"expected a [h, w] or [n, h, w] mask (got shape {tuple(m.shape)})")
    m3 = m if m.ndim == 3 else m[None]
    n, h, w = m3.shape
    if n < 1 or h < 1 or w < 1:
        raise ValueError(f"empty mask (shape {tuple(m.shape)})")
    if h > MAX_SIDE or w > MAX_SIDE:
        raise ValueError(f"h and w must not exceed {MAX_SIDE}, so that every squared distance fits int32 (got {h} x {w})")
    return m3, m.ndim == 3


def _to_host(m):
    return m.cpu().numpy() if isinstance(m, torch.Tensor) else m


def _to_device(m, device):
    return m.to(device) if isinstance(m, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(m)).to(device)


def _place(m, device):
    """the array where this call's route computes: numpy with RUNET_NO_DEVICE_EDT, a device tensor otherwise"""
    return _to_host(m) if _host_route() else _to_device(m, device)


def _cat(parts):
    return torch.cat(parts) if isinstance(parts[0], torch.Tensor) else np.concatenate(parts)


def _u8(m):
    return m.to(torch.uint8) if isinstance(m, torch.Tensor) else m.astype(np.uint8)


def _pair(a, b, what):
    a3, batched = _as_batch(a)
    b3, b_batched = _as_batch(b)
    if tuple(a3.shape) != tuple(b3.shape) or batched != b_batched:
        raise ValueError(f"{what} must have one shape (got {tuple(a3.shape[1 - batched:])} and {tuple(b3.shape[1 - b_batched:])})")
    return a3, b3, batched


# ------------------------------------------------------------------------------------------------ the numpy restatement
def _edt_host_image(feat):
    """bool [h, w] -> int64 [h, w].  Pass 1 along the longer side: the gap to the nearest feature of the same line, by running maxima and
    minima of feature positions.  Pass 2 along the shorter side, literally min over k of k^2 + g(y +- k)^2, stopped once k^2 can improve
    nothing.  A line without a feature is a state of its own (`valid`), never a large distance."""
    h, w = feat.shape
    if h > w:
        return _edt_host_image(feat.T).T
    x = np.arange(w, dtype=np.int64)
    left = np.maximum.accumulate(np.where(feat, x, -1), axis=1)
    right = np.minimum.accumulate(np.where(feat, x, w)[:, ::-1], axis=1)[:, ::-1]
    has_l, has_r = left >= 0, right < w
    valid = has_l | has_r
    g = np.where(has_l & has_r, np.minimum(x - left, right - x), np.where(has_l, x - left, right - x))
    f = np.where(valid, g * g, 0)
    d = np.where(valid, f, NONE)
    for k in range(1, h):
        kk = k * k
        if kk >= int(d.max()):
            break
        d[k:] = np.minimum(d[k:], np.where(valid[:-k], f[:-k] + kk, NONE))
        d[:-k] = np.minimum(d[:-k], np.where(valid[k:], f[k:] + kk, NONE))
    return d


def _edt_host(m3, invert):
    return np.stack([_edt_host_image((m == 0) if invert else (m != 0)) for m in m3]).astype(np.int32)


def distance_transform_sq_host(mask, invert=False):
    """numpy restatement of distance_transform_sq: host array or tensor, [h, w] or [n, h, w], bool or uint8 -> int32 array of that shape."""
    m3, batched = _as_batch(mask)
    d2 = _edt_host(_to_host(m3), invert)
    return d2 if batched else d2[0]


def ordered_sum(e):
    """float64 [m] -> the sum in the order runet_edt_stats documents (chunks of 1024, strided adds, fold by halves, lanes over chunk sums)"""
    e = np.asarray(e, dtype=np.float64).reshape(-1)
    nblk = max(1, -(-e.size // 1024))
    c = np.zeros(nblk * 1024)
    c[:e.size] = e
    c = c.reshape(nblk, 4, 256)
    a = (((c[:, 0] + c[:, 1]) + c[:, 2]) + c[:, 3]).reshape(nblk, 4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        a = a[..., :o] + a[..., o:2 * o]
    chunk = ((a[:, 0, 0] + a[:, 1, 0]) + a[:, 2, 0]) + a[:, 3, 0]
    rows = np.zeros(-(-nblk // 64) * 64)
    rows[:nblk] = chunk
    acc = np.zeros(64)
    for r in rows.reshape(-1, 64):
        acc = acc + r
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc[:o] + acc[o:2 * o]
    return float(acc[0])


def _stats_host(d2, select, tol_sq):
    n = d2.shape[0]
    counts = np.zeros((n, 4 + len(tol_sq)), dtype=np.int64)
    sums = np.zeros(n, dtype=np.float64)
    for i in range(n):
        v = d2[i].reshape(-1).astype(np.int64)
        sel = np.ones(v.shape, bool) if select is None else select[i].reshape(-1) != 0
        live = sel & (v != NONE)
        lv = v[live]
        counts[i, :4] = (sel.sum(), (sel & ~live).sum(), lv.max() if lv.size else 0, lv.sum())
        counts[i, 4:] = [(lv <= t).sum() for t in tol_sq]
        sums[i] = ordered_sum(np.where(live, np.sqrt(v.astype(np.float64)), 0.0))
    return counts, sums


# ------------------------------------------------------------------------------------------------ the device route
def _workspace(n, h, w, device):
    from ._lib import lib
    need = lib.runet_edt_workspace_bytes(n, h, w)
    if need < 0:
        raise ValueError(f"a batch of {n} images of {h} x {w} is more than one call takes")
    return torch.empty(need, device=device, dtype=torch.uint8)


def _edt_device(t3, invert):
    """device uint8 [n, h, w] (rows may be strided) -> device int32 [n, h, w]"""
    from . import ops
    from ._lib import check, lib
    n, h, w = t3.shape
    rs = t3.stride(1) if h > 1 else w
    dense_rows = (w == 1 or t3.stride(2) == 1) and rs >= w
    if not dense_rows or (n > 1 and t3.stride(0) < (h - 1) * rs + w):
        t3 = t3.contiguous()                             # the strides say something row_stride / image_stride cannot
        rs = w
    d2 = torch.empty((n, h, w), device=t3.device, dtype=torch.int32)
    ws = _workspace(n, h, w, t3.device)
    check(lib.runet_edt_sq_u8(t3.data_ptr(), n, h, w, rs, t3.stride(0) if n > 1 else h * rs, int(bool(invert)), d2.data_ptr(), ws.data_ptr(),
                              ws.numel(), ops.stream()))
    return d2


def _stats_device(d2, select, tol_sq):
    from . import ops
    from ._lib import check, lib
    n, h, w = d2.shape
    counts = torch.empty((n, 4 + len(tol_sq)), device=d2.device, dtype=torch.int64)
    sums = torch.empty(n, device=d2.device, dtype=torch.float64)
    ws = _workspace(n, h, w, d2.device)
    tol = (C.c_int * max(1, len(tol_sq)))(*tol_sq)
    if select is not None:
        select = select.contiguous()
    check(lib.runet_edt_stats(d2.data_ptr(), None if select is None else select.data_ptr(), n, h, w, tol, len(tol_sq), counts.data_ptr(),
                              sums.data_ptr(), ws.data_ptr(), ws.numel(), ops.stream()))
    return counts.cpu().numpy(), sums.cpu().numpy()


def _edt(m3, invert):
    return _edt_device(m3, invert) if isinstance(m3, torch.Tensor) else _edt_host(m3, invert)


def _stats(d2, select, tol_sq):
    """-> (counts int64 [n, 4 + len(tol_sq)], sums float64 [n]) on the host"""
    return _stats_device(d2, select, tol_sq) if isinstance(d2, torch.Tensor) else _stats_host(d2, select, tol_sq)


def distance_transform_sq(mask, invert=False, as_tensor=False, device="cuda"):
    """Exact squared Euclidean distance to the nearest feature pixel.  mask: host array or device tensor, [h, w] or [n, h, w], bool or
    uint8; a feature is a non-zero byte, with invert a zero byte.  A device tensor whose rows are strided (a crop of a larger mask) is
    read in place.  -> int32 of the mask's shape (numpy, or a tensor with as_tensor): 0 on a feature, NONE = 2^31 - 1 everywhere in an
    image without one.  Every image of a batch is transformed on its own."""
    m3, batched = _as_batch(mask)
    d2 = _edt(_place(m3, device), invert)
    if not batched:
        d2 = d2[0]
    if as_tensor:
        return d2 if isinstance(d2, torch.Tensor) else torch.from_numpy(d2)
    return _to_host(d2)


# ------------------------------------------------------------------------------------------------ scores
def _check_tolerance(t):
    if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, np.integer)) or not 0 <= int(t) <= 46340:
        raise ValueError(f"a tolerance is a whole number of pixels in 0..46340, so that d <= t is d2 <= t^2 exactly (got {t!r})")
    return int(t)


def _check_tolerances(tolerances):
    tol = [_check_tolerance(t) for t in tolerances]
    if len(tol) > MAX_TOL:
        raise ValueError(f"at most {MAX_TOL} tolerances per call (got {len(tol)})")
    return tol


def _direction(row, s, tol, pixel_size):
    """one direction's figures from its counts row and distance sum"""
    count, unreachable = int(row[0]), int(row[1])
    reach = count - unreachable
    within_counts = [int(v) for v in row[4:]]
    if count == 0:                                       # nothing to measure from
        mean = rms = worst = NAN
    elif reach == 0:                                     # nothing to measure to
        mean = rms = worst = math.inf
    else:
        mean = float(s) / reach * pixel_size
        rms = math.sqrt(int(row[3]) / reach) * pixel_size
        worst = math.sqrt(int(row[2])) * pixel_size
    within = {t: {"count": c, "fraction": c / count if count else NAN} for t, c in zip(tol, within_counts)}
    return {"count": count, "unreachable": unreachable, "mean": mean, "rms": rms, "max": worst, "within": within}


def _deviation_batch(p3, t3, tol, pixel_size):
    n = p3.shape[0]
    both, other = _cat([p3, t3]), _cat([t3, p3])
    counts, sums = _stats(_edt(other, False), both, [t * t for t in tol])
    out = []
    for i in range(n):
        a = _direction(counts[i], sums[i], tol, pixel_size)
        b = _direction(counts[n + i], sums[n + i], tol, pixel_size)
        worst = [v for v in (a["max"], b["max"]) if not math.isnan(v)]
        reach = (a["count"] - a["unreachable"]) + (b["count"] - b["unreachable"])
        if a["unreachable"] or b["unreachable"]:
            assd = math.inf
        elif reach == 0:
            assd = NAN
        else:
            assd = (float(sums[i]) + float(sums[n + i])) / reach * pixel_size
        out.append({"pred_to_true": a, "true_to_pred": b, "hausdorff": max(worst) if worst else NAN, "assd": assd,
                    "tolerances": tuple(tol), "pixel_size": pixel_size})
    return out


def coastline_deviation(pred_coast, true_coast, tolerances=(1, 2, 5), pixel_size=1.0, device="cuda"):
    """How far two coastlines lie apart.  pred_coast, true_coast: binary coastline masks of one shape ([h, w], or [n, h, w]: a list of
    results, one per image), host arrays or device tensors, bool or uint8, non-zero = coastline.
    -> {"pred_to_true": D, "true_to_pred": D, "hausdorff", "assd", "tolerances", "pixel_size"} with
       D = {"count": own coastline pixels, "unreachable": those with no opposite pixel to measure to, "mean", "rms", "max": of the distance
            from each own pixel to the nearest opposite pixel, "within": {t: {"count", "fraction"}} the own pixels at most t pixels away}.
    hausdorff = the larger max; assd = the sum of both distance sums over the sum of both counts.  Tolerances are whole pixels (d <= t is
    d2 <= t^2, an integer test).  rms comes from the exact integer sum of d2, the mean from the float64 sum of the roots in the device's
    fixed order; all ratios are host float64.  An empty opposite set gives inf distances and within 0; an empty own set gives count 0 and
    NaN.  Lengths are multiplied by pixel_size at the very end."""
    tol = _check_tolerances(tolerances)
    pixel_size = float(pixel_size)
    p3, t3, batched = _pair(pred_coast, true_coast, "the two coastline masks")
    out = _deviation_batch(_place(p3, device), _place(t3, device), tol, pixel_size)
    return out if batched else out[0]


def _ratio(num, den):
    """a share of a pixel set; of an empty set 1.0, as train_water_segmentation.py:355 scores an empty union"""
    return 1.0 if den == 0 else num / den


def _boundary_batch(p3, g3, tol):
    n = p3.shape[0]
    regions = _cat([p3, g3])
    inside = regions != 0
    d2c = _edt(regions, True)                            # to the complement inside the image
    edge = _u8(inside & (d2c <= 1))                      # inner boundaries
    band = inside & (d2c <= tol * tol)                   # M_d
    inter = _to_host((band[:n] & band[n:]).sum((1, 2)))
    union = _to_host((band[:n] | band[n:]).sum((1, 2)))
    counts, _ = _stats(_edt(_cat([edge[n:], edge[:n]]), False), edge, [tol * tol])
    out = []
    for i in range(n):
        n_p, n_g = int(counts[i][0]), int(counts[n + i][0])
        precision, recall = _ratio(int(counts[i][4]), n_p), _ratio(int(counts[n + i][4]), n_g)
        out.append({"boundary_precision": precision, "boundary_recall": recall,
                    "bf1": 2 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0,
                    "boundary_iou": _ratio(int(inter[i]), int(union[i])), "pred_boundary_pixels": n_p, "true_boundary_pixels": n_g,
                    "tolerance": tol})
    return out


def boundary_scores(pred_mask, true_mask, tolerance=2, device="cuda"):
    """Boundary F-score and Boundary IoU of two region masks of one shape ([h, w], or [n, h, w]: a list of results, one per image),
    non-zero = inside.  The boundary of a mask M is its inner boundary, M and {distance to the complement of M inside the image <= 1}.
      boundary_precision = the share of predicted boundary pixels within `tolerance` pixels of the true boundary,
      boundary_recall    = the converse, bf1 = their harmonic mean (0.0 where both are 0),
      boundary_iou       = |P_d and G_d| / |P_d or G_d|, M_d = M and {distance to the complement of M inside the image <= tolerance}.
    A share of an empty set is 1.0.  The frame is NOT background: a region that runs off the tile has no boundary along the tile edge,
    because a tile edge is not a coast.  The published Boundary IoU code pads the masks with zeros and so counts that edge; pad the inputs
    with a ring of zeros to get its figures.  Counts are integers from the device, ratios host float64."""
    tol = _check_tolerance(tolerance)
    p3, g3, batched = _pair(pred_mask, true_mask, "the two region masks")
    out = _boundary_batch(_place(p3, device), _place(g3, device), tol)
    return out if batched else out[0]


def evaluate_coastline(result, true_water_mask, tolerances=(1, 2, 5), boundary_tolerance=2, pixel_size=1.0, device="cuda"):
    """Scores of one CoastlineExtractor result (extract_coastline_from_image) against the true water mask of the same image: the true
    coastline band is made from the true mask by the same runet_dilate_diff_u8 and dilation_size that made the predicted band.  Masks that
    the result holds as device tensors are used where they are.
    -> {"deviation": coastline_deviation(predicted band, true band), "boundary": boundary_scores(predicted water, true water),
        "dilation_size"}."""
    from .predict import dilate_diff
    k = int(result.get("dilation_size", 5))
    pred_water, pred_coast = _as_u8(result["water_mask"]), _as_u8(result["coastline_mask"])
    truth = _as_u8(true_water_mask)
    if truth.ndim != 2 or tuple(truth.shape) != tuple(pred_water.shape) or tuple(pred_coast.shape) != tuple(pred_water.shape):
        raise ValueError(f"the true water mask must have the result's shape {tuple(pred_water.shape)} (got {tuple(truth.shape)})")
    truth = _u8(_to_device(truth, device) != 0).contiguous()
    true_coast, _, _ = dilate_diff(truth, k)
    return {"deviation": coastline_deviation(pred_coast, true_coast, tolerances, pixel_size, device),
            "boundary": boundary_scores(pred_water, truth, boundary_tolerance, device), "dilation_size": k}
