"""Regions of a water mask: connected-component labelling on the device, the table of water bodies, and the area filter that removes
specks of water and fills holes of land before the coastline is traced (csrc/ccl.hip; the rules are stated in include/runet_hip.h).

The reference traces coastlines on `dilated - water` and keeps every contour of more than 10 points (predict_coastline.py:583-618), so each
pond, shadow, boat or wrong pixel of the thresholded prediction (Main_Final.py:521) becomes a "coastline".  Everyone who uses such a
pipeline labels the mask and filters by area in front of that step; scipy.ndimage.label needs the mask on the host and seconds for a scene.

  label_components        int32 labels: 0 off the features, else 1 + the smallest linear index y * w + x of the pixel's component
                                                                                                       runet_ccl_label_u8
  label_components_host   the same in numpy alone (runs per row, unions between adjacent rows by repeated minima), no scipy
  dense_labels            labels -> 1..K in ascending root order, which is scipy.ndimage.label's numbering
  water_bodies            per component: label, area, bounding box, which sides of the image it touches       + runet_ccl_areas, runet_ccl_table
  clean_water_mask        water components below min_water_area become land, then land components (dual connectivity) below min_land_area
                          become water; components that touch the image frame are exempt by default           + runet_ccl_filter_u8

Everything is an integer with an exact definition, and every merge on the device is an integer minimum, so the device and the numpy route
give the same bytes.  RUNET_NO_DEVICE_CCL=1 (read at every call) sends all of the above through the numpy restatement.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .boundary import _as_u8, _to_device, _to_host

MAX_SIDE = 32768
MAX_AREA = 2 ** 31 - 1
INFO_KEYS = ("removed_water_components", "removed_water_pixels", "filled_land_components", "filled_land_pixels")
SIDES = ("top", "bottom", "left", "right")               # frame bits 0..3


def _host_route():
    return os.environ.get("RUNET_NO_DEVICE_CCL", "") not in ("", "0")


def _check_connectivity(connectivity):
    if isinstance(connectivity, (bool, np.bool_)) or connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8 (got {connectivity!r})")
    return int(connectivity)


def _check_area(value, what):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or int(value) < 0:
        raise ValueError(f"{what} is a whole number of pixels >= 0 (got {value!r})")
    return min(int(value), MAX_AREA)


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
        raise ValueError(f"h and w must not exceed {MAX_SIDE}, so that every label fits int32 (got {h} x {w})")
    return m3, m.ndim == 3


# ------------------------------------------------------------------------------------------------ the numpy restatement
def _label_host_image(feat, connectivity):
    """bool [h, w] -> int32 [h, w].  The horizontal runs of every row, in row-major order, so that a run's number orders as its first
    pixel's index does; an edge between two runs of adjacent rows whose column ranges overlap (connectivity 8: or touch diagonally); then
    every run takes the smallest run number of its component: roots hook onto the smallest root they share an edge with, paths are
    halved until flat, until nothing moves."""
    h, w = feat.shape
    pad = np.zeros((h, w + 2), dtype=np.int8)
    pad[:, 1:-1] = feat
    d = np.diff(pad, axis=1)
    ry, rs = np.nonzero(d == 1)                          # run r covers the columns rs[r] .. re[r] - 1 of row ry[r]
    re = np.nonzero(d == -1)[1]
    out = np.zeros((h, w), dtype=np.int32)
    if ry.size == 0:
        return out
    reach = 1 if connectivity == 8 else 0
    k = w + 4
    start_key, end_key = ry * k + rs + 1, ry * k + re + 1
    lo = np.searchsorted(end_key, (ry - 1) * k + rs + 1 - reach, side="right")     # the runs of the row above that end after my start
    hi = np.searchsorted(start_key, (ry - 1) * k + re + 1 + reach, side="left")    # and start before my end
    cnt = np.maximum(hi - lo, 0)
    a = np.repeat(np.arange(ry.size), cnt)
    b = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(lo, cnt)
    parent = np.arange(ry.size)
    while True:
        pa, pb = parent[a], parent[b]
        live = pa != pb
        if not live.any():
            break
        a, b, pa, pb = a[live], b[live], pa[live], pb[live]
        np.minimum.at(parent, np.maximum(pa, pb), np.minimum(pa, pb))
        while True:
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt
    label = (ry * w + rs + 1)[parent]
    out[feat] = np.repeat(label, re - rs)
    return out


def _label_host(m3, invert, connectivity):
    return np.stack([_label_host_image((m == 0) if invert else (m != 0), connectivity) for m in m3])


def _areas_host(lab):
    """int32 [h, w] labels -> (roots' labels ascending, areas, x0, y0, x1, y1, frame) as int64 arrays"""
    h, w = lab.shape
    ys, xs = np.nonzero(lab)
    uniq, dense = np.unique(lab[ys, xs], return_inverse=True)
    k = uniq.size
    area = np.bincount(dense, minlength=k).astype(np.int64)
    x0, y0 = np.full(k, w, np.int64), np.full(k, h, np.int64)
    x1, y1 = np.full(k, -1, np.int64), np.full(k, -1, np.int64)
    np.minimum.at(x0, dense, xs)
    np.minimum.at(y0, dense, ys)
    np.maximum.at(x1, dense, xs)
    np.maximum.at(y1, dense, ys)
    frame = (y0 == 0) * 1 + (y1 == h - 1) * 2 + (x0 == 0) * 4 + (x1 == w - 1) * 8
    return uniq.astype(np.int64), area, x0, y0, x1, y1, frame


def _filter_host(out, lab, min_area, keep_frame, value):
    """one image: the components of lab with area < min_area (and, with keep_frame, no frame contact) take `value` in out -> (components, pixels)"""
    uniq, area, _, _, _, _, frame = _areas_host(lab)
    sel = area < min_area
    if keep_frame:
        sel &= frame == 0
    hit = np.isin(lab, uniq[sel]) & (lab != 0)
    out[hit] = value
    return int(sel.sum()), int(hit.sum())


def _clean_host(m3, min_water, min_land, connectivity, keep_frame):
    out = np.array(m3, dtype=np.uint8, copy=True)
    counts = np.zeros((out.shape[0], 4), dtype=np.int64)
    for i, m in enumerate(out):
        if min_water:
            counts[i, 0:2] = _filter_host(m, _label_host_image(m != 0, connectivity), min_water, keep_frame, 0)
        if min_land:
            counts[i, 2:4] = _filter_host(m, _label_host_image(m == 0, 12 - connectivity), min_land, keep_frame, 1)
    return out, counts


# ------------------------------------------------------------------------------------------------ the device route
def _workspace(n, h, w, device):
    from ._lib import lib
    need = lib.runet_ccl_workspace_bytes(n, h, w)
    if need < 0:
        raise ValueError(f"a batch of {n} images of {h} x {w} is more than one call takes")
    return torch.empty(need, device=device, dtype=torch.uint8)


def _label_device(t3, invert, connectivity, ws=None):
    """device uint8 [n, h, w] (rows may be strided) -> device int32 [n, h, w]"""
    from . import ops
    from ._lib import check, lib
    n, h, w = t3.shape
    rs = t3.stride(1) if h > 1 else w
    dense_rows = (w == 1 or t3.stride(2) == 1) and rs >= w
    if not dense_rows or (n > 1 and t3.stride(0) < (h - 1) * rs + w):
        t3 = t3.contiguous()                             # the strides say something row_stride / image_stride cannot
        rs = w
    labels = torch.empty((n, h, w), device=t3.device, dtype=torch.int32)
    if ws is None:
        ws = _workspace(n, h, w, t3.device)
    check(lib.runet_ccl_label_u8(t3.data_ptr(), n, h, w, rs, t3.stride(0) if n > 1 else h * rs, int(bool(invert)), connectivity,
                                 labels.data_ptr(), ws.data_ptr(), ws.numel(), ops.stream()))
    return labels


def _areas_device(labels):
    """-> (areas int32 [n, h, w], frame uint8 [n, h, w]) on the device"""
    from . import ops
    from ._lib import check, lib
    n, h, w = labels.shape
    areas = torch.empty((n, h, w), device=labels.device, dtype=torch.int32)
    frame = torch.empty((n, h, w), device=labels.device, dtype=torch.uint8)
    check(lib.runet_ccl_areas(labels.data_ptr(), n, h, w, areas.data_ptr(), frame.data_ptr(), ops.stream()))
    return areas, frame


def _filter_device(labels, areas, frame, min_area, keep_frame, value, out, counts):
    """out: dense device uint8 [n, h, w], changed in place; counts: device int64 [n, 2], written whole"""
    from . import ops
    from ._lib import check, lib
    n, h, w = labels.shape
    check(lib.runet_ccl_filter_u8(labels.data_ptr(), areas.data_ptr(), frame.data_ptr(), n, h, w, min_area, int(bool(keep_frame)), value,
                                  out.data_ptr(), counts.data_ptr(), ops.stream()))


def _table_device(labels, areas, frame, capacity, ws):
    """-> (n_components int64 [n], table int32 [n, capacity, 8] or None) on the device"""
    from . import ops
    from ._lib import check, lib
    n, h, w = labels.shape
    count = torch.empty(n, device=labels.device, dtype=torch.int64)
    table = torch.empty((n, capacity, 8), device=labels.device, dtype=torch.int32) if capacity else None
    check(lib.runet_ccl_table(labels.data_ptr(), areas.data_ptr(), frame.data_ptr(), n, h, w, capacity, count.data_ptr(),
                              None if table is None else table.data_ptr(), ws.data_ptr(), ws.numel(), ops.stream()))
    return count, table


def _clean_device(mask3, min_water, min_land, connectivity, keep_frame, counts):
    """mask3: dense device uint8 [n, h, w], cleaned in place.  counts: device int64 [n, 4] (contiguous), one row per image in INFO_KEYS'
    order; the pair of a skipped step is cleared.  No host synchronisation."""
    n, h, w = mask3.shape
    ws = _workspace(n, h, w, mask3.device)
    pair = torch.empty((n, 2), device=mask3.device, dtype=torch.int64) if n > 1 else None
    for at, threshold, conn, invert, value in ((0, min_water, connectivity, False, 0), (2, min_land, 12 - connectivity, True, 1)):
        if not threshold:
            counts[:, at:at + 2].zero_()
            continue
        labels = _label_device(mask3, invert, conn, ws)
        areas, frame = _areas_device(labels)
        if n == 1:                                       # a row of counts is the call's [1][2] block where it lies
            _filter_device(labels, areas, frame, threshold, keep_frame, value, mask3, counts[0, at:at + 2])
        else:
            _filter_device(labels, areas, frame, threshold, keep_frame, value, mask3, pair)
            counts[:, at:at + 2].copy_(pair)


# ------------------------------------------------------------------------------------------------ the public surface
def label_components_host(mask, connectivity=8, invert=False):
    """numpy restatement of label_components: host array or tensor, [h, w] or [n, h, w], bool or uint8 -> int32 array of that shape."""
    connectivity = _check_connectivity(connectivity)
    m3, batched = _as_batch(mask)
    labels = _label_host(_to_host(m3), invert, connectivity)
    return labels if batched else labels[0]


def label_components(mask, connectivity=8, invert=False, as_tensor=False, device="cuda"):
    """Connected components of a mask.  mask: host array or device tensor, [h, w] or [n, h, w], bool or uint8; a feature is a non-zero
    byte, with invert a zero byte.  connectivity 4 or 8; only pixels inside the image connect, and the images of a batch are independent.
    A device tensor whose rows are strided (a crop of a larger mask) is read in place.
    -> int32 of the mask's shape (numpy, or a tensor with as_tensor): 0 off the features, otherwise 1 + the smallest linear index y * w + x
    among the pixels of the component, indices per image."""
    connectivity = _check_connectivity(connectivity)
    m3, batched = _as_batch(mask)
    if _host_route():
        labels = _label_host(_to_host(m3), invert, connectivity)
    else:
        labels = _label_device(_to_device(m3, device), invert, connectivity)
    if not batched:
        labels = labels[0]
    if as_tensor:
        return labels if isinstance(labels, torch.Tensor) else torch.from_numpy(labels)
    return _to_host(labels)


def dense_labels(labels):
    """labels as label_components returns them ([h, w], or [n, h, w]: every image on its own) -> int32 of that shape with the components
    numbered 1..K in ascending root order, i.e. in the order in which a row-major scan first meets them: scipy.ndimage.label's numbering,
    for either structure."""
    lab = _to_host(labels)
    if lab.ndim == 3:
        return np.stack([dense_labels(one) for one in lab]) if lab.shape[0] else lab.astype(np.int32)
    if lab.ndim != 2:
        raise ValueError(f"expected [h, w] or [n, h, w] labels (got shape {tuple(lab.shape)})")
    roots = np.unique(lab[lab != 0])
    return np.where(lab != 0, np.searchsorted(roots, lab) + 1, 0).astype(np.int32)


def _bodies(rows, pixel_size):
    """table rows {label, area, x0, y0, x1, y1, frame, 0} -> the list water_bodies returns for one image"""
    unit = float(pixel_size) * float(pixel_size)
    return [{"label": int(r[0]), "area": int(r[1]), "area_units": int(r[1]) * unit, "bbox": (int(r[2]), int(r[3]), int(r[4]), int(r[5])),
             "touches_frame": {side: bool(int(r[6]) >> bit & 1) for bit, side in enumerate(SIDES)}} for r in rows]


def water_bodies(mask, connectivity=8, pixel_size=1.0, device="cuda"):
    """The components of a water mask ([h, w], or [n, h, w]: a list of results, one per image) as a list in ascending label:
    {"label", "area" (pixels), "area_units" (area * pixel_size^2), "bbox": (x0, y0, x1, y1) inclusive, "touches_frame": {"top", "bottom",
    "left", "right"}}.  On the device: labels, areas, a count (the one synchronisation), then a table of exactly that capacity, downloaded."""
    connectivity = _check_connectivity(connectivity)
    m3, batched = _as_batch(mask)
    if _host_route():
        out = [_bodies(np.stack(_areas_host(lab), axis=1), pixel_size) for lab in _label_host(_to_host(m3), False, connectivity)]
    else:
        t3 = _to_device(m3, device)
        n, h, w = t3.shape
        ws = _workspace(n, h, w, t3.device)
        labels = _label_device(t3, False, connectivity, ws)
        areas, frame = _areas_device(labels)
        count, _ = _table_device(labels, areas, frame, 0, ws)
        count = count.cpu().numpy()
        capacity = int(count.max())
        if capacity > MAX_AREA:
            raise ValueError(f"{capacity} components are more than one table takes")
        table = _table_device(labels, areas, frame, capacity, ws)[1].cpu().numpy() if capacity else np.zeros((n, 0, 8), np.int32)
        out = [_bodies(table[i, :int(count[i])], pixel_size) for i in range(n)]
    return out if batched else out[0]


def _info(row):
    return {k: int(v) for k, v in zip(INFO_KEYS, row)}


def clean_water_mask(mask, min_water_area=0, min_land_area=0, connectivity=8, keep_frame=True, as_tensor=False, device="cuda"):
    """Area filter of a water mask ([h, w] or [n, h, w], bool or uint8, non-zero = water; host array or device tensor).
      step 1: the water components under `connectivity` with area < min_water_area become land (byte 0);
      step 2: on that result, the land components under the dual connectivity (8 <-> 4) with area < min_land_area become water (byte 1).
    The dual connectivity is what makes a hole of the one a component of the other: water that touches only diagonally is one body under 8
    and must not also be bridged by the land between.  With keep_frame a component that touches the image frame is exempt from both steps:
    its true area is unknown, and the frame is neither water nor land (boundary.py).  A threshold of 0 skips its step, with no launch; the
    thresholds are whole numbers >= 0 (ValueError otherwise).  The correspondence to skimage: remove_small_objects(mask, min_water_area,
    connectivity = 1 for 4, 2 for 8) then remove_small_holes(., min_land_area) with the dual connectivity, where nothing touches the frame
    or keep_frame is off.
    -> (mask01, info): the mask's bytes as uint8 of its shape with those changes (numpy, or a tensor with as_tensor; always a new array),
    info = {"removed_water_components", "removed_water_pixels", "filled_land_components", "filled_land_pixels"}, ints for one image, a tuple
    of such dicts for a batch."""
    connectivity = _check_connectivity(connectivity)
    min_water, min_land = _check_area(min_water_area, "min_water_area"), _check_area(min_land_area, "min_land_area")
    m3, batched = _as_batch(mask)
    n = m3.shape[0]
    if not (min_water or min_land):
        out = m3.clone() if isinstance(m3, torch.Tensor) else np.array(m3, copy=True)
        counts = np.zeros((n, 4), dtype=np.int64)
    elif _host_route():
        out, counts = _clean_host(_to_host(m3), min_water, min_land, connectivity, bool(keep_frame))
    else:
        src = _to_device(m3, device)
        out = src.contiguous()
        if out.data_ptr() == src.data_ptr() and isinstance(m3, torch.Tensor):
            out = out.clone()                            # never the caller's own memory
        counts = torch.empty((n, 4), device=out.device, dtype=torch.int64)
        _clean_device(out, min_water, min_land, connectivity, bool(keep_frame), counts)
        counts = counts.cpu().numpy()
    info = tuple(_info(r) for r in counts)
    if not batched:
        out, info = out[0], info[0]
    if as_tensor:
        return (out if isinstance(out, torch.Tensor) else torch.from_numpy(out)), info
    return _to_host(out), info
