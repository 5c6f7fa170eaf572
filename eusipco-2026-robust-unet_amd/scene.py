"""Scene ingestion on the device: the step in front of every pipeline of the reference (tif_to_image.py:42-171,
train_water_segmentation.py:103-174, predict_coastline.py:425-581) - from a multi-band satellite raster to the uint8 RGB image the models
were trained on.

  1. pick the band triple                      select_bands            (host)
  2. np.percentile(band, [2, 98]) per band     band_percentiles        runet_band_percentiles: exact radix select + numpy's _lerp, float64
  3. stretch to 0..255 in float64, darken      enhance_scene           runet_band_stretch_u8: the reference's expression per pixel, true
     the low end of channel 0, cast to uint8                           division, no contraction, the cast's detour through the input dtype

The raw bands are uploaded once (or already live on the device); percentiles stay on the device and feed the stretch directly, so with
`as_tensor=True` nothing synchronises and the image goes straight into `predict.scene_to_tiles`.

Modes: "water" = enhance_image_for_water / enhance_image(enhance_water=True), "rgb" = enhance_image(enhance_water=False), "display" =
normalize_image_for_display.  A constant band in "water" / "rgb" is undefined in the reference (0 / 0 cast to an integer); here NaN -> 0,
+inf -> 255, -inf -> 0 (include/runet_hip.h).  GDAL is not a dependency: a .tif path is read through osgeo.gdal only if it imports.
"""
from __future__ import annotations

import json
import math
import os
from datetime import datetime

import numpy as np
import torch

from . import ops
from ._lib import check, lib

MODES = {"water": 0, "rgb": 1, "display": 2}
MAX_BANDS = 6                                    # the reference reads at most six bands
U8, U16, I16, F32 = 0, 1, 2, 3                   # RUNET_BAND_*
_NP_CODES = {np.dtype(np.uint8): U8, np.dtype(np.uint16): U16, np.dtype(np.int16): I16, np.dtype(np.float32): F32}
_TORCH_CODES = {torch.uint8: U8, torch.int16: I16, torch.float32: F32}
if hasattr(torch, "uint16"):
    _TORCH_CODES[torch.uint16] = U16
# the reference's metadata strings (tif_to_image.py:86-98), part of the file format it writes
_ENHANCEMENT = {"nir": "NIR-Red-Green (水体增强)", "rgb": "标准RGB", "gray": "灰度"}


def select_bands(n_bands, mode="water"):
    """-> the three band indices of `mode` for a raster of n_bands bands (only the first six count).  "water": NIR-Red-Green (4, 3, 2) from
    five bands on; exactly four bands fall back to (2, 1, 0), the reference's IndexError branch; three bands are (2, 1, 0); fewer are grey."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)} (got {mode!r})")
    n = min(int(n_bands), MAX_BANDS)
    if n < 1:
        raise ValueError("a raster needs at least one band")
    if n < 3:
        return (0, 0, 0)
    if mode == "display":
        return (0, 1, 2)
    if mode == "water" and n >= 5:
        return (4, 3, 2)
    return (2, 1, 0)


def percentile_ranks(n, q=(2, 98)):
    """numpy's "linear" rule for np.percentile(a, q) of n values -> [(k, gamma), ...]: the result is lerp(sorted[k], sorted[min(k + 1, n - 1)],
    gamma) with quantile = q / 100, vi = (n - 1) * quantile, k = floor(vi), gamma = vi - k, all in float64 as numpy evaluates them."""
    n = int(n)
    if n < 1:
        raise ValueError("no values")
    out = []
    for p in q:
        if not 0 <= p <= 100:
            raise ValueError("percentiles must lie in 0..100")
        vi = np.float64(n - 1) * (np.float64(p) / np.float64(100))
        prev = np.floor(vi)
        k, g = int(prev), float(vi - prev)
        if k >= n - 1:
            k, g = n - 1, 0.0
        out.append((k, g))
    return out


class _Raster:
    """device planes + the arguments every entry point takes for them"""

    def __init__(self, t, code, meta=None):
        if t.dim() == 2:
            t = t.unsqueeze(0)
        if t.dim() != 3 or min(t.shape) < 1:
            raise ValueError("bands must be a non-empty [B, H, W] or [H, W] raster")
        sb, sr, se = t.stride()
        b, h, w = t.shape
        if se < 1 or sr < (w - 1) * se + 1 or (b > 1 and sb < (h - 1) * sr + (w - 1) * se + 1):
            t = t.contiguous()                   # transposed / overlapping views: the kernels take positive strides that cover the extent
            sb, sr, se = t.stride()
        if h * w >= 2 ** 31:
            raise ValueError("h * w must be below 2^31")
        self.t, self.code, self.meta = t, code, meta or {}
        self.n_bands, self.h, self.w = b, h, w
        self.args = (t.data_ptr(), code, b, h, w, sb, sr, se)


def _open_tif(path):
    try:
        from osgeo import gdal
    except ImportError as e:
        raise ImportError(f"reading {path!r} needs GDAL (osgeo.gdal), which is not installed and is not a dependency of this package; "
                          "read the bands yourself and pass the [B, H, W] array or a .npy file") from e
    ds = gdal.Open(path)
    if ds is None:
        raise ValueError(f"GDAL cannot open {path!r}")
    a = np.array([ds.GetRasterBand(i).ReadAsArray() for i in range(1, min(ds.RasterCount + 1, MAX_BANDS + 1))])
    meta = {"bands_count": ds.RasterCount, "geo_transform": ds.GetGeoTransform() if ds.GetGeoTransform() else None,
            "projection": ds.GetProjection() if ds.GetProjection() else None}
    return a, meta


def load_raster(bands, device="cuda"):
    """numpy array, device tensor, .npy path or (with GDAL) .tif path -> _Raster on `device`; uint8, uint16, int16 or float32."""
    if isinstance(bands, _Raster):
        return bands
    meta = {}
    if isinstance(bands, (str, os.PathLike)):
        path = os.fspath(bands)
        ext = os.path.splitext(path)[1].lower()
        if ext in (".tif", ".tiff"):
            bands, meta = _open_tif(path)
        elif ext == ".npy":
            bands = np.load(path, allow_pickle=False)
        else:
            raise ValueError(f"{path!r}: band rasters are read from .npy (or, with GDAL, .tif / .tiff) files")
        meta["path"] = path
    if isinstance(bands, torch.Tensor):
        if bands.dtype not in _TORCH_CODES:
            raise ValueError(f"bands must be uint8, uint16, int16 or float32 (got {bands.dtype})")
        return _Raster(bands.to(device), _TORCH_CODES[bands.dtype], meta)
    a = np.asarray(bands)
    if a.dtype not in _NP_CODES:
        raise ValueError(f"bands must be uint8, uint16, int16 or float32 (got {a.dtype})")
    code = _NP_CODES[a.dtype]
    a = np.ascontiguousarray(a)
    if code == U16:
        a = a.view(np.int16)                     # the same bytes: uint16 tensors are not everywhere; the dtype code travels separately
    return _Raster(torch.from_numpy(a).to(device), code, meta)


def _percentiles(r, sel, q=(2, 98), wide_diff=False):
    """-> (device float64 [len(sel), 2], device int32 [1] count of non-finite values); no synchronisation"""
    n_sel = len(sel)
    dev = r.t.device
    (k_lo, g_lo), (k_hi, g_hi) = percentile_ranks(r.h * r.w, q)
    if k_lo > k_hi:
        raise ValueError("q must be ascending")
    pct = torch.empty((n_sel, 2), device=dev, dtype=torch.float64)
    nonfinite = torch.empty(1, device=dev, dtype=torch.int32)
    ws = torch.empty(lib.runet_band_percentiles_workspace(n_sel), device=dev, dtype=torch.uint8)
    s = tuple(sel) + (0,) * (3 - n_sel)
    check(lib.runet_band_percentiles(*r.args, s[0], s[1], s[2], n_sel, k_lo, g_lo, k_hi, g_hi, int(bool(wide_diff)), pct.data_ptr(),
                                     nonfinite.data_ptr(), ws.data_ptr(), ws.numel(), ops.stream()))
    return pct, nonfinite


def band_percentiles(bands, sel, q=(2, 98), as_float64=False, device="cuda"):
    """np.percentile(bands[i], q) for i in sel (1..3 bands) -> device float64 [len(sel), 2], bit for bit.  as_float64: np.percentile of
    bands[i].astype(np.float64), which differs in the last bit for float32 (and for int16 ranges that wrap): the "display" mode's order."""
    sel = tuple(int(i) for i in sel)
    if not 1 <= len(sel) <= 3:
        raise ValueError("1..3 selected bands")
    return _percentiles(load_raster(bands, device), sel, q, as_float64)[0]


def _enhance(r, mode, out=None):
    """-> (device uint8 [H, W, 3], device int32 [1] non-finite count)"""
    sel = select_bands(r.n_bands, mode)
    if len(set(sel)) == 1:                       # grey: one selection, three copies
        pct, nonfinite = _percentiles(r, sel[:1], wide_diff=mode == "display")
        pct = pct.expand(3, 2).contiguous()
    else:
        pct, nonfinite = _percentiles(r, sel, wide_diff=mode == "display")
    if out is None:
        out = torch.empty((r.h, r.w, 3), device=r.t.device, dtype=torch.uint8)
    check(lib.runet_band_stretch_u8(*r.args, sel[0], sel[1], sel[2], pct.data_ptr(), MODES[mode], out.data_ptr(), out.stride(0), ops.stream()))
    return out, nonfinite


def enhance_scene(bands, mode="water", as_tensor=False, device="cuda"):
    """The reference's enhanced uint8 [H, W, 3] image of a [B, H, W] / [H, W] raster.  as_tensor=True: a device tensor, nothing synchronises
    (non-finite float32 values are then the caller's to rule out).  Otherwise a numpy array, and ValueError if the bands hold NaN or inf."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)} (got {mode!r})")
    r = load_raster(bands, device)
    out, nonfinite = _enhance(r, mode)
    if as_tensor:
        return out
    if int(nonfinite.item()):
        raise ValueError(f"the selected bands hold {int(nonfinite.item())} non-finite values: mask them (nodata) before the stretch")
    return out.cpu().numpy()


def convert_scene(bands, out_png, meta_json=None, enhance_water=True, device="cuda"):
    """tif_to_image.py:42-133 for one raster: the enhanced PNG and, if meta_json is given, the reference's metadata document.  The geo keys
    are None unless GDAL supplied them.  -> (out_png, metadata)"""
    from PIL import Image
    r = load_raster(bands, device)
    mode = "water" if enhance_water else "rgb"
    img = enhance_scene(r, mode)
    os.makedirs(os.path.dirname(os.path.abspath(out_png)), exist_ok=True)
    Image.fromarray(img).save(out_png, "PNG")
    sel = select_bands(r.n_bands, mode)
    kind = "gray" if r.n_bands < 3 else "nir" if sel == (4, 3, 2) else "rgb"
    meta = {"original_file": r.meta.get("path"), "png_file": os.fspath(out_png), "image_size": [r.w, r.h],
            "bands_count": r.meta.get("bands_count", r.n_bands), "enhancement_type": _ENHANCEMENT[kind],
            "conversion_time": str(datetime.now()), "geo_transform": r.meta.get("geo_transform"), "projection": r.meta.get("projection")}
    if meta_json:
        os.makedirs(os.path.dirname(os.path.abspath(meta_json)), exist_ok=True)
        with open(meta_json, "w", encoding="utf-8") as fh:
            json.dump(meta, fh, indent=2, ensure_ascii=False)
    return out_png, meta
