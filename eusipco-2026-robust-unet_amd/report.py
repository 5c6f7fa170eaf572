"""The reference's two report figures: the analysis report of one extraction, `<base>_coastsat_analysis.png`
(predict_coastline.py:659-846), and the error maps of the model comparison, `error_maps_comparison.png`
(Extended_Baseline_Comparison.py:863-977).

Everything the figures show is an array the reference computes per pixel on the host in numpy.  Here the arrays come from the device
(csrc/report.hip; the rules are stated in include/runet_hip.h) and equal numpy's bit for bit, and matplotlib only draws them:

  combined_overlay     :708-730   water tint and coastline on the display image         runet_report_overlay_u8
  ndwi_histograms      :789-813   np.histogram(density=True) of NDWI, water / rest      runet_ndwi_stats, runet_ndwi_hist; edges on the host
  rgb_histograms       :821-829   the fallback below four bands                         runet_rgb_hist_u8; folded into bins on the host
  coastline_lengths    :763-770   open polyline lengths                                 host, float64
  analysis_report                 the arrays of one report, from a result dict
  error_overlays       Extended_Baseline_Comparison.py:882-959   denormalised image, TP / FP / FN / TN overlay, |prob - mask|, counts, error sum
                                                                                        runet_error_overlays
  error_map_arrays                the arrays of the error-map figure for a dict of models and a validation loader
  create_coastsat_style_visualization, generate_error_maps      the two figures (matplotlib, imported inside the drawing functions only)

Inputs are numpy arrays or device tensors (a uint8 device view that does not start on a 4-byte address is copied once: the overlay and
RGB kernels read whole dwords).  as_tensor=True returns device tensors and does not synchronise, except ndwi_histograms: the
edges of np.histogram depend on the data's minimum and maximum, so its eight statistics words are downloaded between its two passes.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import data, ops, scene as _scene
from ._lib import check, lib
from .predict import _dev_u8, _raise_nonfinite, resize_nearest

MAX_BINS = 256
WATER_TINT = (0, 100, 200)                               # predict_coastline.py:723
CLASS_COLOURS = ((0.2, 0.8, 0.2), (0.9, 0.2, 0.2), (0.2, 0.2, 0.9), (0.9, 0.9, 0.9), (0.0, 0.0, 0.0))   # TP FP FN TN, no class
CLASS_NAMES = ("tp", "fp", "fn", "tn", "none")
OURS = "Robust U-Net (Ours)"                             # Extended_Baseline_Comparison.py:947


def _check_bins(bins):
    bins = int(bins)
    if not 2 <= bins <= MAX_BINS:
        raise ValueError(f"bins must lie in 2..{MAX_BINS} (got {bins})")
    return bins


# ------------------------------------------------------------------------------------------------ A. the scene report
def overlay_table():
    """-> uint8 [3, 256]: what `img[water] * 0.6 + np.array([0, 100, 200]) * 0.4` stores into a uint8 image for every byte value and channel:
    numpy's own float64 expression and its C cast (truncation)."""
    v = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    return np.ascontiguousarray((v * 0.6 + np.array(WATER_TINT) * 0.4).astype(np.uint8).T)


def _overlay(image, water, coast):
    """device tensors -> device uint8 [H, W, 3]; masks of another size go through resize_nearest first (:714-717)"""
    if image.dim() != 3 or image.shape[2] != 3 or water.dim() != 2 or coast.dim() != 2:
        raise ValueError("expected a [H, W, 3] image and two [h, w] masks")
    h, w, _ = image.shape
    water, coast = (resize_nearest(m, (h, w)) for m in (water, coast))
    image, water, coast = (t.clone() if t.data_ptr() % 4 else t for t in (image, water, coast))
    table = torch.from_numpy(overlay_table()).to(image.device)
    out = torch.empty_like(image)
    check(lib.runet_report_overlay_u8(image.data_ptr(), water.data_ptr(), coast.data_ptr(), h, w, table.data_ptr(), out.data_ptr(), ops.stream()))
    return out


def combined_overlay(display_rgb, water_mask, coastline_mask, as_tensor=False, device="cuda"):
    """predict_coastline.py:708-730 -> uint8 [H, W, 3]: where water == 1 every channel becomes uint8(v * 0.6 + (0, 100, 200)[c] * 0.4)
    (float64, truncated), then where coast == 1 the pixel is white.  Mask values other than 1 leave the pixel alone."""
    out = _overlay(_dev_u8(display_rgb, device), _dev_u8(water_mask, device), _dev_u8(coastline_mask, device))
    return out if as_tensor else out.cpu().numpy()


def histogram_edges(lo, hi, bins):
    """np.histogram's edges for data whose minimum and maximum are lo, hi (None, None: no data): linspace over (lo, hi), over
    (lo - 0.5, hi + 0.5) where they are equal, over (0, 1) without data."""
    if lo is None:
        lo, hi = 0, 1
    elif lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    return np.linspace(lo, hi, bins + 1, endpoint=True, dtype=np.float64)


def _density(counts, edges):
    """np.histogram(density=True): counts / diff(edges) / counts.sum(); NaN for a class without pixels, as numpy gives it"""
    with np.errstate(all="ignore"):
        return counts / np.array(np.diff(edges), float) / counts.sum()


def _key_to_float64(key):
    key = int(key)
    bits = key ^ (1 << 63) if key >> 63 else ~key & (2 ** 64 - 1)
    return np.array([bits], dtype=np.uint64).view(np.float64)[0]


def _ndwi(r, mask, bins, as_tensor=False):
    bins = _check_bins(bins)
    if r.n_bands < 4:
        raise ValueError(f"NDWI needs at least four bands (got {r.n_bands})")
    if tuple(mask.shape) != (r.h, r.w):
        raise ValueError(f"the mask must have the raster's size {(r.h, r.w)} (got {tuple(mask.shape)})")
    dev = r.t.device
    stats = torch.empty(8, device=dev, dtype=torch.int64)
    check(lib.runet_ndwi_stats(*r.args, mask.data_ptr(), stats.data_ptr(), ops.stream()))
    words = [int(v) & (2 ** 64 - 1) for v in stats.cpu().tolist()]                # the one synchronisation
    _raise_nonfinite(words[2])
    n = words[:2]
    lohi = [(None, None) if n[c] == 0 else (_key_to_float64(words[3 + 2 * c]), _key_to_float64(words[4 + 2 * c])) for c in range(2)]
    edges = np.stack([histogram_edges(lo, hi, bins) for lo, hi in lohi])
    counts = torch.empty((2, bins), device=dev, dtype=torch.int64)
    check(lib.runet_ndwi_hist(*r.args, mask.data_ptr(), torch.from_numpy(edges).to(dev).data_ptr(), bins, counts.data_ptr(), ops.stream()))
    if as_tensor:
        return {name: {"counts": counts[c], "edges": edges[c]} for c, name in enumerate(("water", "other"))}
    counts = counts.cpu().numpy()
    return {name: {"counts": counts[c], "edges": edges[c], "density": _density(counts[c], edges[c])} for c, name in enumerate(("water", "other"))}


def ndwi_histograms(bands, water_mask, bins=50, as_tensor=False, device="cuda"):
    """predict_coastline.py:789-813: NDWI = (green - nir) / (green + nir + 1e-8) in float64 (green = band 1, NIR = band 3 of a raster of at
    least four), and np.histogram(., bins, density=True) of it over the pixels with mask == 1 ("water") and with mask == 0 ("other").
    -> {"water": {"counts" int64 [bins], "edges" float64 [bins + 1], "density" float64 [bins]}, "other": {...}}; as_tensor: counts stay on
    the device and there is no density.  ValueError if a pixel of either class has a non-finite NDWI."""
    r = _scene.load_raster(bands, device)
    return _ndwi(r, _dev_u8(water_mask, r.t.device), bins, as_tensor)


def fold_byte_histogram(hist, bins=50):
    """exact byte counts int64 [256] -> (counts int64 [bins], edges) = np.histogram(the bytes, bins): np.histogram's own binning rule
    applied to the 256 values, each weighted by its count"""
    bins = _check_bins(bins)
    hist = np.asarray(hist, dtype=np.int64)
    present = np.flatnonzero(hist)
    counts = np.zeros(bins, dtype=np.int64)
    if present.size == 0:
        return counts, histogram_edges(None, None, bins)
    edges = histogram_edges(np.uint8(present[0]), np.uint8(present[-1]), bins)
    v = present.astype(np.float64)
    idx = (((v - edges[0]) / (edges[-1] - edges[0])) * bins).astype(np.intp)
    idx[idx == bins] -= 1
    idx[v < edges[idx]] -= 1
    idx[(v >= edges[idx + 1]) & (idx != bins - 1)] += 1
    np.add.at(counts, idx, hist[present])
    return counts, edges


def _rgb_hist(image):
    h, w, _ = image.shape
    if image.data_ptr() % 4:                             # a view off the 4-byte grid: the kernel reads whole dwords
        image = image.clone()
    hist = torch.empty((3, 256), device=image.device, dtype=torch.int64)
    check(lib.runet_rgb_hist_u8(image.data_ptr(), h, w, hist.data_ptr(), ops.stream()))
    return hist


def rgb_histograms(image_u8, bins=50, as_tensor=False, device="cuda"):
    """predict_coastline.py:821-829: np.histogram(channel, bins, density=True) of the three channels of a uint8 [H, W, 3] image, each over
    its own min..max.  The device counts every byte value exactly; the host folds the 256 counts into the bins.
    -> {"red" | "green" | "blue": {"counts", "edges", "density"}}; as_tensor: the device int64 [3, 256] byte counts, nothing else."""
    bins = _check_bins(bins)
    image = _dev_u8(image_u8, device)
    if image.dim() != 3 or image.shape[2] != 3:
        raise ValueError("expected a uint8 [H, W, 3] image")
    hist = _rgb_hist(image)
    return hist if as_tensor else _fold_rgb(hist.cpu().numpy(), bins)


def _fold_rgb(hist, bins):
    out = {}
    for c, name in enumerate(("red", "green", "blue")):
        counts, edges = fold_byte_histogram(hist[c], bins)
        out[name] = {"counts": counts, "edges": edges, "density": _density(counts, edges)}
    return out


def coastline_lengths(coastlines):
    """predict_coastline.py:763-770 -> [float]: the length of every coastline with more than one point as an OPEN polyline (the reference
    does not close it).  Per segment sqrt(dx^2 + dy^2) with the squares summed exactly in integers, then numpy's sum over the segments."""
    lengths = []
    for line in coastlines:
        if len(line) < 2:
            continue
        step = np.diff(np.asarray(line, dtype=np.int64).reshape(-1, 2), axis=0)
        lengths.append(float(np.sqrt((step * step).sum(axis=1)).sum()))
    return lengths


def _device_arrays(display, water, coast, raster, bins):
    """device display image and masks (+ the raster, or None) -> the per-pixel arrays of the report, downloaded: what analysis_report and
    the extractor (which calls this before its own download, while the scene and the masks are on the device) share"""
    overlay = _overlay(display, water, coast)
    if raster is not None and raster.n_bands >= 4:
        hist = {"ndwi": _ndwi(raster, water, bins)}
    else:
        hist = {"rgb_hist": _fold_rgb(_rgb_hist(display).cpu().numpy(), bins)}
    return {"display": display.cpu().numpy(), "combined_overlay": overlay.cpu().numpy(), **hist}


def _with_statistics(arrays, total, n_water, n_coast, coastlines):
    """+ the statistics of :739-742 and the lengths"""
    return {**arrays, "total_pixels": int(total), "water_pixels": int(n_water), "coastline_pixels": int(n_coast),
            "water_ratio": int(n_water) / int(total) * 100, "coastline_lengths": coastline_lengths(coastlines)}


def analysis_report(result, display=None, bands=None, device="cuda", bins=50):
    """The arrays of predict_coastline.py:708-835 for one extraction result (CoastlineExtractor.extract_coastline_from_image):
    {"display", "combined_overlay", "total_pixels", "water_pixels" (the sum of the mask, :740), "coastline_pixels", "water_ratio" (percent),
    "coastline_lengths", and "ndwi" (bands with at least four planes given) or "rgb_hist"}.
    display: the background image, uint8 [H, W, 3]; None: the "display"-mode image of `bands` (normalize_image_for_display), or, without
    bands, the file result["image_path"]."""
    bins = _check_bins(bins)
    raster = None if bands is None else _scene.load_raster(bands, device)
    if display is not None:
        disp = _dev_u8(display, device)
    elif raster is not None:
        disp, nonfinite = _scene._enhance(raster, "display")
        _raise_nonfinite(int(nonfinite.item()))
    else:
        from PIL import Image
        if not os.path.exists(str(result["image_path"])):
            raise ValueError(f"the result's image_path {result['image_path']!r} is not a file: pass the background as display= or the raster as bands=")
        disp = _dev_u8(np.array(Image.open(result["image_path"]).convert("RGB"), dtype=np.uint8), device)
    masks = (result["water_mask"], result["coastline_mask"])
    arrays = _device_arrays(disp, *(_dev_u8(m, device) for m in masks), raster, bins)
    water, coast = (m.cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m) for m in masks)
    return _with_statistics(arrays, water.size, np.sum(water, dtype=np.int64), np.sum(coast, dtype=np.int64), result["coastlines"])


_PANELS = [["scene", "scene", "water", "coast"],
           ["scene", "scene", "combined", "numbers"],
           ["lengths", "lengths", "hist", "hist"]]


def _picture(ax, array, title, **kw):
    ax.imshow(array, **kw)
    ax.set_title(title, fontsize=12)
    ax.set_axis_off()


def _steps(ax, hist, colour, label):
    """one density histogram as a filled step curve over its own edges; a class without pixels (density NaN) draws as zero"""
    ax.stairs(np.nan_to_num(hist["density"]), hist["edges"], fill=True, alpha=0.45, color=colour, label=label)


def create_coastsat_style_visualization(result, output_dir, report=None, display=None, bands=None, device="cuda"):
    """The reference's analysis figure (predict_coastline.py:659-846) from the report arrays: seven panels - the scene with the coastlines,
    the water region, the coastline band, the combined overlay, the numbers, the length of every coastline, and the NDWI or RGB
    histograms -> the path of <base>_coastsat_analysis.png (dpi 200).  report: analysis_report's dict (None: computed here from result,
    display, bands).  Layout, colours and wording are the project's own.  Only this function needs matplotlib."""
    if report is None:
        report = analysis_report(result, display=display, bands=bands, device=device)
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from matplotlib.colors import ListedColormap
    name = os.path.basename(str(result["image_path"]))
    fig, ax = plt.subplot_mosaic(_PANELS, figsize=(20, 12), gridspec_kw={"hspace": 0.3, "wspace": 0.25})

    _picture(ax["scene"], report["display"], f"{name}: {result['coastline_count']} coastlines", interpolation="nearest")
    for line in result["coastlines"]:
        xy = np.asarray(line).reshape(-1, 2)
        if len(xy) > 2:
            ax["scene"].plot(*xy.T, color="red", linewidth=2.5)
    _picture(ax["water"], np.asarray(result["water_mask"]) == 1, "water", cmap=ListedColormap(["black", (0.0, 0.4, 0.8)]), vmin=0, vmax=1,
             interpolation="nearest")
    _picture(ax["coast"], np.asarray(result["coastline_mask"]) == 1, "coastline band", cmap="gray", vmin=0, vmax=1, interpolation="nearest")
    _picture(ax["combined"], report["combined_overlay"], "water and coastline on the scene", interpolation="nearest")

    rows = [("image", "{} x {}".format(*result["image_size"])), ("pixels", f"{report['total_pixels']:,}"),
            ("water", f"{report['water_pixels']:,} ({report['water_ratio']:.1f} %)"), ("coastline band", f"{report['coastline_pixels']:,}"),
            ("coastlines", str(result["coastline_count"])), ("dilation", str(result.get("dilation_size", 5))),
            ("extracted", str(result["extraction_time"])[:19])]
    ax["numbers"].set_axis_off()
    table = ax["numbers"].table(cellText=rows, colWidths=[0.4, 0.6], cellLoc="left", loc="center", edges="horizontal")
    table.scale(1, 1.6)

    lengths = report["coastline_lengths"]
    ax["lengths"].set_title("coastline lengths (open polylines, pixels)", fontsize=12)
    if lengths:
        bars = ax["lengths"].bar(np.arange(1, len(lengths) + 1), lengths, color="tab:orange")
        ax["lengths"].bar_label(bars, fmt="%.0f", fontsize=8)
        ax["lengths"].set_xticks(np.arange(1, len(lengths) + 1))
        ax["lengths"].set_xlabel("coastline")

    if "ndwi" in report:
        _steps(ax["hist"], report["ndwi"]["other"], "saddlebrown", "not water")
        _steps(ax["hist"], report["ndwi"]["water"], "royalblue", "water")
        ax["hist"].set_title("NDWI = (green - NIR) / (green + NIR), density per class", fontsize=12)
    else:
        for channel in ("red", "green", "blue"):
            _steps(ax["hist"], report["rgb_hist"][channel], channel, channel)
        ax["hist"].set_title("pixel values, density per channel", fontsize=12)
    ax["hist"].legend()

    fig.suptitle("Coastline extraction report", fontsize=18)
    os.makedirs(output_dir, exist_ok=True)
    path = os.path.join(output_dir, f"{os.path.splitext(name)[0]}_coastsat_analysis.png")
    fig.savefig(path, dpi=200, bbox_inches="tight")
    plt.close(fig)
    return path


# ------------------------------------------------------------------------------------------------ B. the error maps
def class_colour_terms():
    """-> float64 [5, 3]: 0.6 * colour of TP, FP, FN, TN and of no class, as numpy's `0.6 * overlay` computes them"""
    return 0.6 * np.array(CLASS_COLOURS, dtype=np.float64)


def _f32_dev(a, device, shape_tail, what):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype != torch.float32 or t.dim() != 4 or t.shape[1] != shape_tail:
        raise ValueError(f"{what} must be a float32 [N, {shape_tail}, H, W] array")
    return t.to(device).contiguous()


def error_overlays(images, prob, masks, threshold=0.5, mean=data.IMAGENET_MEAN, std=data.IMAGENET_STD, as_tensor=False, device="cuda"):
    """Extended_Baseline_Comparison.py:882-959 for N samples at once, one pass over the pixels.  images: float32 [N, 3, H, W], normalised;
    prob, masks: float32 [N, 1, H, W].  ->
      "image"      float32 [N, H, W, 3]  (x * std + mean).clamp(0, 1), two float32 roundings (NaN stays NaN)
      "overlay"    float64 [N, H, W, 3]  0.4 * image + 0.6 * colour of the pixel's class: TP, FP, FN, TN from prob > threshold (NaN is not)
                                         and the mask; a mask value that is neither 0 nor 1 has no class and the colour (0, 0, 0)
      "error_map"  float32 [N, H, W]     |prob - mask|
      "counts"     int64 [N, 5]          pixels per class: tp, fp, fn, tn, none
      "error_sum"  float64 [N]           the sum of error_map in float64, in the fixed order stated in include/runet_hip.h
    and, unless as_tensor, on the host "iou" [N] = tp / (tp + fp + fn + 1e-8) and "mae" [N] = error_sum / (H * W).  The reference's np.mean
    of the float32 map adds pairwise in float32; mae differs from it by that float32 rounding only (it is printed to four decimals)."""
    images = _f32_dev(images, device, 3, "images")
    dev = images.device
    prob, masks = _f32_dev(prob, dev, 1, "prob"), _f32_dev(masks, dev, 1, "masks")
    n, _, h, w = images.shape
    if tuple(prob.shape) != (n, 1, h, w) or tuple(masks.shape) != (n, 1, h, w):
        raise ValueError("images, prob and masks must agree in N, H and W")
    nbytes = lib.runet_error_overlays_workspace_bytes(n, h, w)
    if nbytes < 0:
        raise ValueError(f"{n} samples of {h} x {w}: 1..65535 samples, h * w below 2^31")
    ws = torch.empty(nbytes // 8, device=dev, dtype=torch.float64)
    colours = torch.from_numpy(class_colour_terms()).to(dev)
    out = {"image": torch.empty((n, h, w, 3), device=dev, dtype=torch.float32), "overlay": torch.empty((n, h, w, 3), device=dev, dtype=torch.float64),
           "error_map": torch.empty((n, h, w), device=dev, dtype=torch.float32), "counts": torch.empty((n, 5), device=dev, dtype=torch.int64),
           "error_sum": torch.empty(n, device=dev, dtype=torch.float64)}
    check(lib.runet_error_overlays(images.data_ptr(), prob.data_ptr(), masks.data_ptr(), n, h, w, float(threshold), *(float(v) for v in mean),
                                   *(float(v) for v in std), colours.data_ptr(), out["image"].data_ptr(), out["overlay"].data_ptr(),
                                   out["error_map"].data_ptr(), out["counts"].data_ptr(), out["error_sum"].data_ptr(), ws.data_ptr(), nbytes,
                                   ops.stream()))
    if as_tensor:
        return out
    out = {k: v.cpu().numpy() for k, v in out.items()}
    tp, fp, fn = (out["counts"][:, i] for i in range(3))
    out["iou"] = tp / (tp + fp + fn + 1e-8)
    out["mae"] = out["error_sum"] / (h * w)
    return out


CLASS_LABELS = ("water found (TP)", "false alarm (FP)", "water missed (FN)", "land (TN)")


def draw_error_maps(images, masks, per_model, error_map, mae, save_path):
    """The figure of Extended_Baseline_Comparison.py:890-974 from its arrays, one row per sample: the image, the ground truth, one class
    overlay per model with its IoU, and the error map with its MAE.  images: float32 [n, H, W, 3] in 0..1; masks: [n, H, W]; per_model:
    {name: {"overlay" [n, H, W, 3], "iou" [n]}} in column order; error_map [n, H, W] and mae [n]: the last column."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from matplotlib.patches import Patch
    columns = ["image", "ground truth", *per_model, f"|p - g| of {OURS}"]
    fig, grid = plt.subplots(len(images), len(columns), figsize=(3.5 * len(columns), 3.5 * len(images)), squeeze=False, layout="constrained")
    for row, axes in enumerate(grid):
        cells = [(images[row], {}, None), (masks[row], {"cmap": "Blues", "vmin": 0, "vmax": 1}, None)]
        cells += [(np.clip(arrays["overlay"][row], 0, 1), {}, f"IoU {arrays['iou'][row]:.3f}") for arrays in per_model.values()]
        cells.append((error_map[row], {"cmap": "hot", "vmin": 0, "vmax": 1}, f"MAE {mae[row]:.4f}"))
        for ax, title, (array, kw, note) in zip(axes, columns, cells):
            ax.imshow(array, interpolation="nearest", **kw)
            ax.set_axis_off()
            if row == 0:
                ax.set_title(title, fontsize=11)
            if note:
                ax.annotate(note, (0.03, 0.97), xycoords="axes fraction", va="top", fontsize=9, color="white", backgroundcolor="black")
    fig.legend(handles=[Patch(color=c, label=t) for c, t in zip(CLASS_COLOURS, CLASS_LABELS)], loc="outside lower center", ncols=4)
    fig.savefig(save_path, dpi=300)
    plt.close(fig)
    return save_path


def error_map_arrays(models, val_loader, device, n_samples=6):
    """The arrays of Extended_Baseline_Comparison.py:870-959: the first n_samples samples of val_loader (it yields (images, masks, paths))
    -> (masks float32 [n, H, W], {model name: error_overlays' dict}).  Every model predicts one sample per call, as there; a prediction
    of another size than the masks is resized on the device (bilinear, align_corners=False), as there."""
    batches, have = [], 0
    for batch in val_loader:
        batches.append(batch[:2])
        have += len(batch[2])
        if have >= n_samples:
            break
    images, masks = (torch.cat(part)[:n_samples].to(device=device, dtype=torch.float32) for part in zip(*batches))
    per_model = {}
    for name, model in models.items():
        model.eval()
        with torch.no_grad():
            prob = torch.cat([model(x[None]) for x in images])
            if prob.shape[-2:] != masks.shape[-2:]:
                prob = torch.nn.functional.interpolate(prob, size=masks.shape[-2:], mode="bilinear", align_corners=False)
        per_model[name] = error_overlays(images, prob.float(), masks, device=device)
    return masks[:, 0].cpu().numpy(), per_model


def generate_error_maps(models, val_loader, device, save_dir="./error_maps"):
    """Extended_Baseline_Comparison.py:863-977: the first six validation samples, every model's TP / FP / FN overlay with its IoU, and the
    error map of models['Robust U-Net (Ours)'] with its MAE -> save_dir/error_maps_comparison.png, drawn from error_map_arrays."""
    if OURS not in models:
        raise KeyError(OURS)
    os.makedirs(save_dir, exist_ok=True)
    masks, per_model = error_map_arrays(models, val_loader, device)
    ours = per_model[OURS]
    return draw_error_maps(ours["image"], masks, per_model, ours["error_map"], ours["mae"], os.path.join(save_dir, "error_maps_comparison.png"))
