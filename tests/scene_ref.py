"""numpy-only restatement of the reference's scene ingestion (tif_to_image.py:78-171, predict_coastline.py:448-581): band selection and the
three enhancement modes, operation by operation in numpy's own promotion rules, so that it equals the reference bit for bit (checked against
tests/golden/scene_bands.npz, which the reference itself produced).  Constant bands are undefined there (0 / 0 cast to an integer)."""
import numpy as np


def select_bands(n_bands, mode="water"):
    n = min(n_bands, 6)
    if n < 3:
        return (0, 0, 0)
    if mode == "display":
        return (0, 1, 2)
    if mode == "water" and n >= 5:
        return (4, 3, 2)
    return (2, 1, 0)                             # also exactly four bands: bands[4] raises IndexError there and the fallback is taken


def stack(bands, mode):
    bands = np.asarray(bands)
    bands = bands[None] if bands.ndim == 2 else bands
    return np.dstack([bands[i] for i in select_bands(bands.shape[0], mode)])


def enhance(rgb, mode):
    """rgb: [H, W, 3] in the raster's dtype -> [H, W, 3] in the same dtype (the reference's zeros_like), before the final astype(uint8)"""
    out = np.zeros_like(rgb)
    for i in range(3):
        band = rgb[:, :, i].astype(np.float64) if mode == "display" else rgb[:, :, i]
        p2, p98 = np.percentile(band, [2, 98])
        if mode != "display" or p98 - p2 > 0:
            s = np.clip((band - p2) / (p98 - p2) * 255, 0, 255)
        else:
            s = np.clip(band, 0, 255)
        if mode == "water" and i == 0:
            low = s < 100
            s[low] = s[low] * 0.7
        out[:, :, i] = s
    return out


def enhance_scene(bands, mode="water"):
    """[B, H, W] or [H, W] raster -> uint8 [H, W, 3]"""
    with np.errstate(all="ignore"):
        return enhance(stack(bands, mode), mode).astype(np.uint8)
