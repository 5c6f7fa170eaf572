"""Seeded inputs shared by test_report_ref_cpu.py and test_gpu_report.py: the cases at which the report kernels can go wrong."""
from fractions import Fraction

import numpy as np

from conftest import load_npz

SHAPES = [(1, 1), (3, 5), (37, 53), (64, 64), (129, 257)]      # one pixel; a tail only; odd; whole groups; more than one block and chunk
TAGS = ("u8", "u16", "i16", "f32")
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def golden_rasters():
    """the four 6 x 37 x 53 rasters of tests/golden/scene_bands.npz"""
    g = load_npz("scene_bands.npz")
    return {tag: g["in_" + tag] for tag in TAGS}


def masks(h, w, seed):
    rng = np.random.default_rng(seed)
    return {"random": rng.integers(0, 2, (h, w)).astype(np.uint8), "all water": np.ones((h, w), np.uint8),
            "all land": np.zeros((h, w), np.uint8), "with 2": rng.integers(0, 3, (h, w)).astype(np.uint8)}


def raster(tag, h, w, seed, bands=4):
    rng = np.random.default_rng(seed)
    if tag == "f32":
        return (rng.random((bands, h, w)) * 0.9 + 0.05).astype(np.float32)
    lo, hi = {"u8": (0, 256), "u16": (0, 65536), "i16": (1, 32768)}[tag]         # int16 stays positive: g + n + 1e-8 must not be 0
    return rng.integers(lo, hi, (bands, h, w)).astype({"u8": np.uint8, "u16": np.uint16, "i16": np.int16}[tag])


def image_u8(h, w, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    img.reshape(-1)[:min(256, img.size)] = np.arange(min(256, img.size))      # every byte value where the image is large enough
    return img


def constant_ndwi_raster(h=5, w=7):
    """green 300, NIR 100 everywhere: min == max"""
    a = np.zeros((4, h, w), np.uint16)
    a[1], a[3] = 300, 100
    return a


def on_edge_raster(lower=False):
    """float32 [4, 1, 51]: g = i 2^24, n = 2^30 - i 2^24, so NDWI = i / 32 - 1 lies exactly on the 51 edges of 50 bins over [-1, 0.5625];
    lower: g one float32 ulp below (0 stays 0)"""
    i = np.arange(51, dtype=np.float64)
    g = (i * 2.0 ** 24).astype(np.float32)
    n = (2.0 ** 30 - i * 2.0 ** 24).astype(np.float32)
    if lower:
        g = np.where(g > 0, np.nextafter(g, np.float32(0)), g).astype(np.float32)
    a = np.zeros((4, 1, 51), np.float32)
    a[1, 0], a[3, 0] = g, n
    return a


def fma_sensitive(c, count=8, seed=0):
    """float32 x for which fl32(fl32(x * std[c]) + mean[c]) differs from the single rounding of x * std[c] + mean[c] (what a fused
    multiply-add gives).  Only x whose exact sum float64 holds exactly are kept, so that its float32 rounding IS the fused result.
    -> (x, unfused, fused)"""
    rng = np.random.default_rng(seed + c)
    x = (rng.random(20000) * 4 - 2).astype(np.float32)
    s, m = np.float32(STD[c]), np.float32(MEAN[c])
    unfused = (x * s) + m
    wide = x.astype(np.float64) * np.float64(s) + np.float64(m)
    idx = [int(i) for i in np.flatnonzero(wide.astype(np.float32) != unfused)
           if Fraction(float(wide[i])) == Fraction(float(x[i])) * Fraction(float(s)) + Fraction(float(m))
           and 0 < unfused[i] < 1 and 0 < wide[i] < 1][:count]
    return x[idx], unfused[idx], wide[idx].astype(np.float32)


def error_case(n, h, w, seed):
    """-> images [n, 3, h, w], prob, masks [n, 1, h, w], float32.  Images clamp at both ends and start with the FMA-sensitive values;
    probabilities hold exact 0.5 and, in sample 0 only, NaN; masks hold 0.5."""
    rng = np.random.default_rng(seed)
    images = (rng.standard_normal((n, 3, h, w)) * 2.5).astype(np.float32)
    for c in range(3):
        x = fma_sensitive(c)[0]
        k = min(len(x), h * w)
        images[:, c].reshape(n, -1)[:, :k] = x[:k]
    prob = rng.random((n, 1, h, w)).astype(np.float32)
    u = rng.random((n, 1, h, w))
    prob[u < 0.1] = 0.5
    prob[0][(u[0] >= 0.1) & (u[0] < 0.15)] = np.nan
    masks_ = rng.integers(0, 2, (n, 1, h, w)).astype(np.float32)
    masks_[rng.random((n, 1, h, w)) < 0.1] = 0.5
    if h * w >= 4:                                       # small shapes too: one of each by hand
        prob.reshape(n, -1)[:, 0], prob.reshape(n, -1)[0, 1] = 0.5, np.nan
        masks_.reshape(n, -1)[:, 2] = 0.5
    return images, prob, masks_
