"""The rules behind the device input pipeline restated in integer / float32 numpy, executing the package's own host tables
(device_data.resample_tables, nearest_table, rotation_words), and the PIL chains they stand in for.  PIL is the judge: test_input_ref_cpu.py
holds the restatement to it on the host, test_gpu_device_data.py holds the kernels to it on the device.  The case list is shared."""
import importlib

import numpy as np
import torch
from PIL import Image, ImageEnhance, ImageStat

DD = importlib.import_module("eusipco-2026-robust-unet_amd.device_data")
DATA = importlib.import_module("eusipco-2026-robust-unet_amd.data")

# (H, W) -> (h, w)
RESIZE_SHAPES = [((37, 53), (16, 16)), ((16, 16), (64, 64)), ((33, 64), (64, 64)), ((64, 31), (64, 64)), ((211, 307), (64, 64)),
                 ((5, 7), (64, 64)), ((1, 1), (8, 8)), ((64, 64), (64, 64))]
UPSCALING = [((16, 16), (64, 64)), ((5, 7), (64, 64)), ((33, 64), (64, 64))]         # the shapes that must clamp in both directions
PIL_FILTER = {"lanczos": Image.LANCZOS, "bilinear": Image.BILINEAR, "nearest": Image.NEAREST}
ENHANCERS = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)    # numbered as device_data.BRIGHTNESS / CONTRAST / SATURATION
ANGLES = (0.0, 10.0, -10.0, 3.7)
_CACHE = {}


def shape_id(case):
    (h, w), (oh, ow) = case
    return f"{h}x{w}-{oh}x{ow}"


def content(h, w, c, seed=0):
    """Random bytes with the top half replaced by 3-pixel blocks of 0 / 255 (steps that make LANCZOS overshoot both ways).  uint8 [h, w, c]"""
    key = ("content", h, w, c, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 * seed + 7 * h + w)
        a = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        yy, xx = np.mgrid[0:h, 0:w]
        blocks = (((yy // 3 + xx // 3) & 1) * 255).astype(np.uint8)
        top = (h + 1) // 2
        a[:top] = blocks[:top, :, None]
        a.setflags(write=False)
        _CACHE[key] = a
    return _CACHE[key]


def mask_content(h, w, seed=0):
    rng = np.random.default_rng(77 + 1000 * seed + 7 * h + w)
    return (rng.integers(0, 4, (h, w)) == 0).astype(np.uint8)


def to_pil(a):
    a = np.ascontiguousarray(a)
    return Image.fromarray(a[:, :, 0] if a.ndim == 3 and a.shape[2] == 1 else a)


def pil_resize(a, size_wh, filter):
    """Image.resize on a uint8 array [H, W] / [H, W, 1] / [H, W, 3]; the result has the input's rank."""
    out = np.asarray(to_pil(a).resize(tuple(size_wh), PIL_FILTER[filter]), dtype=np.uint8)
    return out[:, :, None] if a.ndim == 3 and a.shape[2] == 1 else out


# --------------------------------------------------------------------------- numpy restatement
def _pass(a, axis, out_size, filter, extremes):
    """One resampling pass along `axis` of uint8 [H, W, C] from the package's tables; int32 accumulator, arithmetic shift, clamp."""
    bounds, coeffs = DD.resample_tables(a.shape[axis], out_size, filter)
    src = np.moveaxis(a, axis, 0).astype(np.int32)
    out = np.empty((out_size,) + src.shape[1:], np.uint8)
    for o in range(out_size):
        first, n = int(bounds[o, 0]), int(bounds[o, 1])
        acc = np.full(src.shape[1:], 1 << 21, np.int32)
        for t in range(n):
            acc = acc + coeffs[o, t] * src[first + t]
        v = acc >> 22
        extremes[0], extremes[1] = min(extremes[0], int(v.min())), max(extremes[1], int(v.max()))
        out[o] = np.clip(v, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize_ref(a, size_wh, filter, extremes=None):
    """Image.resize(size, LANCZOS | BILINEAR) restated: horizontal pass, then vertical, each skipped when its dimension is unchanged.
    extremes: a [lo, hi] list updated with the values in front of the clamp."""
    a3 = a if a.ndim == 3 else a[:, :, None]
    ex = extremes if extremes is not None else [0, 0]
    ow, oh = size_wh
    if ow != a3.shape[1]:
        a3 = _pass(a3, 1, ow, filter, ex)
    if oh != a3.shape[0]:
        a3 = _pass(a3, 0, oh, filter, ex)
    return np.ascontiguousarray(a3 if a.ndim == 3 else a3[:, :, 0])


def nearest_ref(a, size_wh):
    return np.ascontiguousarray(a[DD.nearest_table(a.shape[0], size_wh[1])][:, DD.nearest_table(a.shape[1], size_wh[0])])


def gray_ref(a):
    a = a.astype(np.int64)
    return ((19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 32768) >> 16).astype(np.int32)


def blend_ref(d, a, f):
    """Image.blend(degenerate d, image a, f) on int arrays: float32 product rounded before the float32 add."""
    f = np.float32(f)
    t = d.astype(np.float32) + (f * (a.astype(np.int32) - d.astype(np.int32)).astype(np.float32)).astype(np.float32)
    if 0.0 <= f <= 1.0:
        return np.trunc(t).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(t))).astype(np.uint8)


def enhance_ref(a, which, f):
    """-> (uint8 [H, W, 3], the contrast mean or None)"""
    if which == DD.BRIGHTNESS:
        return blend_ref(np.zeros_like(a), a, f), None
    if which == DD.CONTRAST:
        l = gray_ref(a)
        mean = int(int(l.sum()) / l.size + 0.5)
        return blend_ref(np.full_like(a, mean), a, f), mean
    return blend_ref(np.repeat(gray_ref(a)[..., None], 3, axis=2), a, f), None


def rotate_ref(a, angle):
    """Image.rotate(angle, NEAREST, expand=False, fillcolor=0) from the package's rotation words."""
    h, w = a.shape[:2]
    a0, a1, a2, a3, a4, a5 = (int(v) for v in DD.rotation_words(w, h, angle))
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    sx, sy = (a2 + y * a1 + x * a0) >> 16, (a5 + y * a4 + x * a3) >> 16
    ok = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    out = np.zeros_like(a)
    out[ok] = a[sy[ok], sx[ok]]
    return out


def augment_ref(img, mask, flip, angle, factors, order, masks="follow"):
    """numpy chain -> (uint8 [S, S, 3], uint8 [S, S], contrast mean)"""
    a, m = img, mask
    if flip:
        a = a[:, ::-1]
        m = m[:, ::-1] if masks == "follow" else m
    a = rotate_ref(a, angle)
    m = rotate_ref(m, angle) if masks == "follow" else m
    cmean = None
    for which in order:
        a, c = enhance_ref(a, which, factors[which])
        cmean = c if c is not None else cmean
    return np.ascontiguousarray(a), np.ascontiguousarray(m), cmean


# --------------------------------------------------------------------------- the PIL chain (the reference)
def pil_augment(img, mask, flip, angle, factors, order, masks="follow"):
    """torchvision's RandomHorizontalFlip -> RandomRotation -> ColorJitter as the PIL calls they make -> (uint8 [S, S, 3], uint8 [S, S],
    the contrast mean ImageEnhance.Contrast took)."""
    a, m = to_pil(img), to_pil(mask)
    if flip:
        a = a.transpose(Image.FLIP_LEFT_RIGHT)
        m = m.transpose(Image.FLIP_LEFT_RIGHT) if masks == "follow" else m
    a = a.rotate(angle, Image.NEAREST, expand=False, fillcolor=0)
    m = m.rotate(angle, Image.NEAREST, expand=False, fillcolor=0) if masks == "follow" else m
    cmean = None
    for which in order:
        if which == DD.CONTRAST:
            cmean = int(ImageStat.Stat(a.convert("L")).mean[0] + 0.5)
        a = ENHANCERS[which](a).enhance(float(factors[which]))
    return np.asarray(a, dtype=np.uint8), np.asarray(m, dtype=np.uint8), cmean


def normalize_ref(u8_hwc):
    """ToTensor + Normalize on the host in float32: uint8 [..., S, S, 3] -> float32 [..., 3, S, S]"""
    t = torch.from_numpy(np.array(u8_hwc)).movedim(-1, -3).float() / 255
    mean = torch.tensor(DATA.IMAGENET_MEAN, dtype=torch.float32).view(3, 1, 1)
    std = torch.tensor(DATA.IMAGENET_STD, dtype=torch.float32).view(3, 1, 1)
    return ((t - mean) / std).contiguous()


def augment_cases(size):
    """The parameter sets of the augmentation tests for a size x size cache of M = 7 samples: every order with every listed angle and factor,
    flip on and off.  -> list of dicts (index, flip, angle, factors float32 [3], order tuple)"""
    drawn = DD.Augment().draw(4, seed=3, epoch=1)
    fsets = [np.array(v, np.float32) for v in ((0.9, 0.9, 0.9), (1.0, 1.0, 1.0), (1.1, 1.1, 1.1), (0.9, 1.1, 1.0))] + [drawn["factors"][0]]
    cases, k = [], 0
    for order in DD.ORDERS:
        for angle in ANGLES + (float(drawn["angle"][1]),):
            cases.append({"index": (5 * k + 6) % 7, "flip": k & 1, "angle": angle, "factors": fsets[k % len(fsets)], "order": order})
            k += 1
    for j, f in enumerate(fsets):                          # every factor set with flip on and off, whatever the walk above paired
        for flip in (0, 1):
            cases.append({"index": (j + 3 * flip) % 7, "flip": flip, "angle": ANGLES[(j + flip) % 4], "factors": f, "order": DD.ORDERS[(j + 2 * flip) % 6]})
    return cases


def cache_content(size, m=7):
    """A byte cache of m samples: images uint8 [m, size, size, 3] (sample 0 holds all 256 byte values in every channel when it has room),
    masks uint8 [m, size, size] in {0, 1}."""
    key = ("cache", size, m)
    if key not in _CACHE:
        imgs = np.stack([content(size, size, 3, seed=10 + i) for i in range(m)]).copy()
        if size * size >= 256:
            ramp = np.arange(size * size, dtype=np.int64) % 256
            imgs[0] = np.stack([ramp, (ramp * 7 + 3) % 256, 255 - ramp], axis=-1).reshape(size, size, 3).astype(np.uint8)
        masks = np.stack([mask_content(size, size, seed=i) for i in range(m)])
        imgs.setflags(write=False)
        masks.setflags(write=False)
        _CACHE[key] = (imgs, masks)
    return _CACHE[key]
