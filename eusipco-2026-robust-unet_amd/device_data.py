"""Device-resident dataset: every sample is decoded, rasterised and resized ONCE, kept on the device as bytes, and every batch is assembled
there (shuffle, augmentation, ToTensor, Normalize in one pass; csrc/input_pipeline.hip).  The host pipeline of data.py builds each sample
again on every epoch (Main_Final.py:40-54) and has no augmentation; this module stands in for PIL and is exact against it, byte for byte:

  Image.resize(size, LANCZOS | BILINEAR) on 8-bit images   resample_tables  + runet_resample8_rows / runet_resample8_cols
  Image.resize(size, NEAREST)                                nearest_table    + runet_gather2d_u8
  the train_transform of train_water_segmentation.py:313-321 (RandomHorizontalFlip, RandomRotation(10), ColorJitter(0.1, 0.1, 0.1),
  ToTensor, Normalize)                                       rotation_words, Augment + runet_batch_gray_sums / runet_batch_assemble

The tables and the fixed-point rotation words are made on the host in double precision, by PIL's own rules (Resample.c precompute_coeffs /
normalize_coeffs_8bpc, Geometry.c ImagingScaleAffine / affine_fixed, Image.rotate); the kernels only apply them.  The host rules import
without the HIP library; everything that computes needs it and a device.  Out of scope: decode and rasterisation on the device, hue jitter,
rotation with interpolation or `expand`, multiples of 90 degrees, TIF datasets, torch's RNG stream.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from . import portable_rng as prng
from .data import IMAGENET_MEAN, IMAGENET_STD, CoastalDataset

FILTER_SUPPORT = {"lanczos": 3.0, "bilinear": 1.0}
PRECISION_BITS = 22                     # PIL: 32 - 8 - 2
MAX_TAPS = 255                          # runet_resample8_*: the coefficient rows of one block stay in LDS
MAX_SIDE = 4096                         # runet_batch_*: 16.16 source coordinates and x * a0 stay inside int32
BRIGHTNESS, CONTRAST, SATURATION = 0, 1, 2
ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
MASK_MODES = {"fixed": 0, "follow": 1}
_TABLES = {}
_DEV_TABLES = {}


# --------------------------------------------------------------------------- host rules (pure Python / numpy)
def _lanczos(x):
    if -3.0 <= x < 3.0:
        def sinc(v):
            if v == 0.0:
                return 1.0
            v = v * math.pi
            return math.sin(v) / v
        return sinc(x) * sinc(x / 3)
    return 0.0


def _bilinear(x):
    if x < 0.0:
        x = -x
    return 1.0 - x if x < 1.0 else 0.0


_FILTERS = {"lanczos": _lanczos, "bilinear": _bilinear}


def resample_tables(in_size, out_size, filter="lanczos"):
    """One pass of PIL's 8-bit Image.resize along a dimension of in_size -> out_size pixels: (bounds int32 [out_size, 2] = (first source
    index, tap count), coeffs int32 [out_size, ksize] = the 22-bit fixed-point weights, zero past the tap count).  Double precision, the
    weights summed left to right and normalised by their sum, rounded half away from zero - PIL's precompute_coeffs / normalize_coeffs_8bpc."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("sizes must be positive")
    if filter not in _FILTERS:
        raise ValueError(f"filter must be one of {sorted(_FILTERS)}")
    key = (in_size, out_size, filter)
    if key in _TABLES:
        return _TABLES[key]
    fn = _FILTERS[filter]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = FILTER_SUPPORT[filter] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((out_size, 2), np.int32)
    coeffs = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [fn((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, xmax)
        coeffs[xx, :xmax] = [int(0.5 + v * (1 << PRECISION_BITS)) if v >= 0 else int(-0.5 + v * (1 << PRECISION_BITS)) for v in w]
    bounds.setflags(write=False)
    coeffs.setflags(write=False)
    _TABLES[key] = (bounds, coeffs)
    return _TABLES[key]


def nearest_table(in_size, out_size):
    """Source index of every output index of Image.resize(NEAREST) along one dimension, int32 [out_size]: int(xo) with xo = scale / 2
    accumulated by repeated addition of scale in double precision, as ImagingScaleAffine does."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("sizes must be positive")
    key = (in_size, out_size, "nearest")
    if key in _TABLES:
        return _TABLES[key]
    scale = in_size / out_size
    tab = np.empty(out_size, np.int32)
    xo = scale * 0.5
    for x in range(out_size):
        tab[x] = -1 if xo < 0.0 else int(xo)
        xo += scale
    if tab.min() < 0 or tab.max() >= in_size:       # PIL leaves such pixels unwritten; the rule cannot reach it for in, out >= 1
        raise ValueError(f"nearest table {in_size} -> {out_size} leaves the source")
    tab.setflags(write=False)
    _TABLES[key] = tab
    return tab


def _fix(v):
    return int(math.floor(v * 65536.0 + 0.5))


def rotation_words(w, h, angle):
    """The six 16.16 fixed-point words (a0 .. a5) with which Image.rotate(angle, NEAREST, expand=False, fillcolor=0) reads its source: output
    (x, y) takes source ((a2 + y a1 + x a0) >> 16, (a5 + y a4 + x a3) >> 16), or 0 outside the image.  Angle 0 (a copy in PIL) gives the
    identity words, which read the same bytes; the other multiples of 90 take PIL's transpose path and are refused."""
    angle = float(angle) % 360.0
    if angle in (90.0, 180.0, 270.0):
        raise ValueError("multiples of 90 degrees take another path in PIL and are not supported")
    cx, cy = w / 2.0, h / 2.0
    r = -math.radians(angle)
    m = [round(math.cos(r), 15), round(math.sin(r), 15), 0.0, round(-math.sin(r), 15), round(math.cos(r), 15), 0.0]
    m[2] = m[0] * -cx + m[1] * -cy + m[2] + cx
    m[5] = m[3] * -cx + m[4] * -cy + m[5] + cy
    words = np.array([_fix(m[0]), _fix(m[1]), _fix(m[2] + m[0] * 0.5 + m[1] * 0.5),
                      _fix(m[3]), _fix(m[4]), _fix(m[5] + m[3] * 0.5 + m[4] * 0.5)], np.int64)
    if np.abs(words).max() >= 1 << 31:
        raise ValueError("rotation words do not fit int32")
    return words.astype(np.int32)


def pack_order(order):
    """(first, second, third) of BRIGHTNESS / CONTRAST / SATURATION -> the packed permutation of the kernels, two bits per step."""
    order = tuple(int(o) for o in order)
    if sorted(order) != [0, 1, 2]:
        raise ValueError("order must be a permutation of (0, 1, 2)")
    return order[0] | order[1] << 2 | order[2] << 4


class Augment:
    """The training augmentation of train_water_segmentation.py:313-321 as explicit per-sample parameters: horizontal flip with probability
    flip_p, rotation by an angle in [-degrees, degrees] (nearest, no expand, fill 0), then brightness, contrast and saturation with factors in
    [1 - v, 1 + v] in a random order of the three.  masks="follow" applies the flip and the rotation to the mask too; "fixed" leaves the mask
    alone, as the reference does (its label then no longer matches the image).  The draws come from portable_rng and are reproducible from
    (seed, epoch); they do not follow torch's RNG stream."""

    def __init__(self, flip_p=0.5, degrees=10.0, brightness=0.1, contrast=0.1, saturation=0.1, masks="follow"):
        if masks not in MASK_MODES:
            raise ValueError(f"masks must be one of {sorted(MASK_MODES)}")
        if not 0.0 <= float(degrees) < 90.0:
            raise ValueError("degrees must be in [0, 90)")
        if not 0.0 <= float(flip_p) <= 1.0:
            raise ValueError("flip_p must be in [0, 1]")
        for v in (brightness, contrast, saturation):
            if not 0.0 <= float(v) <= 1.0:
                raise ValueError("jitter ranges must be in [0, 1]")
        self.flip_p, self.degrees = float(flip_p), float(degrees)
        self.ranges = (float(brightness), float(contrast), float(saturation))
        self.masks = masks

    def draw(self, n, seed=0, epoch=0):
        """-> dict of host arrays for n samples: flip int32 [n], angle float64 [n], factors float32 [n, 3] (brightness, contrast,
        saturation), order int32 [n] (pack_order)."""
        u = prng.uniform(6 * n, prng.name_seed("augment", int(seed) * 1000003 + int(epoch))).reshape(6, n)
        flip = (u[0] < self.flip_p).astype(np.int32)
        angle = (2.0 * u[1] - 1.0) * self.degrees
        factors = np.stack([1.0 + (2.0 * u[2 + k] - 1.0) * self.ranges[k] for k in range(3)], axis=1).astype(np.float32)
        which = np.minimum((u[5] * 6).astype(np.int64), 5)
        order = np.array([pack_order(ORDERS[k]) for k in which], np.int32).reshape(n)
        return {"flip": flip, "angle": angle, "factors": factors, "order": order}


def geometry_words(size, flip, angle, order):
    """The per-sample int32 [n, 8] block of the batch kernels: flip flag, the six rotation words of a size x size image, the packed order."""
    n = len(flip)
    g = np.empty((n, 8), np.int32)
    for i in range(n):
        g[i, 0] = int(flip[i]) != 0
        g[i, 1:7] = rotation_words(size, size, float(angle[i]))
        g[i, 7] = int(order[i])
    return g


def epoch_permutation(n, seed, epoch, shuffle=True):
    """The visiting order of epoch `epoch`: a permutation of range(n) from (seed, epoch), or range(n) itself."""
    if not shuffle:
        return np.arange(n, dtype=np.int64)
    return np.argsort(prng.uniform(n, prng.name_seed("epoch_order", int(seed) * 1000003 + int(epoch))), kind="stable").astype(np.int64)


def rank_share(order, rank=0, world=1):
    """Rank `rank`'s strided share of an epoch order."""
    if not 0 <= rank < world:
        raise ValueError("rank must be in [0, world)")
    return order[rank::world]


def batch_slices(n, batch_size, drop_last=False):
    """[(start, stop)] of the batches over n items."""
    if batch_size < 1:
        raise ValueError("batch_size must be positive")
    stop = n - n % batch_size if drop_last else n
    return [(i, min(i + batch_size, stop)) for i in range(0, stop, batch_size)]


# --------------------------------------------------------------------------- device side
def _native():
    from . import ops
    from ._lib import check, lib
    return lib, check, ops.stream


def _dev_i32(a, device):
    return torch.from_numpy(np.array(a, dtype=np.int32)).to(device)


def _dev_tables(in_size, out_size, filter, device):
    """The tables of one pass on the device, uploaded once per (in, out, filter, device): (bounds, coeffs, ksize) or the nearest index table."""
    key = (in_size, out_size, filter, str(device))
    if key not in _DEV_TABLES:
        if filter == "nearest":
            _DEV_TABLES[key] = _dev_i32(nearest_table(in_size, out_size), device)
        else:
            bounds, coeffs = resample_tables(in_size, out_size, filter)
            if coeffs.shape[1] > MAX_TAPS:
                raise ValueError(f"{in_size} -> {out_size} needs {coeffs.shape[1]} taps; the device resampler takes at most {MAX_TAPS}")
            _DEV_TABLES[key] = (_dev_i32(bounds, device), _dev_i32(coeffs, device), coeffs.shape[1])
    return _DEV_TABLES[key]


def resize_pil_device(u8_hwc, size, filter="lanczos"):
    """PIL's Image.resize(size, filter) of an 8-bit image on the device.  u8_hwc: device uint8 [H, W], [H, W, 1] or [H, W, 3]; size: (width,
    height) as PIL takes it; filter: "lanczos", "bilinear" or "nearest" (one channel only, the mask's resize).  Returns a new tensor of the
    input's rank; the bytes equal PIL's."""
    if not isinstance(u8_hwc, torch.Tensor) or u8_hwc.dtype != torch.uint8 or not u8_hwc.is_cuda or u8_hwc.ndim not in (2, 3):
        raise ValueError("expected a uint8 device tensor [H, W] or [H, W, C]")
    lib, check, stream = _native()
    src = u8_hwc.contiguous()
    h, w = src.shape[:2]
    c = 1 if src.ndim == 2 else src.shape[2]
    ow, oh = int(size[0]), int(size[1])
    if c not in (1, 3) or min(h, w, ow, oh) < 1:
        raise ValueError("expected 1 or 3 channels and positive sizes")
    shape = (oh, ow) if src.ndim == 2 else (oh, ow, c)
    dev = src.device
    with torch.cuda.device(dev):
        if filter not in ("nearest", "lanczos", "bilinear"):
            raise ValueError("filter must be lanczos, bilinear or nearest")
        if filter == "nearest":
            if c != 1:
                raise ValueError("the nearest resize is the mask's: one channel")
            dst = torch.empty(shape, dtype=torch.uint8, device=dev)
            yt, xt = _dev_tables(h, oh, "nearest", dev), _dev_tables(w, ow, "nearest", dev)
            check(lib.runet_gather2d_u8(src.data_ptr(), h, w, yt.data_ptr(), xt.data_ptr(), dst.data_ptr(), oh, ow, stream()))
            return dst
        cur = src
        if ow != w:
            bd, cd, ksize = _dev_tables(w, ow, filter, dev)
            nxt = torch.empty((h, ow, c), dtype=torch.uint8, device=dev)
            check(lib.runet_resample8_rows(cur.data_ptr(), h, w, c, bd.data_ptr(), cd.data_ptr(), ksize, nxt.data_ptr(), ow, stream()))
            cur = nxt
        if oh != h:
            bd, cd, ksize = _dev_tables(h, oh, filter, dev)
            nxt = torch.empty((oh, ow, c), dtype=torch.uint8, device=dev)
            check(lib.runet_resample8_cols(cur.data_ptr(), h, ow, c, bd.data_ptr(), cd.data_ptr(), ksize, nxt.data_ptr(), oh, stream()))
            cur = nxt
        if cur is src:
            cur = src.clone()
        return cur.reshape(shape)


def assemble_batch(images, masks, index, mean=IMAGENET_MEAN, std=IMAGENET_STD, geom=None, factors=None, mask_mode="follow"):
    """One batch from the byte cache.  images uint8 [M, S, S, 3], masks uint8 [M, S, S], index int32 [B] (any order, repeats allowed), all on
    one device; geom int32 [B, 8] (geometry_words) and factors float32 [B, 3] switch the augmentation on.  Returns (images float32
    [B, 3, S, S], masks float32 [B, 1, S, S], gray_sums int64 [B] or None): gray_sums are the integer sums of L in front of each sample's
    contrast step, from which the kernel takes PIL's contrast mean int(sum / S^2 + 0.5)."""
    lib, check, stream = _native()
    m, s = images.shape[0], images.shape[1]
    b = index.shape[0]
    if images.dtype != torch.uint8 or masks.dtype != torch.uint8 or tuple(images.shape) != (m, s, s, 3) or tuple(masks.shape) != (m, s, s):
        raise ValueError("expected a uint8 cache [M, S, S, 3] with masks [M, S, S]")
    if index.dtype != torch.int32 or index.ndim != 1 or (geom is None) != (factors is None):
        raise ValueError("index must be int32 [B]; geom and factors come together")
    if geom is not None and (geom.dtype != torch.int32 or tuple(geom.shape) != (b, 8) or factors.dtype != torch.float32
                             or tuple(factors.shape) != (b, 3)):
        raise ValueError("geom must be int32 [B, 8] and factors float32 [B, 3]")
    dev = images.device
    with torch.cuda.device(dev):
        out_i = torch.empty((b, 3, s, s), dtype=torch.float32, device=dev)
        out_m = torch.empty((b, 1, s, s), dtype=torch.float32, device=dev)
        sums = None
        if geom is not None:
            geom, factors = geom.contiguous(), factors.contiguous()
            sums = torch.empty(b, dtype=torch.int64, device=dev)
            check(lib.runet_batch_gray_sums(images.data_ptr(), m, s, index.data_ptr(), b, geom.data_ptr(), factors.data_ptr(), sums.data_ptr(),
                                            stream()))
        check(lib.runet_batch_assemble(images.data_ptr(), masks.data_ptr(), m, s, index.data_ptr(), b, mean[0], mean[1], mean[2], std[0],
                                       std[1], std[2], geom.data_ptr() if geom is not None else None,
                                       factors.data_ptr() if factors is not None else None, sums.data_ptr() if sums is not None else None,
                                       MASK_MODES[mask_mode], out_i.data_ptr(), out_m.data_ptr(), stream()))
    return out_i, out_m, sums


class DeviceCoastalDataset:
    """CoastalDataset built once and kept on the device as bytes: per sample the host runs load_image and the Labelme rasteriser of data.py
    (unchanged, the same fallbacks: unreadable image -> grey 512 x 512, unreadable JSON -> empty mask), the native-size bytes are uploaded
    and resampled there (LANCZOS for the image, NEAREST for the mask) into `images` uint8 [M, S, S, 3] and `masks` uint8 [M, S, S].  Costs
    4 bytes per pixel per sample of device memory (1 MiB per 512 x 512 sample).  image_size must be square; tables are cached per (in, out)."""

    def __init__(self, image_paths, label_paths, image_size=(512, 512), device="cuda"):
        if len(image_paths) != len(label_paths):
            raise ValueError("image_paths and label_paths must pair up")
        if int(image_size[0]) != int(image_size[1]) or not 1 <= int(image_size[0]) <= MAX_SIDE:
            raise ValueError(f"the device dataset takes square sizes up to {MAX_SIDE}")
        self.image_paths, self.label_paths = list(image_paths), list(label_paths)
        self.image_size = (int(image_size[0]), int(image_size[1]))
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("DeviceCoastalDataset needs a GPU device; data.CoastalDataset is the host dataset")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        s = self.image_size[0]
        host = CoastalDataset(self.image_paths, self.label_paths, image_size=self.image_size)
        self.images = torch.empty((len(host), s, s, 3), dtype=torch.uint8, device=self.device)
        self.masks = torch.empty((len(host), s, s), dtype=torch.uint8, device=self.device)
        for i in range(len(host)):
            image = host.load_image(self.image_paths[i])
            mask = host.create_mask_from_labelme(self.label_paths[i], image.size)
            img = torch.from_numpy(np.array(image, dtype=np.uint8)).to(self.device)
            msk = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8)).to(self.device)
            self.images[i] = resize_pil_device(img, self.image_size, "lanczos")
            self.masks[i] = resize_pil_device(msk, self.image_size, "nearest")

    def __len__(self):
        return len(self.image_paths)


class DeviceLoader:
    """Batches of a DeviceCoastalDataset, assembled on the device: iterating yields (images float32 [B, 3, S, S], masks float32
    [B, 1, S, S]) device tensors, the contract of data.prepare_dataset's loaders, so it goes through DevicePrefetcher and fit unchanged.
    Each iteration is one epoch; its order comes from (seed, epoch) via portable_rng (epoch counts the iterations, or set_epoch), ranks take
    strided shares of it.  One upload of the epoch's indices and augmentation parameters per epoch; no host work per batch but the launches."""

    def __init__(self, dataset, batch_size, shuffle=False, seed=0, augment=None, drop_last=False, rank=0, world=1):
        if not 0 <= rank < world:
            raise ValueError("rank must be in [0, world)")
        if batch_size < 1:
            raise ValueError("batch_size must be positive")
        self.dataset, self.batch_size, self.shuffle, self.seed = dataset, int(batch_size), bool(shuffle), int(seed)
        self.augment, self.drop_last, self.rank, self.world = augment, bool(drop_last), int(rank), int(world)
        self.epoch = 0

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def indices(self, epoch):
        """This rank's sample indices of an epoch (host int64)."""
        return rank_share(epoch_permutation(len(self.dataset), self.seed, epoch, self.shuffle), self.rank, self.world)

    def parameters(self, epoch):
        """The augmentation parameters (Augment.draw) of this rank's samples of an epoch, in the order of indices(epoch); None without augment."""
        if self.augment is None:
            return None
        return self.augment.draw(len(self.indices(epoch)), self.seed * self.world + self.rank, epoch)

    def __len__(self):
        return len(batch_slices(len(self.indices(0)), self.batch_size, self.drop_last))

    def __iter__(self):
        epoch = self.epoch
        self.epoch += 1
        ds = self.dataset
        idx = self.indices(epoch)
        dev = ds.device
        index = _dev_i32(idx, dev)
        geom = factors = None
        p = self.parameters(epoch)
        if p is not None:
            geom = _dev_i32(geometry_words(ds.image_size[0], p["flip"], p["angle"], p["order"]), dev)
            factors = torch.from_numpy(p["factors"]).to(dev)
        mode = self.augment.masks if self.augment is not None else "follow"
        for a, b in batch_slices(len(idx), self.batch_size, self.drop_last):
            images, masks, _ = assemble_batch(ds.images, ds.masks, index[a:b], geom=None if geom is None else geom[a:b],
                                              factors=None if factors is None else factors[a:b], mask_mode=mode)
            yield images, masks


def prepare_device_dataset(images_dir, labels_dir, batch_size=4, image_size=(512, 512), device="cuda", augment=None, seed=0):
    """data.prepare_dataset with device-resident loaders: the same sorted listing, image / JSON pairing by basename and first 80 % train /
    last 20 % validation split; the training loader is shuffled (from `seed`) and takes `augment`, the validation loader neither."""
    image_files, label_files = [], []
    for img_file in sorted(os.listdir(images_dir)):
        if img_file.lower().endswith((".png", ".jpg", ".jpeg")):
            label_path = os.path.join(labels_dir, os.path.splitext(img_file)[0] + ".json")
            if os.path.exists(label_path):
                image_files.append(os.path.join(images_dir, img_file))
                label_files.append(label_path)
    print(f"Found {len(image_files)} valid image-label pairs")
    if not image_files:
        return None
    split = int(0.8 * len(image_files))
    train = DeviceCoastalDataset(image_files[:split], label_files[:split], image_size=image_size, device=device)
    val = DeviceCoastalDataset(image_files[split:], label_files[split:], image_size=image_size, device=device)
    return (DeviceLoader(train, batch_size, shuffle=True, seed=seed, augment=augment),
            DeviceLoader(val, batch_size, shuffle=False))
