"""CPU: the host rules of the device input pipeline (device_data.resample_tables / nearest_table / rotation_words, executed by input_ref.py)
against PIL, byte for byte, on the case list the GPU test runs; the properties of Augment.draw and of the DeviceLoader's epoch order; and
the C ABI of the new entry points with their host-side validation."""
import ctypes
import importlib
import os

import numpy as np
import pytest

import input_ref as R
from conftest import ROOT

DD = R.DD
ENTRIES = ("runet_resample8_rows", "runet_resample8_cols", "runet_gather2d_u8", "runet_batch_gray_sums", "runet_batch_assemble")
P16 = ctypes.c_void_p(4096)          # a non-null, 16-byte aligned "pointer": validation must fail before anything would touch it
ODD = ctypes.c_void_p(4097)


def _lib():
    return importlib.import_module("eusipco-2026-robust-unet_amd._lib")


# --------------------------------------------------------------------------- resampling
@pytest.mark.parametrize("case", R.RESIZE_SHAPES + [((64, 64), (64, 64))], ids=R.shape_id)
@pytest.mark.parametrize("c", [3, 1])
@pytest.mark.parametrize("filter", ["lanczos", "bilinear"])
def test_resize_rule_equals_pil(case, c, filter):
    (h, w), (oh, ow) = case
    a = R.content(h, w, c)
    assert np.array_equal(R.resize_ref(a, (ow, oh), filter), R.pil_resize(a, (ow, oh), filter))


@pytest.mark.parametrize("case", R.RESIZE_SHAPES, ids=R.shape_id)
def test_nearest_rule_equals_pil(case):
    (h, w), (oh, ow) = case
    m = R.mask_content(h, w)
    assert np.array_equal(R.nearest_ref(m, (ow, oh)), R.pil_resize(m, (ow, oh), "nearest"))


def test_case_list_covers_what_it_names():
    for (h, w), (oh, ow) in R.UPSCALING:
        ex = [0, 0]
        R.resize_ref(R.content(h, w, 3), (ow, oh), "lanczos", ex)
        assert ex[0] < 0 and ex[1] > 255, ((h, w), ex)                               # values on both sides exist in front of the clamp
        assert ((h, w), (oh, ow)) in R.RESIZE_SHAPES
    bounds, coeffs = DD.resample_tables(307, 64, "lanczos")
    assert bounds[:, 1].max() == 29 and coeffs.shape[1] >= 29
    assert DD.resample_tables(211, 64, "lanczos")[0][:, 1].max() < 29
    a = R.content(33, 33, 3, seed=5)
    rot = R.rotate_ref(np.full_like(a, 255), 10.0)
    assert rot[0, 0].max() == 0 and rot[-1, -1].max() == 0 and rot[16, 16].min() == 255      # an angle-10 case fills corners
    assert 10.0 in R.ANGLES and -10.0 in R.ANGLES and 0.0 in R.ANGLES and 3.7 in R.ANGLES
    for size in (16, 33):
        cases = R.augment_cases(size)
        assert {c["order"] for c in cases} == set(DD.ORDERS)
        assert {c["flip"] for c in cases} == {0, 1}
        assert set(R.ANGLES) <= {c["angle"] for c in cases}
        for v in (0.9, 1.0, 1.1):
            assert any(np.all(c["factors"] == np.float32(v)) for c in cases)
        assert {c["index"] for c in cases} == set(range(7))
    imgs, _ = R.cache_content(16)
    for ch in range(3):
        assert np.unique(imgs[0][..., ch]).size == 256


def test_tables_are_cached_and_well_formed():
    b, k = DD.resample_tables(211, 64, "lanczos")
    assert DD.resample_tables(211, 64, "lanczos")[0] is b
    assert b.dtype == np.int32 and k.dtype == np.int32 and b.shape == (64, 2) and k.shape[0] == 64
    assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= 211).all() and (b[:, 1] <= k.shape[1]).all()
    assert (np.abs(k.sum(axis=1) - (1 << 22)) <= k.shape[1]).all()                   # the weights of an output sum to one, up to rounding
    t = DD.nearest_table(7, 64)
    assert t.dtype == np.int32 and t.min() == 0 and t.max() == 6 and (np.diff(t) >= 0).all()
    with pytest.raises(ValueError):
        DD.resample_tables(0, 4)
    with pytest.raises(ValueError):
        DD.resample_tables(4, 4, "bicubic")
    with pytest.raises(ValueError):
        DD.rotation_words(8, 8, 90)
    assert DD.rotation_words(8, 8, 0).tolist() == [65536, 0, 32768, 0, 65536, 32768]


# --------------------------------------------------------------------------- enhancers, rotation, the chain
@pytest.mark.parametrize("which", [DD.BRIGHTNESS, DD.CONTRAST, DD.SATURATION])
@pytest.mark.parametrize("f", [0.9, 1.0, 1.1, 0.0, 0.37, 1.9, -0.5, 2.5])
def test_enhancer_rule_equals_pil(which, f):
    for seed, (h, w) in enumerate([(16, 16), (33, 21), (5, 7)]):
        a = R.content(h, w, 3, seed=seed)
        want = np.asarray(R.ENHANCERS[which](R.to_pil(a)).enhance(float(np.float32(f))), dtype=np.uint8)
        got, _ = R.enhance_ref(a, which, np.float32(f))
        assert np.array_equal(got, want), (which, f, h, w)


@pytest.mark.parametrize("angle", list(R.ANGLES) + [-3.7, 45.0, 89.5, 123.4, -0.01])
def test_rotation_rule_equals_pil(angle):
    from PIL import Image
    for h, w in [(16, 16), (33, 33), (21, 40), (1, 1)]:
        a = R.content(h, w, 3, seed=2)
        want = np.asarray(R.to_pil(a).rotate(angle, Image.NEAREST, expand=False, fillcolor=0), dtype=np.uint8)
        assert np.array_equal(R.rotate_ref(a, angle), want), (angle, h, w)


@pytest.mark.parametrize("size", [16, 33])
@pytest.mark.parametrize("masks", ["follow", "fixed"])
def test_augmentation_chain_equals_pil_in_all_six_orders(size, masks):
    imgs, msk = R.cache_content(size)
    for c in R.augment_cases(size):
        i = c["index"]
        got = R.augment_ref(imgs[i], msk[i], c["flip"], c["angle"], c["factors"], c["order"], masks)
        want = R.pil_augment(imgs[i], msk[i], c["flip"], c["angle"], c["factors"], c["order"], masks)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], c


# --------------------------------------------------------------------------- Augment.draw, the loader's order
def test_augment_draw_properties():
    aug = DD.Augment()
    p = aug.draw(600, seed=5, epoch=2)
    assert p["flip"].dtype == np.int32 and set(p["flip"].tolist()) == {0, 1} and 200 < p["flip"].sum() < 400
    assert p["angle"].shape == (600,) and (np.abs(p["angle"]) <= 10.0).all() and p["angle"].min() < -8 and p["angle"].max() > 8
    assert p["factors"].dtype == np.float32 and p["factors"].shape == (600, 3)
    assert (p["factors"] >= np.float32(0.9)).all() and (p["factors"] <= np.float32(1.1)).all()
    assert set(p["order"].tolist()) == {DD.pack_order(o) for o in DD.ORDERS} and len(set(p["order"].tolist())) == 6
    q = aug.draw(600, seed=5, epoch=2)
    assert all(np.array_equal(p[k], q[k]) for k in p)
    other = aug.draw(600, seed=5, epoch=3)
    assert not np.array_equal(p["angle"], other["angle"]) and not np.array_equal(p["order"], other["order"])
    assert not np.array_equal(p["angle"], aug.draw(600, seed=6, epoch=2)["angle"])
    off = DD.Augment(flip_p=0.0, degrees=0.0, brightness=0.0, contrast=0.0, saturation=0.0).draw(20, 1, 1)
    assert not off["flip"].any() and not off["angle"].any() and (off["factors"] == 1).all()
    g = DD.geometry_words(32, p["flip"][:5], p["angle"][:5], p["order"][:5])
    assert g.dtype == np.int32 and g.shape == (5, 8) and np.array_equal(g[0, 1:7], DD.rotation_words(32, 32, p["angle"][0]))
    with pytest.raises(ValueError):
        DD.Augment(degrees=90)
    with pytest.raises(ValueError):
        DD.Augment(masks="sometimes")


class _FakeDataset:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def test_loader_epoch_order_properties():
    n = 23
    ds = _FakeDataset(n)
    for epoch in range(3):
        full = DD.DeviceLoader(ds, 4, shuffle=True, seed=9).indices(epoch)
        assert sorted(full.tolist()) == list(range(n))                                # every index exactly once per epoch
        a = DD.DeviceLoader(ds, 4, shuffle=True, seed=9, rank=0, world=2).indices(epoch)
        b = DD.DeviceLoader(ds, 4, shuffle=True, seed=9, rank=1, world=2).indices(epoch)
        assert not set(a.tolist()) & set(b.tolist()) and sorted(a.tolist() + b.tolist()) == list(range(n))
    ld = DD.DeviceLoader(ds, 4, shuffle=True, seed=9)
    assert not np.array_equal(ld.indices(0), ld.indices(1)) and np.array_equal(ld.indices(1), ld.indices(1))
    assert not np.array_equal(ld.indices(0), DD.DeviceLoader(ds, 4, shuffle=True, seed=10).indices(0))
    assert DD.DeviceLoader(ds, 4).indices(5).tolist() == list(range(n))              # unshuffled
    assert len(DD.DeviceLoader(ds, 4)) == 6 and len(DD.DeviceLoader(ds, 4, drop_last=True)) == 5
    assert DD.batch_slices(23, 4) == [(0, 4), (4, 8), (8, 12), (12, 16), (16, 20), (20, 23)]
    assert DD.batch_slices(23, 4, drop_last=True)[-1] == (16, 20) and DD.batch_slices(3, 4, drop_last=True) == []
    assert len(DD.DeviceLoader(ds, 4, rank=1, world=2)) == 3 and len(DD.DeviceLoader(ds, 4, rank=0, world=2)) == 3
    with pytest.raises(ValueError):
        DD.DeviceLoader(ds, 4, rank=2, world=2)


# --------------------------------------------------------------------------- the C ABI
def test_new_entry_points_are_declared_exported_and_cite_the_reference():
    lm = _lib()
    protos = lm.parse_header(os.path.join(ROOT, "include", "runet_hip.h"))
    raw = ctypes.CDLL(lm.LIB_PATH)
    for name in ENTRIES:
        assert name in protos, f"{name} not declared in include/runet_hip.h"
        assert hasattr(raw, name), f"{name} not exported by librunet_hip.so"
    assert len(protos["runet_resample8_rows"][1]) == 10 and len(protos["runet_resample8_cols"][1]) == 10
    assert len(protos["runet_gather2d_u8"][1]) == 9 and len(protos["runet_batch_gray_sums"][1]) == 9
    assert len(protos["runet_batch_assemble"][1]) == 19
    header = open(os.path.join(ROOT, "include", "runet_hip.h")).read()
    assert "Main_Final.py:40-54" in header and "train_water_segmentation.py:313-321" in header
    pkg = importlib.import_module("eusipco-2026-robust-unet_amd")
    for name in ("DeviceCoastalDataset", "DeviceLoader", "Augment", "prepare_device_dataset", "resize_pil_device", "resample_tables",
                 "nearest_table", "rotation_words"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(DD, name)


def test_host_side_validation_without_a_gpu():
    lib = _lib().lib
    err = lib.runet_last_error
    for fn in (lib.runet_resample8_rows, lib.runet_resample8_cols):
        assert fn(None, 8, 8, 3, P16, P16, 7, P16, 4, None) != 0 and b"null pointer" in err()
        assert fn(P16, 8, 8, 3, None, P16, 7, P16, 4, None) != 0 and b"null pointer" in err()
        assert fn(P16, 8, 8, 3, P16, None, 7, P16, 4, None) != 0 and b"null pointer" in err()
        assert fn(P16, 8, 8, 3, P16, P16, 7, None, 4, None) != 0 and b"null pointer" in err()
        assert fn(P16, 0, 8, 3, P16, P16, 7, P16, 4, None) != 0 and b"bad shape" in err()
        assert fn(P16, 8, 8, 2, P16, P16, 7, P16, 4, None) != 0 and b"bad shape" in err()
        assert fn(P16, 8, 8, 3, P16, P16, 7, P16, 0, None) != 0 and b"bad shape" in err()
        assert fn(P16, 8, 8, 3, P16, P16, 0, P16, 4, None) != 0 and b"ksize" in err()
        assert fn(P16, 8, 8, 3, P16, P16, 256, P16, 4, None) != 0 and b"ksize" in err()
        assert fn(P16, 8, 8, 3, ODD, P16, 7, P16, 4, None) != 0 and b"aligned" in err()
        assert fn(P16, 8, 8, 3, P16, ctypes.c_void_p(4098), 7, P16, 4, None) != 0 and b"aligned" in err()
        assert fn(P16, 32768, 32768, 3, P16, P16, 7, P16, 4, None) != 0 and b"2^31" in err()
    assert lib.runet_resample8_cols(P16, 8, 8, 3, P16, P16, 7, P16, 65536, None) != 0 and b"65535" in err()

    g = lib.runet_gather2d_u8
    assert g(None, 8, 8, P16, P16, P16, 4, 4, None) != 0 and b"null pointer" in err()
    assert g(P16, 8, 8, None, P16, P16, 4, 4, None) != 0 and b"null pointer" in err()
    assert g(P16, 8, 8, P16, None, P16, 4, 4, None) != 0 and b"null pointer" in err()
    assert g(P16, 8, 8, P16, P16, None, 4, 4, None) != 0 and b"null pointer" in err()
    assert g(P16, 8, 0, P16, P16, P16, 4, 4, None) != 0 and b"bad shape" in err()
    assert g(P16, 8, 8, P16, P16, P16, 4, -1, None) != 0 and b"bad shape" in err()
    assert g(P16, 65536, 32768, P16, P16, P16, 4, 4, None) != 0 and b"2^31" in err()
    assert g(P16, 8, 8, P16, ODD, P16, 4, 4, None) != 0 and b"aligned" in err()
    assert g(P16, 8, 8, P16, P16, ODD, 4, 4, None) != 0 and b"aligned" in err()

    s = lib.runet_batch_gray_sums
    assert s(None, 7, 16, P16, 5, P16, P16, P16, None) != 0 and b"null pointer" in err()
    assert s(P16, 7, 16, None, 5, P16, P16, P16, None) != 0 and b"null pointer" in err()
    assert s(P16, 7, 16, P16, 5, None, P16, P16, None) != 0 and b"null pointer" in err()
    assert s(P16, 7, 16, P16, 5, P16, None, P16, None) != 0 and b"null pointer" in err()
    assert s(P16, 7, 16, P16, 5, P16, P16, None, None) != 0 and b"null pointer" in err()
    assert s(P16, 0, 16, P16, 5, P16, P16, P16, None) != 0 and b"bad shape" in err()
    assert s(P16, 7, 0, P16, 5, P16, P16, P16, None) != 0 and b"bad shape" in err()
    assert s(P16, 7, 16, P16, 0, P16, P16, P16, None) != 0 and b"bad shape" in err()
    assert s(P16, 7, 16, P16, 65536, P16, P16, P16, None) != 0 and b"bad shape" in err()
    assert s(P16, 7, 4097, P16, 5, P16, P16, P16, None) != 0 and b"4096" in err()
    assert s(P16, 7, 16, P16, 5, P16, P16, ctypes.c_void_p(4100), None) != 0 and b"aligned" in err()
    assert s(P16, 7, 16, ODD, 5, P16, P16, P16, None) != 0 and b"aligned" in err()

    def asm(images=P16, masks=P16, m=7, size=16, index=P16, b=5, std=(0.229, 0.224, 0.225), geom=None, factors=None, sums=None, mode=1,
            oi=P16, om=P16):
        return lib.runet_batch_assemble(images, masks, m, size, index, b, 0.485, 0.456, 0.406, std[0], std[1], std[2], geom, factors, sums, mode,
                                        oi, om, None)
    for k in ("images", "masks", "index", "oi", "om"):
        assert asm(**{k: None}) != 0 and b"null pointer" in err(), k
    assert asm(m=0) != 0 and b"bad shape" in err()
    assert asm(size=0) != 0 and b"bad shape" in err()
    assert asm(b=0) != 0 and b"bad shape" in err()
    assert asm(size=4097) != 0 and b"4096" in err()
    assert asm(geom=P16) != 0 and b"come together" in err()
    assert asm(geom=P16, factors=P16) != 0 and b"come together" in err()
    assert asm(sums=P16) != 0 and b"come together" in err()
    assert asm(mode=2) != 0 and b"mask_mode" in err()
    assert asm(std=(0.229, 0.0, 0.225)) != 0 and b"std" in err()
    assert asm(oi=ctypes.c_void_p(4104)) != 0 and b"aligned" in err()
    assert asm(om=ctypes.c_void_p(4100)) != 0 and b"aligned" in err()
    assert asm(masks=ODD) != 0 and b"aligned" in err()
    assert asm(geom=P16, factors=P16, sums=ctypes.c_void_p(4100)) != 0 and b"aligned" in err()

    import torch
    with pytest.raises(ValueError):
        DD.resize_pil_device(torch.zeros((4, 4, 3), dtype=torch.uint8), (2, 2))      # a host tensor: PIL is the function for it
    with pytest.raises(ValueError):
        DD.DeviceCoastalDataset([], [], image_size=(32, 16))
    with pytest.raises(ValueError):
        DD.DeviceCoastalDataset([], [], image_size=(32, 32), device="cpu")
