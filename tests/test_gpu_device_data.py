"""GPU: the device input pipeline (device_data.py, csrc/input_pipeline.hip) against PIL on the host, exact everywhere (byte equality,
torch.equal): the two resampling passes and the mask gather on the case list of input_ref.py, the batch assembly with and without the
augmentation against the PIL chain, and a small Labelme dataset end to end against CoastalDataset."""
import importlib
import os
import shutil

import numpy as np
import pytest
import torch
from PIL import Image

import input_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DD = R.DD
INDEX = [6, 3, 3, 1, 0]              # repeated and descending
_WANT = {}


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _at_odd_address(a):
    """the same bytes on the device, starting one byte past an allocation's (aligned) base"""
    buf = torch.empty(a.size + 1, dtype=torch.uint8, device=DEV)
    view = buf[1:].view(a.shape)
    view.copy_(_dev(a))
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    return view


@pytest.mark.parametrize("case", R.RESIZE_SHAPES, ids=R.shape_id)
@pytest.mark.parametrize("c", [3, 1])
@pytest.mark.parametrize("filter", ["lanczos", "bilinear"])
def test_resample_equals_pil(case, c, filter):
    (h, w), (oh, ow) = case
    a = R.content(h, w, c)
    got = DD.resize_pil_device(_dev(a), (ow, oh), filter)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (oh, ow, c)
    assert np.array_equal(got.cpu().numpy(), R.pil_resize(a, (ow, oh), filter))


@pytest.mark.parametrize("case", [R.RESIZE_SHAPES[0], R.RESIZE_SHAPES[2], R.RESIZE_SHAPES[3], R.RESIZE_SHAPES[4]], ids=R.shape_id)
@pytest.mark.parametrize("c", [3, 1])
def test_resample_of_a_source_at_an_odd_byte_address(case, c):
    (h, w), (oh, ow) = case
    a = R.content(h, w, c)
    got = DD.resize_pil_device(_at_odd_address(a), (ow, oh), "lanczos")
    assert np.array_equal(got.cpu().numpy(), R.pil_resize(a, (ow, oh), "lanczos"))


def test_resample_of_a_plane_without_channel_axis():
    a = R.content(37, 53, 1)[:, :, 0]
    got = DD.resize_pil_device(_dev(a), (16, 16), "lanczos")
    assert tuple(got.shape) == (16, 16) and np.array_equal(got.cpu().numpy(), R.pil_resize(a, (16, 16), "lanczos"))


@pytest.mark.parametrize("case", R.RESIZE_SHAPES, ids=R.shape_id)
def test_mask_gather_equals_pil_nearest(case):
    (h, w), (oh, ow) = case
    m = R.mask_content(h, w)
    got = DD.resize_pil_device(_dev(m), (ow, oh), "nearest")
    assert np.array_equal(got.cpu().numpy(), R.pil_resize(m, (ow, oh), "nearest"))
    got = DD.resize_pil_device(_at_odd_address(m), (ow, oh), "nearest")
    assert np.array_equal(got.cpu().numpy(), R.pil_resize(m, (ow, oh), "nearest"))


@pytest.mark.parametrize("size", [16, 33])
def test_assemble_without_augmentation(size):
    imgs, msk = R.cache_content(size)
    if size == 16:
        assert 0 in INDEX and all(np.unique(imgs[0][..., ch]).size == 256 for ch in range(3))     # the whole domain of the normalisation
    out_i, out_m, sums = DD.assemble_batch(_dev(imgs), _dev(msk), _dev(np.array(INDEX, np.int32)))
    assert sums is None and out_i.dtype == torch.float32 and tuple(out_i.shape) == (5, 3, size, size) and tuple(out_m.shape) == (5, 1, size, size)
    u8 = torch.from_numpy(imgs[INDEX])
    mean = torch.tensor(R.DATA.IMAGENET_MEAN, dtype=torch.float32).view(1, 3, 1, 1)
    std = torch.tensor(R.DATA.IMAGENET_STD, dtype=torch.float32).view(1, 3, 1, 1)
    want = (u8.permute(0, 3, 1, 2).float() / 255 - mean) / std
    assert torch.equal(out_i.cpu(), want)
    assert torch.equal(out_m.cpu(), torch.from_numpy(msk[INDEX]).float().unsqueeze(1))


def _want_augmented(size, masks):
    """the PIL chain of every case, computed once per (size, mask mode)"""
    key = (size, masks)
    if key not in _WANT:
        imgs, msk = R.cache_content(size)
        res = [R.pil_augment(imgs[c["index"]], msk[c["index"]], c["flip"], c["angle"], c["factors"], c["order"], masks)
               for c in R.augment_cases(size)]
        _WANT[key] = (R.normalize_ref(np.stack([r[0] for r in res])), torch.from_numpy(np.stack([r[1] for r in res])).float().unsqueeze(1),
                      [r[2] for r in res])
    return _WANT[key]


@pytest.mark.parametrize("size", [16, 33])
@pytest.mark.parametrize("masks", ["follow", "fixed"])
def test_assemble_with_augmentation_equals_the_pil_chain(size, masks):
    imgs, msk = R.cache_content(size)
    cases = R.augment_cases(size)
    index = _dev(np.array([c["index"] for c in cases], np.int32))
    geom = _dev(DD.geometry_words(size, [c["flip"] for c in cases], [c["angle"] for c in cases], [DD.pack_order(c["order"]) for c in cases]))
    factors = _dev(np.stack([c["factors"] for c in cases]).astype(np.float32))
    di, dm = _dev(imgs), _dev(msk)
    out_i, out_m, sums = DD.assemble_batch(di, dm, index, geom=geom, factors=factors, mask_mode=masks)
    want_i, want_m, want_mean = _want_augmented(size, masks)
    got_mean = [int(s / (size * size) + 0.5) for s in sums.cpu().tolist()]
    assert got_mean == want_mean                                                     # ImageStat's mean of the PIL intermediate
    bad = [k for k in range(len(cases)) if not torch.equal(out_i[k].cpu(), want_i[k])]
    assert not bad, [cases[k] for k in bad[:3]]
    assert torch.equal(out_m.cpu(), want_m)
    again = DD.assemble_batch(di, dm, index, geom=geom, factors=factors, mask_mode=masks)
    assert torch.equal(again[0], out_i) and torch.equal(again[1], out_m) and torch.equal(again[2], sums)      # byte-identical repeats


def test_assemble_with_several_blocks_per_sample_on_the_16_byte_path():
    size = 64                                                # 4096 pixels: four blocks of 256 lanes x 4 pixels per sample
    imgs, msk = R.cache_content(size)
    cases = R.augment_cases(size)[:8]
    index = _dev(np.array([c["index"] for c in cases], np.int32))
    di, dm = _dev(imgs), _dev(msk)
    out_i, out_m, _ = DD.assemble_batch(di, dm, index)
    assert torch.equal(out_i.cpu(), R.normalize_ref(imgs[[c["index"] for c in cases]]))
    assert torch.equal(out_m.cpu(), torch.from_numpy(msk[[c["index"] for c in cases]]).float().unsqueeze(1))
    geom = _dev(DD.geometry_words(size, [c["flip"] for c in cases], [c["angle"] for c in cases], [DD.pack_order(c["order"]) for c in cases]))
    factors = _dev(np.stack([c["factors"] for c in cases]).astype(np.float32))
    out_i, out_m, sums = DD.assemble_batch(di, dm, index, geom=geom, factors=factors, mask_mode="follow")
    for k, c in enumerate(cases):
        a, m, mean = R.pil_augment(imgs[c["index"]], msk[c["index"]], c["flip"], c["angle"], c["factors"], c["order"], "follow")
        assert int(sums[k].item() / (size * size) + 0.5) == mean
        assert torch.equal(out_i[k].cpu(), R.normalize_ref(a)) and torch.equal(out_m[k, 0].cpu(), torch.from_numpy(m).float()), c


def _write_dataset(root):
    """six files: four PNGs of different sizes, one unreadable image, one image paired with the invalid JSON fixture"""
    idir, ldir = os.path.join(root, "images"), os.path.join(root, "labels")
    os.makedirs(idir), os.makedirs(ldir)
    rng = np.random.default_rng(11)
    plan = [("a", (40, 30), "float_coords.json"), ("b", (64, 64), "two_labels.json"), ("c", (100, 75), "out_of_bounds.json"),
            ("d", (17, 90), "too_few_points.json"), ("e", None, "no_shapes.json"), ("f", (48, 52), "bad_json.json")]
    for name, wh, label in plan:
        path = os.path.join(idir, name + ".png")
        if wh is None:
            with open(path, "wb") as f:
                f.write(b"this is not a png")
        else:
            Image.fromarray(rng.integers(0, 256, (wh[1], wh[0], 3), dtype=np.uint8)).save(path)
        shutil.copy(os.path.join(GOLDEN, "labelme", label), os.path.join(ldir, name + ".json"))
    return idir, ldir


def test_dataset_end_to_end_equals_coastal_dataset(tmp_path):
    idir, ldir = _write_dataset(str(tmp_path))
    names = sorted(os.listdir(idir))
    ipaths = [os.path.join(idir, n) for n in names]
    lpaths = [os.path.join(ldir, os.path.splitext(n)[0] + ".json") for n in names]
    size = (32, 32)
    tf = R.DATA.Compose([R.DATA.Resize(size), R.DATA.ToTensor(), R.DATA.Normalize(R.DATA.IMAGENET_MEAN, R.DATA.IMAGENET_STD)])
    host = R.DATA.CoastalDataset(ipaths, lpaths, transform=tf, image_size=size)
    ds = DD.DeviceCoastalDataset(ipaths, lpaths, image_size=size, device=DEV)
    assert len(ds) == 6 and ds.images.dtype == torch.uint8 and tuple(ds.images.shape) == (6, 32, 32, 3) and tuple(ds.masks.shape) == (6, 32, 32)
    assert ds.masks.sum().item() > 0
    loader = DD.DeviceLoader(ds, 4)
    assert len(loader) == 2
    batches = list(loader)
    assert [b[0].shape[0] for b in batches] == [4, 2] and all(b[0].is_cuda and b[1].is_cuda for b in batches)
    images, masks = torch.cat([b[0] for b in batches]).cpu(), torch.cat([b[1] for b in batches]).cpu()
    for i in range(6):
        want_i, want_m = host[i]
        assert torch.equal(images[i], want_i) and torch.equal(masks[i], want_m), names[i]
    pre = list(R.DATA.DevicePrefetcher(loader, torch.device(DEV)))
    assert len(pre) == 2 and all(torch.equal(p[0], b[0]) and torch.equal(p[1], b[1]) for p, b in zip(pre, batches))

    loaders = DD.prepare_device_dataset(idir, ldir, batch_size=2, image_size=size, device=DEV, augment=DD.Augment(), seed=4)
    train, val = loaders
    assert len(train.dataset) == 4 and len(val.dataset) == 2 and train.augment is not None and val.augment is None and train.shuffle
    vi, vm = next(iter(val))
    assert torch.equal(vi.cpu(), torch.stack([host[4][0], host[5][0]])) and torch.equal(vm.cpu(), torch.stack([host[4][1], host[5][1]]))
    # an augmented, shuffled epoch: every sample is the PIL chain of the cached bytes under the loader's own parameters
    idx, p = train.indices(0), train.parameters(0)
    cached_i, cached_m = train.dataset.images.cpu().numpy(), train.dataset.masks.cpu().numpy()
    got = list(train)
    gi, gm = torch.cat([b[0] for b in got]).cpu(), torch.cat([b[1] for b in got]).cpu()
    assert sorted(idx.tolist()) == [0, 1, 2, 3] and gi.shape[0] == 4
    for k, i in enumerate(idx.tolist()):
        order = [(int(p["order"][k]) >> (2 * j)) & 3 for j in range(3)]
        a, m, _ = R.pil_augment(cached_i[i], cached_m[i], int(p["flip"][k]), float(p["angle"][k]), p["factors"][k], order, "follow")
        assert torch.equal(gi[k], R.normalize_ref(a)) and torch.equal(gm[k], torch.from_numpy(m).float().unsqueeze(0)), (k, i)
