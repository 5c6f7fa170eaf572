"""GPU: the prediction path (predict.py, csrc/coastline.hip).  Each kernel alone against the CPU restatement in tests/coastline_ref.py,
BIT-EQUAL (integer results, or one correctly rounded fp32 expression), then CoastlineExtractor end to end with a U-Net trained for a few steps
on the CPU: the water mask may differ from the CPU restatement only at near-tie pixels (bound derived from tests/test_gpu_unet.py's eval-logit
bound, see _compare_water), the coastline mask and the counts are bit-equal to the CPU rule applied to the product's own water mask."""
import importlib

import numpy as np
import pytest
import torch

import coastline_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _predict():
    return importlib.import_module("eusipco-2026-robust-unet_amd.predict")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("h,w,tile", [(37, 53, 16), (37, 53, 32), (64, 64, 64), (5, 3, 16)])
def test_scene_to_tiles_is_totensor_normalize_bit_for_bit(h, w, tile):
    P = _predict()
    rng = np.random.default_rng(h * 1000 + w + tile)
    scene = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    scene[0, 0] = (0, 128, 255)
    origins = np.array([(0, 0), (-5, -7), (h - 3, w - 4), (-tile + 1, 2), (3, -tile), (h, 0), (h // 2, w // 2)], dtype=np.int32)
    got = P.scene_to_tiles(_dev(scene), _dev(origins), tile).cpu().numpy()
    want = R.tiles_nhwc4(scene, origins, tile)
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # a scene that is a column slice of a wider image: the row stride is not 3 * w
    wide = rng.integers(0, 256, (h, w + 9, 3), dtype=np.uint8)
    view = _dev(wide)[:, 4:4 + w]
    assert view.stride(0) == 3 * (w + 9)
    lib = importlib.import_module("eusipco-2026-robust-unet_amd._lib")
    out = torch.empty((len(origins), tile, tile, 4), device=DEV)
    o = _dev(origins)
    lib.check(lib.lib.runet_scene_to_tiles(view.data_ptr(), h, w, view.stride(0), o.data_ptr(), len(origins), tile, *R.MEAN, *R.STD,
                                           out.data_ptr(), None))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), R.tiles_nhwc4(np.ascontiguousarray(wide[:, 4:4 + w]), origins, tile).view(np.uint32))


@pytest.mark.parametrize("classes", [2, 4])
@pytest.mark.parametrize("h,w,tile,halo", [(70, 90, 32, 0), (70, 90, 160, 64), (200, 312, 128, 32), (33, 1531, 64, 8), (16, 16, 16, 0)])
def test_argmax_stitch_equals_torch_argmax(classes, h, w, tile, halo):
    P = _predict()
    plan = P.tile_plan(h, w, tile, halo)
    g = torch.Generator().manual_seed(h + w + tile + classes)
    z = torch.randn((len(plan), tile, tile, 4), generator=g)
    z[1::2] = torch.round(z[1::2] * 2) / 2                       # coarse values: many exact ties, incl. -0.0 against 0.0
    u = torch.rand(z.shape, generator=g)
    z[u < 0.02] = float("nan")
    z[(u >= 0.02) & (u < 0.03)] = float("inf")
    z[(u >= 0.03) & (u < 0.04)] = float("-inf")
    z[0, :2, :4] = torch.tensor([[[1, 1, 1, 1], [float("nan"), 1, 0, 0], [1, float("nan"), 0, 0], [0, 0, float("nan"), float("nan")]],
                                 [[-0.0, 0.0, -1, -1], [0, 0, 0, 1], [5, 5, 7, 7], [float("nan")] * 4]])
    zd = z.to(DEV)
    mask = torch.full((h, w), 255, device=DEV, dtype=torch.uint8)
    P.argmax_stitch(zd, _dev(plan), halo, mask, classes)
    want = R.argmax_stitch(zd.cpu().numpy(), plan, halo, h, w, classes)
    assert int((want == 255).sum()) == 0                         # the plan covers the scene
    assert np.array_equal(mask.cpu().numpy(), want)
    # tiles that do not cover the scene leave the rest of the mask alone
    some = plan[::3]
    mask.fill_(255)
    P.argmax_stitch(zd[::3].contiguous(), _dev(some), halo, mask, classes)
    assert np.array_equal(mask.cpu().numpy(), R.argmax_stitch(zd[::3].cpu().numpy(), some, halo, h, w, classes))


@pytest.mark.parametrize("src,dst", [((512, 512), (1000, 1531)), ((512, 512), (300, 200)), ((4, 4), (10, 10)), ((37, 53), (53, 37)),
                                      ((128, 128), (200, 312)), ((1, 1), (7, 5)), ((9, 17), (1, 1)), ((16, 48), (16, 47))])
def test_resize_nearest_equals_the_index_rule(src, dst):
    P = _predict()
    m = np.random.default_rng(src[0] + dst[1]).integers(0, 256, src, dtype=np.uint8)
    got = P.resize_nearest(_dev(m), dst).cpu().numpy()
    assert got.shape == dst and np.array_equal(got, R.resize_nearest(m, *dst))
    same = _dev(m)
    assert P.resize_nearest(same, src) is same                   # identity size: no launch


def _patterns(h, w, seed):
    rng = np.random.default_rng(seed)
    yield "10%", (rng.random((h, w)) < 0.1).astype(np.uint8)
    yield "50%", (rng.random((h, w)) < 0.5).astype(np.uint8)
    yield "zeros", np.zeros((h, w), np.uint8)
    yield "ones", np.ones((h, w), np.uint8)


@pytest.mark.parametrize("h,w", [(1, 1), (37, 53), (512, 512), (1000, 1531)])
def test_dilate_diff_and_counts_equal_scipy(h, w):
    P = _predict()
    for name, m in _patterns(h, w, h + w):
        md = _dev(m)
        for k in (1, 3, 5, 7, 15, 31):
            coast, counts, dil = P.dilate_diff(md, k, want_dilated=True)
            wc, wd, n_water, n_coast = R.dilate_diff(m, k)
            assert np.array_equal(coast.cpu().numpy(), wc), (name, k)
            assert np.array_equal(dil.cpu().numpy(), wd), (name, k)
            assert counts.cpu().tolist() == [n_water, n_coast], (name, k)
            coast2, counts2, none = P.dilate_diff(md, k)
            assert none is None and torch.equal(coast2, coast) and torch.equal(counts2, counts)
    with pytest.raises(ValueError):
        P.dilate_diff(md, 4)
    with pytest.raises(ValueError):
        P.dilate_diff(md, 33)


def test_dilate_diff_on_a_sparse_mask_with_unaligned_rows():
    """single pixels near every edge and corner of a mask whose rows start at every 16-byte phase (w = 1531), written into a buffer that itself
    starts off the 16-byte grid"""
    P = _predict()
    h, w = 67, 1531
    m = np.zeros((h, w), np.uint8)
    for y, x in [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (33, 255), (33, 256), (31, 700), (32, 701), (40, 1279), (40, 1280), (66, 1530)]:
        m[y, x] = 1
    buf = torch.zeros(h * w + 64, device=DEV, dtype=torch.uint8)
    coast = buf[5:5 + h * w].view(h, w)
    for k in (5, 31):
        _, counts, _ = P.dilate_diff(_dev(m), k, coast=coast)
        wc, _, n_water, n_coast = R.dilate_diff(m, k)
        assert np.array_equal(coast.cpu().numpy(), wc) and counts.cpu().tolist() == [n_water, n_coast]
        assert int(buf[:5].sum()) == 0 and int(buf[5 + h * w:].sum()) == 0       # nothing written outside the mask


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def trained():
    torch.manual_seed(0)
    return R.train_plain_unet(steps=25, size=128, n=2, seed=0, lr=1e-3)


@pytest.fixture(scope="module")
def extractor(pkg, trained):
    net = pkg.UNet(3, 2)
    net.load_state_dict(trained)
    return pkg.CoastlineExtractor(model=net, device=DEV, input_size=128)


def _near_ties(logits):
    """-> (argmax mask uint8, near-tie map bool) of CPU logits [n, 2, H, W].  A pixel is a near-tie when its margin |z1 - z0| is at most twice
    the project's eval-logit bound 1e-3 * max(1, max|z_cpu|) (tests/test_gpu_unet.py): either logit may move by that bound."""
    z = logits.double()
    bound = 2 * 1e-3 * max(1.0, float(z.abs().max()))
    return torch.argmax(logits, dim=1).numpy().astype(np.uint8), ((z[:, 1] - z[:, 0]).abs() <= bound).numpy()


def _compare_water(got, want, near, what):
    frac = float(near.mean())
    diff = got != want
    print(f"\n{what}: near-tie pixels {frac:.2e} of the scene, {int(diff.sum())} pixels differ from the CPU restatement "
          f"({int((diff & ~near).sum())} outside the near-ties), water share {float(want.mean()):.3f}")
    assert frac <= 1e-3, "the CPU logits alone must leave at most 0.1 % of the pixels exempt"
    assert not (diff & ~near).any()
    assert 0.02 < float(want.mean()) < 0.98                      # the trained model separates something: not a constant mask


def _check_post(P, result, k):
    coast, _, n_water, n_coast = R.dilate_diff(result["water_mask"], k)
    assert np.array_equal(result["coastline_mask"], coast)
    assert (result["water_pixels"], result["coastline_pixels"]) == (n_water, n_coast)
    assert result["coastlines"] == P.coastlines_from_mask(coast) and result["coastline_count"] == len(result["coastlines"])
    assert result["water_mask"].dtype == np.uint8 and result["coastline_mask"].dtype == np.uint8


@pytest.mark.parametrize("size,h,w,seed", [(128, 200, 312, 11), (512, 300, 420, 12)])
def test_reference_size_path_end_to_end(pkg, trained, extractor, size, h, w, seed, tmp_path):
    P = _predict()
    data = importlib.import_module("eusipco-2026-robust-unet_amd.data")
    from PIL import Image
    ex = extractor if size == 128 else pkg.CoastlineExtractor(model=extractor.model, device=DEV, input_size=size)
    scene, _ = R.synthetic_scene(h, w, seed)
    small = np.array(data.Resize((size, size))(Image.fromarray(scene)), dtype=np.uint8)
    pred, near = _near_ties(R.cpu_logits(trained, R.normalize_u8(small)[None]))
    want, near = R.resize_nearest(pred[0], h, w), R.resize_nearest(near[0], h, w)
    res = ex.extract_coastline_from_image(scene, dilation_size=5)
    assert res["image_size"] == (w, h) and res["water_mask"].shape == (h, w) and res["dilation_size"] == 5
    _compare_water(res["water_mask"], want, near, f"input {size}^2 -> {h} x {w}")
    _check_post(P, res, 5)
    assert res["coastline_count"] >= 1
    if size == 128:
        path = tmp_path / "scene_a.png"
        Image.fromarray(scene).save(path)
        res2 = ex.extract_coastline_from_image(str(path), output_dir=str(tmp_path / "out"), dilation_size=7)
        assert res2["image_path"] == str(path) and np.array_equal(res2["water_mask"], res["water_mask"])
        _check_post(P, res2, 7)
        assert np.array_equal(np.array(Image.open(tmp_path / "out" / "scene_a_coastline_mask.png")), res2["coastline_mask"] * 255)
        lines, cm = ex.extract_coastline_contours(res["water_mask"], 5)
        lines_t, cm_t = ex.extract_coastline_contours(torch.from_numpy(res["water_mask"]).to(DEV), dilation_kernel_size=5)
        assert np.array_equal(cm, res["coastline_mask"]) and np.array_equal(cm_t, cm) and lines == res["coastlines"] == lines_t
        with pytest.raises(ValueError):
            ex.extract_coastline_from_image(scene, dilation_size=4)


def test_predict_scene_tiled_end_to_end(trained, extractor):
    P = _predict()
    h, w, tile, halo = 200, 312, 128, 32
    scene, _ = R.synthetic_scene(h, w, 13)
    plan = P.tile_plan(h, w, tile, halo)
    x = torch.from_numpy(R.tiles_nhwc4(scene, plan, tile)[..., :3]).permute(0, 3, 1, 2).contiguous()
    logits = torch.cat([R.cpu_logits(trained, x[i:i + 4]) for i in range(0, len(plan), 4)])
    bound = 2 * 1e-3 * max(1.0, float(logits.abs().max()))
    pred = torch.argmax(logits, dim=1).numpy().astype(np.uint8)
    near = ((logits[:, 1].double() - logits[:, 0].double()).abs() <= bound).numpy()
    want = R.stitch_cores(pred, plan, halo, h, w, 255)
    near = R.stitch_cores(near, plan, halo, h, w, False)
    got = extractor.predict_scene(scene, tile=tile, halo=halo, batch=8)
    assert got.dtype == np.uint8 and got.shape == (h, w)
    _compare_water(got, want, near, f"tiled {h} x {w}, tile {tile}, halo {halo}")
    assert np.array_equal(extractor.predict_scene(scene, tile=tile, halo=halo, batch=3), got)        # batching does not change a tile's result
    res = extractor.extract_coastline_from_image(scene, tiled=True, tile=tile, halo=halo, batch=8)
    assert np.array_equal(res["water_mask"], got)
    _check_post(P, res, 5)


def test_prediction_is_deterministic_and_leaves_the_model_alone(extractor):
    scene, _ = R.synthetic_scene(200, 312, 14)
    before = {k: v.detach().clone() for k, v in extractor.model.state_dict().items()}
    a = extractor.extract_coastline_from_image(scene)
    ta = extractor.predict_scene(scene, tile=128, halo=32)
    b = extractor.extract_coastline_from_image(scene)
    tb = extractor.predict_scene(scene, tile=128, halo=32)
    assert np.array_equal(a["water_mask"], b["water_mask"]) and np.array_equal(a["coastline_mask"], b["coastline_mask"])
    assert a["coastlines"] == b["coastlines"] and np.array_equal(ta, tb)
    after = extractor.model.state_dict()
    assert list(before) == list(after)
    for k, v in before.items():
        assert torch.equal(v, after[k]), k
    assert not extractor.model.training


def test_one_tile_without_halo_is_the_model_forward(extractor):
    scene, _ = R.synthetic_scene(128, 128, 15)
    got = extractor.predict_scene(scene, tile=128, halo=0, as_tensor=True)
    with torch.no_grad():
        logits = extractor.model(R.normalize_u8(scene)[None].to(DEV))
    assert torch.equal(got, logits.argmax(1)[0].to(torch.uint8))
    # and the reference-size path at the network's own size is the same mask (no resize either way)
    assert np.array_equal(extractor.extract_coastline_from_image(scene)["water_mask"], got.cpu().numpy())
