"""CPU: the probability route of the prediction path without a device - the reference rule itself (tests/predict_prob_ref.py against
torch.gt), that the near-threshold exemption of the GPU tests is satisfiable by the CPU oracle alone, the host-side validation of the two new
C entry points, and the size refusal of CoastlineExtractor."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import coastline_ref as R
import predict_prob_ref as Q


def _predict():
    return importlib.import_module("eusipco-2026-robust-unet_amd.predict")


@pytest.mark.parametrize("thr", [0.5, 0.3])
@pytest.mark.parametrize("h,w,tile,halo", [(70, 90, 32, 0), (70, 90, 160, 64), (33, 153, 64, 8)])
def test_threshold_stitch_ref_is_torch_gt_stitched(thr, h, w, tile, halo):
    plan = _predict().tile_plan(h, w, tile, halo)
    prob = Q.special_probs((len(plan), tile, tile), thr, seed=h + w + tile)
    t32 = np.float32(thr)
    for v in (t32, np.nextafter(t32, np.float32(1)), np.nextafter(t32, np.float32(0)), np.inf, -np.inf, 0.0, 1.0):
        assert (prob == np.float32(v)).any()
    assert np.isnan(prob).any() and (np.signbit(prob) & (prob == 0)).any()
    mask, soft = Q.threshold_stitch_ref(prob, plan, halo, h, w, thr)
    gt = torch.gt(torch.from_numpy(prob), thr)                               # the scalar is rounded to the tensor's fp32
    assert np.array_equal(mask, R.stitch_cores(gt.numpy().astype(np.uint8), plan, halo, h, w, 255))
    assert int((mask == 255).sum()) == 0 and set(np.unique(mask)) <= {0, 1}
    assert np.array_equal(soft.view(np.uint32), R.stitch_cores(prob.view(np.uint32), plan, halo, h, w, 0))
    # the rule at the values it can go wrong at: NaN -> 0, +Inf -> 1, the threshold itself -> 0, its upper neighbour -> 1
    one = lambda v: int(Q.threshold_stitch_ref(np.full((1, 16, 16), v, np.float32), [(0, 0)], 0, 16, 16, thr)[0][0, 0])
    assert [one(np.nan), one(np.inf), one(-np.inf), one(t32), one(np.nextafter(t32, np.float32(1))), one(np.nextafter(t32, np.float32(0))),
            one(-0.0), one(1.0)] == [0, 1, 0, 0, 1, 0, 0, 1]


@pytest.fixture(scope="module")
def trained():
    torch.manual_seed(0)
    return Q.train_robust_unet()


def _report(what, prob, water_true, resize_to=None):
    near, pred = Q.near_threshold(prob), prob > np.float32(0.5)
    if resize_to is not None:                                                # the maps the GPU test compares: at the scene's own size
        near, pred = R.resize_nearest(near, *resize_to), R.resize_nearest(pred, *resize_to)
    share = float(pred.mean())
    print(f"\n{what}: near-threshold share {float(near.mean()):.2e}, predicted water share {share:.3f} (true {float(water_true.mean()):.3f})")
    assert float(near.mean()) <= Q.NEAR_CAP
    assert 0.02 < share < 0.98


def test_the_exemption_cap_is_satisfiable_by_the_oracle_alone(trained):
    """the scenes, tiles and input size of tests/test_gpu_predict_prob.py (tests 4-6), on the CPU probabilities alone"""
    P = _predict()
    h, w, seed = Q.SCENE
    scene, water = R.synthetic_scene(h, w, seed)
    small = Q.resized_input(scene)
    p = Q.cpu_prob(trained, R.normalize_u8(small)[None])[0, 0].numpy()
    _report(f"reference-size path, {Q.INPUT_SIZE}^2 input", p, water, resize_to=(h, w))
    plan = P.tile_plan(h, w, Q.TILE, Q.HALO)
    assert len(plan) == 20
    x = Q.tiled_input(scene, plan)
    pt = torch.cat([Q.cpu_prob(trained, x[i:i + 4]) for i in range(0, len(plan), 4)])[:, 0].numpy()
    _, soft = Q.threshold_stitch_ref(pt, plan, Q.HALO, h, w)
    _report(f"tiled path, tile {Q.TILE} halo {Q.HALO}", soft, water)


def test_host_validation_of_the_new_entry_points_without_a_device():
    lib = importlib.import_module("eusipco-2026-robust-unet_amd._lib").lib
    p = ctypes.c_void_p(64)                                                   # never dereferenced: every call below is refused on the host
    ok = dict(n_tiles=1, tile=16, halo=0, h=8, w=8)

    def stitch(prob=p, origins=p, mask=p, soft=None, thr=0.5, **kw):
        a = {**ok, **kw}
        return lib.runet_threshold_stitch(prob, a["n_tiles"], a["tile"], origins, a["halo"], thr, mask, soft, a["h"], a["w"], None)

    for kw in (dict(prob=None), dict(origins=None), dict(mask=None)):
        assert stitch(**kw) != 0 and b"null pointer" in lib.runet_last_error()
    for kw in (dict(tile=0), dict(tile=-16)):
        assert stitch(**kw) != 0 and b"tile must be positive" in lib.runet_last_error()
    for kw in (dict(halo=8), dict(halo=9), dict(halo=-1), dict(tile=160, halo=80)):
        assert stitch(**kw) != 0 and b"2 * halo must be smaller than the tile" in lib.runet_last_error()
    assert stitch(h=65536, w=32768) != 0 and b"h * w" in lib.runet_last_error()
    assert stitch(h=0) != 0 and b"bad scene shape" in lib.runet_last_error()
    assert stitch(n_tiles=0) != 0 and b"bad tile count" in lib.runet_last_error()
    assert b"runet_threshold_stitch" in lib.runet_last_error()

    def tiles(scene=p, origins=p, out=p, h=8, w=8, stride=24, n=1, tile=16, std=(0.229, 0.224, 0.225)):
        return lib.runet_scene_to_tiles_nchw(scene, h, w, stride, origins, n, tile, 0.485, 0.456, 0.406, *std, out, None)

    for kw in (dict(scene=None), dict(origins=None), dict(out=None)):
        assert tiles(**kw) != 0 and b"null pointer" in lib.runet_last_error()
    assert tiles(tile=0) != 0 and b"bad tile count / size" in lib.runet_last_error()
    assert tiles(stride=23) != 0 and b"bad scene shape" in lib.runet_last_error()
    assert tiles(std=(0.229, 0.0, 0.225)) != 0 and b"zero std" in lib.runet_last_error()
    assert tiles(out=ctypes.c_void_p(66)) != 0 and b"aligned" in lib.runet_last_error()


def test_the_extractor_refuses_sizes_and_models_before_any_device_work(pkg):
    """every refusal below comes from the constructor on the CPU: nothing is allocated on a device, nothing launched"""
    torch.manual_seed(0)
    with pytest.raises(ValueError, match="multiples of 32"):
        pkg.CoastlineExtractor(model=pkg.SegFormerLite(), device="cpu", input_size=80)
    with pytest.raises(ValueError, match="multiples of 16"):
        pkg.CoastlineExtractor(model=pkg.RobustUNet(3, 1, 16), device="cpu", input_size=72)
    with pytest.raises(ValueError, match="multiples of 16"):
        pkg.CoastlineExtractor(model=pkg.DeepLabV3Plus(), device="cpu", input_size=40)
    with pytest.raises(ValueError):
        pkg.CoastlineExtractor(model=pkg.RobustUNet(3, 1, 16), device="cpu", input_size=0)
    with pytest.raises(TypeError):
        pkg.CoastlineExtractor(model=torch.nn.Conv2d(3, 1, 1), device="cpu", input_size=64)
    with pytest.raises(TypeError):
        pkg.CoastlineExtractor(model=object(), device="cpu", input_size=64)
    ex = pkg.CoastlineExtractor(model=pkg.RobustUNet(3, 1, 16), device="cpu", input_size=64, threshold=0.3)
    assert ex.prob and ex.threshold == 0.3 and not ex.model.training
    with pytest.raises(ValueError, match="multiples of 16"):
        ex.predict_scene(np.zeros((8, 8, 3), np.uint8), tile=40, halo=4)
    with pytest.raises(ValueError, match="multiples of 16"):
        ex.extract_coastline_from_image(np.zeros((8, 8, 3), np.uint8), tiled=True, tile=40, halo=4)
    unet = pkg.CoastlineExtractor(device="cpu", input_size=64)
    assert not unet.prob
    with pytest.raises(ValueError, match="logits"):
        unet.predict_scene(np.zeros((8, 8, 3), np.uint8), tile=64, halo=0, return_prob=True)


def test_every_probability_model_answers_check_input_on_a_shape_only_tensor(pkg):
    P = _predict()
    for name, mod in P.PROB_MODELS.items():
        cls = getattr(importlib.import_module(f"eusipco-2026-robust-unet_amd.{mod}"), name)
        assert getattr(pkg, name) is cls
        net = (cls(3, 1, 16) if name == "RobustUNet" else cls()).eval()
        assert P._is_prob_model(net)
        net._check_input(torch.empty((2, 3, 64, 96), device="meta"))
        with pytest.raises(ValueError, match="multiples of"):
            net._check_input(torch.empty((2, 3, 64, 100), device="meta"))
    assert not P._is_prob_model(pkg.UNet(3, 2))
