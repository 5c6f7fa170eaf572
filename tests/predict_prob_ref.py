"""TEST INFRASTRUCTURE - CPU restatement of the probability route of the prediction path (Main_Final.py:521: `pred > threshold`): a Robust
U-Net trained for a few Adam steps on the CPU oracle, its eval forward, the threshold rule stitched by coastline_ref.stitch_cores, and the
scenes / sizes the CPU and the GPU tests share."""
import importlib

import numpy as np
import torch

import coastline_ref as R

BASE = 16                       # RobustUNet(3, 1, 16)
INPUT_SIZE = 64                 # the reference-size path of the end-to-end tests
SCENE = (100, 156, 21)          # h, w, seed of the end-to-end scene (tests 4-6 of tests/test_gpu_predict_prob.py)
TILE, HALO = 64, 16             # the tiled path: cores of 32, 4 x 5 = 20 tiles on SCENE
NEAR = 2e-3                     # |p - 0.5| within twice the project's probability tolerance 1e-3 (tests/test_gpu_model.py)
NEAR_CAP = 1e-3                 # at most 0.1 % of the pixels may be that near, on the CPU probabilities alone
SPECIALS = (float("nan"), float("inf"), float("-inf"), 0.0, 1.0, -0.0)


def _oracle():
    return importlib.import_module("oracle.robust_unet_ref")


def train_robust_unet(steps=25, size=64, n=2, seed=0, lr=1e-3, base=BASE):
    """A few Adam steps of oracle.robust_unet_ref on the CPU on n seeded scenes -> state dict (reference keys) that separates water from land."""
    ru = _oracle()
    st = ru.init_state(3, 1, base, seed=seed, perturb_bn=False)
    names = ru.param_names(3, 1, base)
    pairs = [R.synthetic_scene(size, size, seed * 100 + i) for i in range(n)]
    x = torch.stack([R.normalize_u8(s) for s, _ in pairs])
    y = torch.stack([torch.from_numpy(m.astype(np.float32))[None] for _, m in pairs])
    for k in names:
        st[k].requires_grad_(True)
    opt = torch.optim.Adam([st[k] for k in names], lr=lr)
    for _ in range(steps):
        opt.zero_grad()
        ru.bce_mean(ru.forward(st, x, True, None)[0], y).backward()
        opt.step()
    return {k: v.detach().clone() for k, v in st.items()}


def cpu_prob(state, x_nchw):
    """eval forward of the oracle -> float32 [n, 1, H, W] probabilities"""
    with torch.no_grad():
        return _oracle().forward({k: v.clone() for k, v in state.items()}, x_nchw, False, None)[0]


def threshold_stitch_ref(prob, origins, halo, h, w, thr=0.5, fill=255, soft_fill=0.0):
    """prob [n, T, T] float32 -> (uint8 [h, w] mask of `prob > float32(thr)`, float32 [h, w] soft map), both stitched from the tiles' cores;
    pixels no core covers keep `fill` (mask) / `soft_fill` (soft map)."""
    prob = np.asarray(prob, dtype=np.float32)
    mask = R.stitch_cores((prob > np.float32(thr)).astype(np.uint8), origins, halo, h, w, fill)
    return mask, R.stitch_cores(prob, origins, halo, h, w, np.float32(soft_fill))


def special_probs(shape, thr, seed):
    """uniform [0, 1) float32 probabilities seeded with the values at which a threshold rule can go wrong: the fp32 threshold, its two fp32
    neighbours, NaN, +-Inf, 0, 1 and -0.0; the first entries hold one of each, about 8 % of the rest are drawn from them."""
    rng = np.random.default_rng(seed)
    p = rng.random(shape, dtype=np.float32)
    t = np.float32(thr)
    vals = np.array([t, np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(0))] + list(SPECIALS), dtype=np.float32)
    pick = rng.integers(0, len(vals), shape)
    p = np.where(rng.random(shape) < 0.08, vals[pick], p).astype(np.float32)
    p.reshape(-1)[:len(vals)] = vals
    return p


def near_threshold(prob, thr=0.5):
    """the pixels a correct device forward may put on the other side of the threshold"""
    return np.abs(np.asarray(prob, dtype=np.float64) - thr) <= NEAR


def resized_input(scene_u8, size=INPUT_SIZE):
    """PIL bilinear resize to size x size, the reference's first step -> uint8 [size, size, 3]"""
    from PIL import Image
    d = importlib.import_module("eusipco-2026-robust-unet_amd.data")
    return np.array(d.Resize((size, size))(Image.fromarray(scene_u8)), dtype=np.uint8)


def tiled_input(scene_u8, plan, tile=TILE):
    """the normalised scene cut into NCHW tiles float32 [n, 3, tile, tile], 0 outside the scene"""
    return torch.from_numpy(R.tiles_nhwc4(scene_u8, plan, tile)[..., :3]).permute(0, 3, 1, 2).contiguous()
