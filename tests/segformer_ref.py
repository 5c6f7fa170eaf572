"""CPU restatement of the reference's SegFormer-Lite baseline (TEST INFRASTRUCTURE ONLY -- never imported by the product path).

Functional form, on stock torch CPU fp32 ops over a flat name -> tensor state, of `SegFormerLite` in the reference's
Extended_Baseline_Comparison.py:622-744: four patch embeddings (Conv2d -> BatchNorm2d -> GELU), three stages of `c = c + attn(c); c = c + ffn(c)`
(EfficientSelfAttention with a stride-r key / value reduction, MixFFN with a depthwise 3x3 and GELU), the MLP decoder and the bilinear resize of
the probability map.  Trained there with nn.BCELoss (ModelEvaluator.train_model, :780-837).  Pinned by tests/golden/segformer_*.npz, which
tests/golden/make_golden_segformer.py produced from the reference class itself.

`F` is looked up at module level on every call, so tests/decisions_seq.py's recorder can log (and force) the two ReLU masks of the decoder -
GELU and softmax are smooth, so those masks are the only decisions.
"""
from __future__ import annotations

import importlib
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

from segnet_ref import adam_step, bce_mean  # noqa: F401  (the same nn.BCELoss / Adam(lr, weight_decay) step)

_rng = importlib.import_module("eusipco-2026-robust-unet_amd.portable_rng")
BN_EPS, BN_MOMENTUM = 1e-5, 0.1

EMBED = ((3, 32, 7, 4, 3), (32, 64, 3, 2, 1), (64, 128, 3, 2, 1), (128, 256, 3, 2, 1))       # (cin, cout, kernel, stride, padding)
STAGES = ((32, 1, 8, 128), (64, 2, 4, 256), (128, 4, 2, 512))                                   # (dim, heads, reduction, MixFFN hidden)
# the parameters whose gradient is analytically zero (a constant that a train-mode BatchNorm or a softmax removes): compared with an
# absolute band.  The key half of attn{i}.kv.bias is listed separately (only its first `dim` entries vanish).
ZERO_GRAD = tuple(f"patch_embed{i}.0.bias" for i in range(1, 5)) + ("linear_fuse.0.bias", "head.0.bias") + \
    tuple(f"linear_c{i}.bias" for i in range(1, 5))


def module_spec():
    """(name, shape, kind) in the reference's registration order; conv shapes are [cout, cin / groups, k, k]"""
    s = []
    for i, (cin, cout, k, _, _) in enumerate(EMBED, 1):
        s += [(f"patch_embed{i}.0", (cout, cin, k, k), "conv"), (f"patch_embed{i}.1", cout, "bn")]
    for i, (dim, _, r, hid) in enumerate(STAGES, 1):
        s += [(f"attn{i}.q", (dim, dim, 1, 1), "conv"), (f"attn{i}.kv", (2 * dim, dim, 1, 1), "conv"),
              (f"attn{i}.proj", (dim, dim, 1, 1), "conv"), (f"attn{i}.reduction", (dim, dim, r, r), "conv"),
              (f"ffn{i}.fc1", (hid, dim, 1, 1), "conv"), (f"ffn{i}.dwconv", (hid, 1, 3, 3), "conv"), (f"ffn{i}.fc2", (dim, hid, 1, 1), "conv")]
    s += [("linear_c4", (256, 256, 1, 1), "conv"), ("linear_c3", (256, 128, 1, 1), "conv"), ("linear_c2", (256, 64, 1, 1), "conv"),
          ("linear_c1", (256, 32, 1, 1), "conv"), ("linear_fuse.0", (256, 1024, 1, 1), "conv"), ("linear_fuse.1", 256, "bn"),
          ("head.0", (64, 256, 3, 3), "conv"), ("head.1", 64, "bn"), ("head.3", (1, 64, 1, 1), "conv")]
    return s


def init_state(seed=0, perturb_bn=True):
    """torch's default initialisation DISTRIBUTIONS (the reference class defines no initialiser) from the portable generator: conv weights
    and biases U(-1/sqrt(fan_in), +) with fan_in = cin / groups * k * k (9 for the depthwise convolutions), BatchNorm gamma = 1 / beta = 0
    (jittered when perturb_bn)."""
    st = OrderedDict()
    for name, shape, kind in module_spec():
        s = lambda k: _rng.name_seed(f"segformer.{name}.{k}", seed)     # noqa: E731
        if kind == "bn":
            c = shape
            st[f"{name}.weight"] = torch.from_numpy(_rng.normal_f32((c,), s("weight"), 0.1, 1.0)) if perturb_bn else torch.ones(c)
            st[f"{name}.bias"] = torch.from_numpy(_rng.normal_f32((c,), s("bias"), 0.1, 0.0)) if perturb_bn else torch.zeros(c)
            st[f"{name}.running_mean"], st[f"{name}.running_var"] = torch.zeros(c), torch.ones(c)
            st[f"{name}.num_batches_tracked"] = torch.zeros((), dtype=torch.int64)
        else:
            bound = 1.0 / math.sqrt(shape[1] * shape[2] * shape[3])
            st[f"{name}.weight"] = torch.from_numpy(_rng.uniform_f32(shape, s("weight"), -bound, bound))
            st[f"{name}.bias"] = torch.from_numpy(_rng.uniform_f32((shape[0],), s("bias"), -bound, bound))
    return st


def param_names():
    return [k for k in init_state(0, False) if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]


def _conv(P, name, x, stride=1, padding=0, groups=1):
    return F.conv2d(x, P[f"{name}.weight"], P[f"{name}.bias"], stride, padding, 1, groups)


def _bn(P, name, x, training):
    y = F.batch_norm(x, P[f"{name}.running_mean"], P[f"{name}.running_var"], P[f"{name}.weight"], P[f"{name}.bias"], training, BN_MOMENTUM, BN_EPS)
    if training:
        P[f"{name}.num_batches_tracked"] += 1
    return y


def attention(P, pre, x, heads, r):
    b, c, h, w = x.shape
    q = _conv(P, f"{pre}.q", x).reshape(b, heads, c // heads, h * w).permute(0, 1, 3, 2)
    xr = _conv(P, f"{pre}.reduction", x, stride=r)
    kv = _conv(P, f"{pre}.kv", xr).reshape(b, 2, heads, c // heads, xr.shape[2] * xr.shape[3])
    k, v = kv[:, 0].permute(0, 1, 3, 2), kv[:, 1].permute(0, 1, 3, 2)
    a = ((q @ k.transpose(-2, -1)) * (c // heads) ** -0.5).softmax(dim=-1)
    out = (a @ v).permute(0, 1, 3, 2).reshape(b, c, h, w)
    return _conv(P, f"{pre}.proj", out)


def mixffn(P, pre, x, hidden):
    return _conv(P, f"{pre}.fc2", F.gelu(_conv(P, f"{pre}.dwconv", _conv(P, f"{pre}.fc1", x), padding=1, groups=hidden)))


def forward(P, x, training=True):
    """x [N, 3, H, W] -> probabilities [N, 1, H, W]"""
    H, W = x.shape[2:]
    feats = []
    c = x
    for i, (_, _, _, s, p) in enumerate(EMBED, 1):
        c = F.gelu(_bn(P, f"patch_embed{i}.1", _conv(P, f"patch_embed{i}.0", c, stride=s, padding=p), training))
        if i <= 3:
            _, heads, r, hid = STAGES[i - 1]
            c = c + attention(P, f"attn{i}", c, heads, r)
            c = c + mixffn(P, f"ffn{i}", c, hid)
        feats.append(c)
    c1, c2, c3, c4 = feats
    size = c1.shape[-2:]
    up = lambda t: F.interpolate(t, size=size, mode="bilinear", align_corners=False)      # noqa: E731
    fused = torch.cat([up(_conv(P, "linear_c4", c4)), up(_conv(P, "linear_c3", c3)), up(_conv(P, "linear_c2", c2)), _conv(P, "linear_c1", c1)], 1)
    y = F.relu(_bn(P, "linear_fuse.1", _conv(P, "linear_fuse.0", fused), training))
    y = F.relu(_bn(P, "head.1", _conv(P, "head.0", y, padding=1), training))
    p = torch.sigmoid(_conv(P, "head.3", y))
    return F.interpolate(p, size=(H, W), mode="bilinear", align_corners=False)
