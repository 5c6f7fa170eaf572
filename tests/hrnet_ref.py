"""CPU restatement of the reference's HRNet-Water baseline (TEST INFRASTRUCTURE ONLY -- never imported by the product path).

Functional form, on stock torch CPU fp32 ops over a flat name -> tensor state, of `HRNetWater` in the reference's
Extended_Baseline_Comparison.py:554-616: a stride-2 stem, a high- (48 channels, H/2), a medium- (96, H/4) and a low-resolution (192, H/8)
branch of two Conv2d -> BatchNorm2d -> ReLU each, the fusions Conv2d 1x1 -> BatchNorm2d -> Upsample x2 / x4, torch.cat and the head
Conv2d 3x3 -> BatchNorm2d -> ReLU -> Upsample x2 -> Conv2d 1x1 -> Sigmoid - in the reference's order of operations (upsample, then the 1x1
convolution; BatchNorm, then upsample), not the commuted order of the HIP kernels.  Trained there with nn.BCELoss
(ModelEvaluator.train_model, :780-837).  Pinned by tests/golden/hrnet_*.npz, which tests/golden/make_golden_hrnet.py produced from the
reference class itself.

`F` is looked up at module level on every call, so tests/decisions_seq.py's recorder can log (and force) the nine ReLU masks, in the order
stem.2, stem.5, hr_branch.2, hr_branch.5, mr_branch.2, mr_branch.5, lr_branch.2, lr_branch.5, head.2 (RELU_SITES).
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

# Sequentials of Conv2d 3x3 -> BatchNorm2d -> ReLU, twice: (name, ((cin, cout, stride), (cin, cout, stride)))
BRANCHES = (("stem", ((3, 64, 2), (64, 64, 1))), ("hr_branch", ((64, 48, 1), (48, 48, 1))), ("mr_branch", ((64, 96, 2), (96, 96, 1))),
            ("lr_branch", ((96, 192, 2), (192, 192, 1))))
FUSIONS = (("mr_to_hr", 96, 2), ("lr_to_hr", 192, 4))                   # Conv2d 1x1 -> 48, BatchNorm2d, Upsample(scale)
RELU_SITES = tuple(f"{name}.{i}" for name, _ in BRANCHES for i in (2, 5)) + ("head.2",)
# the parameters whose gradient is analytically zero (a constant that a train-mode BatchNorm removes): every conv bias but the last
ZERO_GRAD = tuple(f"{name}.{i}.bias" for name, _ in BRANCHES for i in (0, 3)) + tuple(f"{name}.0.bias" for name, _, _ in FUSIONS) + ("head.0.bias",)


def module_spec():
    """(name, shape, kind) in the reference's registration order; conv shapes are [cout, cin, k, k]"""
    s = []
    for name, convs in BRANCHES:
        for i, (cin, cout, _) in zip((0, 3), convs):
            s += [(f"{name}.{i}", (cout, cin, 3, 3), "conv"), (f"{name}.{i + 1}", cout, "bn")]
    for name, cin, _ in FUSIONS:
        s += [(f"{name}.0", (48, cin, 1, 1), "conv"), (f"{name}.1", 48, "bn")]
    s += [("head.0", (64, 144, 3, 3), "conv"), ("head.1", 64, "bn"), ("head.4", (1, 64, 1, 1), "conv")]
    return s


def init_state(seed=0, perturb_bn=True):
    """torch's default initialisation DISTRIBUTIONS (the reference class defines no initialiser) from the portable generator: conv weights
    and biases U(-1/sqrt(fan_in), +), BatchNorm gamma = 1 / beta = 0 (jittered when perturb_bn)."""
    st = OrderedDict()
    for name, shape, kind in module_spec():
        s = lambda k: _rng.name_seed(f"hrnet.{name}.{k}", seed)     # noqa: E731
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


def _conv(P, name, x, stride=1, padding=0):
    return F.conv2d(x, P[f"{name}.weight"], P[f"{name}.bias"], stride, padding)


def _bn(P, name, x, training):
    y = F.batch_norm(x, P[f"{name}.running_mean"], P[f"{name}.running_var"], P[f"{name}.weight"], P[f"{name}.bias"], training, BN_MOMENTUM, BN_EPS)
    if training:
        P[f"{name}.num_batches_tracked"] += 1
    return y


def _up(x, s):
    return F.interpolate(x, scale_factor=s, mode="bilinear", align_corners=False)


def _pair(P, name, x, training):
    stride = dict(BRANCHES)[name][0][2]
    x = F.relu(_bn(P, f"{name}.1", _conv(P, f"{name}.0", x, stride=stride, padding=1), training))
    return F.relu(_bn(P, f"{name}.4", _conv(P, f"{name}.3", x, padding=1), training))


def forward(P, x, training=True):
    """x [N, 3, H, W] -> probabilities [N, 1, H, W]"""
    stem = _pair(P, "stem", x, training)
    hr = _pair(P, "hr_branch", stem, training)
    mr = _pair(P, "mr_branch", stem, training)
    lr = _pair(P, "lr_branch", mr, training)
    mr_up = _up(_bn(P, "mr_to_hr.1", _conv(P, "mr_to_hr.0", mr), training), 2)
    lr_up = _up(_bn(P, "lr_to_hr.1", _conv(P, "lr_to_hr.0", lr), training), 4)
    fused = torch.cat([hr, mr_up, lr_up], 1)
    y = F.relu(_bn(P, "head.1", _conv(P, "head.0", fused, padding=1), training))
    return torch.sigmoid(_conv(P, "head.4", _up(y, 2)))
