"""CPU restatement of the reference's SegNet baseline (TEST INFRASTRUCTURE ONLY -- never imported by the product path).

Functional form, on stock torch CPU fp32 ops over a flat name -> tensor state, of `SegNet` in the reference's comne.py:84-211: Conv3x3 (bias)
-> BatchNorm2d -> ReLU stacks, MaxPool2d(2, 2, return_indices=True) behind every encoder stack, MaxUnpool2d(2, 2) by those indices in front
of every decoder stack, Conv2d(64, 1, 3) + sigmoid head.  Trained there with nn.BCELoss (comne.py:650).  Pinned by tests/golden/segnet_*.npz,
which tests/golden/make_golden_segnet.py produced from the reference class itself.

`F` is looked up at module level on every call, so tests/decisions_segnet.py can swap in a recorder that logs (and forces) every ReLU mask
and every pool winner - a forced winner also drives the unpool.
"""
from __future__ import annotations

import importlib
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

_rng = importlib.import_module("eusipco-2026-robust-unet_amd.portable_rng")
BN_EPS, BN_MOMENTUM = 1e-5, 0.1

# (stack, [(cin, cout) of each Conv-BN-ReLU triple]); dec1 then ends in the head conv "dec1.3" (64 -> 1, no BatchNorm)
ENC = (("enc1", ((3, 64), (64, 64))), ("enc2", ((64, 128), (128, 128))), ("enc3", ((128, 256), (256, 256), (256, 256))),
       ("enc4", ((256, 512), (512, 512), (512, 512))))
DEC = (("dec4", ((512, 512), (512, 512), (512, 256))), ("dec3", ((256, 256), (256, 256), (256, 128))), ("dec2", ((128, 128), (128, 64))),
       ("dec1", ((64, 64),)))


def module_spec():
    s = []
    for pre, convs in ENC + DEC:
        for i, (cin, cout) in enumerate(convs):
            s += [(f"{pre}.{3 * i}", (cout, cin, 3, 3), "conv"), (f"{pre}.{3 * i + 1}", cout, "bn")]
    s.append(("dec1.3", (1, 64, 3, 3), "conv"))
    return s


def init_state(seed=0, perturb_bn=True):
    """torch's default initialisation DISTRIBUTIONS (the reference class defines no initialiser) from the portable generator: conv weights
    and biases U(-1/sqrt(fan_in), +), BatchNorm gamma = 1 / beta = 0 (jittered when perturb_bn)."""
    st = OrderedDict()
    for name, shape, kind in module_spec():
        s = lambda k: _rng.name_seed(f"segnet.{name}.{k}", seed)     # noqa: E731
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
    # registration order of the reference: enc1..4 then dec4..1 (module_spec already follows it)
    return st


def param_names():
    return [k for k in init_state(0, False) if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]


def _bn(P, name, x, training):
    y = F.batch_norm(x, P[f"{name}.running_mean"], P[f"{name}.running_var"], P[f"{name}.weight"], P[f"{name}.bias"], training, BN_MOMENTUM, BN_EPS)
    if training:
        P[f"{name}.num_batches_tracked"] += 1
    return y


def stack(P, pre, x, n, training):
    for i in range(n):
        x = F.relu(_bn(P, f"{pre}.{3 * i + 1}", F.conv2d(x, P[f"{pre}.{3 * i}.weight"], P[f"{pre}.{3 * i}.bias"], padding=1), training))
    return x


def forward(P, x, training=True, want_logit=False):
    """x [N, 3, H, W] -> sigmoid probabilities [N, 1, H, W] (and the logit when want_logit)"""
    idx, sizes = {}, {}
    for lvl, (pre, convs) in enumerate(ENC, 1):
        x = stack(P, pre, x, len(convs), training)
        sizes[lvl] = x.shape[2:]
        x, idx[lvl] = F.max_pool2d(x, 2, 2, return_indices=True)
    for lvl, (pre, convs) in zip((4, 3, 2, 1), DEC):
        x = F.max_unpool2d(x, idx[lvl], 2, 2, output_size=sizes[lvl])
        x = stack(P, pre, x, len(convs), training)
    z = F.conv2d(x, P["dec1.3.weight"], P["dec1.3.bias"], padding=1)
    p = torch.sigmoid(z)
    return (p, z) if want_logit else p


def bce_mean(prob, target):
    return F.binary_cross_entropy(prob, target)


def adam_step(params, grads, m, v, step, lr=1e-4, wd=1e-4, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam(lr, weight_decay) (comne.py:651), one step, in place."""
    for p, g, mm, vv in zip(params, grads, m, v):
        g = g + wd * p.detach()
        mm.mul_(b1).add_(g, alpha=1 - b1)
        vv.mul_(b2).addcmul_(g, g, value=1 - b2)
        denom = (vv.sqrt() / math.sqrt(1 - b2 ** step)).add_(eps)
        with torch.no_grad():
            p.addcdiv_(mm, denom, value=-lr / (1 - b1 ** step))
