"""CPU restatement of the reference's MSWNet baseline (TEST INFRASTRUCTURE ONLY -- never imported by the product path).

Functional form, on stock torch CPU ops over a flat name -> tensor state (fp32, or float64 when the state is), of `MultiScaleBlock` and `MSWNet`
in the reference's Extended_Baseline_Comparison.py:479-548, written from the model's description: four encoder levels (64 / 128 / 256 / 512
channels) that are each the concatenation of four parallel branches on one input - Conv2d 1x1, Conv2d 3x3, Conv2d 5x5 and MaxPool2d(3, stride 1,
padding 1) -> Conv2d 1x1, every one followed by BatchNorm2d and ReLU at a quarter of the level's channels - with MaxPool2d(2) between the
levels, a bridge (Conv2d 3x3 -> BatchNorm2d -> ReLU, 512 -> 1024 -> 1024), four ConvTranspose2d(k2, s2) + cat([up, skip]) decoder levels of one
Conv2d 3x3 -> BatchNorm2d -> ReLU each, and a Conv2d 1x1 -> Sigmoid head - in the reference's order of operations (every branch output
materialised, a real torch.cat), not the fused order of the HIP kernels.  Trained there with nn.BCELoss (ModelEvaluator.train_model, :780-837).
Pinned by tests/golden/mswnet_*.npz, which tests/golden/make_golden_mswnet.py produced from the reference class itself.

`F` is looked up at module level on every call, so tests/decisions_seq.py's recorder can log (and force) the discrete decisions in call order
(DECISION_SITES): every ReLU mask, every 2x2 pool winner and the 3x3 pool winners of levels 2-4.  The 3x3 pool of level 1 runs on the image:
no gradient depends on its winner, so it goes through `torch`, not `F`, and is neither logged nor forced.  `step(..., forced=...)` evaluates
one loss + backward under given decisions.
"""
from __future__ import annotations

import importlib
import math
import sys
from collections import OrderedDict

import torch
import torch.nn.functional as F

from segnet_ref import adam_step, bce_mean  # noqa: F401  (the same nn.BCELoss / Adam(lr, weight_decay) step)

_rng = importlib.import_module("eusipco-2026-robust-unet_amd.portable_rng")
BN_EPS, BN_MOMENTUM = 1e-5, 0.1

ENC = (("enc1", 3, 64), ("enc2", 64, 128), ("enc3", 128, 256), ("enc4", 256, 512))
DEC = (("dec4", 1024, 512), ("dec3", 512, 256), ("dec2", 256, 128), ("dec1", 128, 64))
UPS = (("up4", 1024, 512), ("up3", 512, 256), ("up2", 256, 128), ("up1", 128, 64))
# (branch, index of its convolution in the Sequential, kernel size); the BatchNorm sits behind the convolution, the ReLU behind that
BRANCHES = (("branch1", 0, 1), ("branch2", 0, 3), ("branch3", 0, 5), ("branch4", 1, 1))
# every discrete decision the recorder sees, in call order: ("relu" | "pool", site)
DECISION_SITES = tuple(
    s for lvl, (name, _, _) in enumerate(ENC, 1)
    for s in ([("relu", f"{name}.{br}.{i + 2}") for br, i, _ in BRANCHES[:3]] + ([("pool", f"{name}.branch4.0")] if lvl > 1 else [])
              + [("relu", f"{name}.branch4.3"), ("pool", f"pool{lvl}")])
) + (("relu", "bridge.2"), ("relu", "bridge.5")) + tuple(("relu", f"{name}.2") for name, _, _ in DEC)
# the parameters whose gradient is analytically zero (a constant that a train-mode BatchNorm removes): every conv bias in front of one
ZERO_GRAD = (tuple(f"{name}.{br}.{i}.bias" for name, _, _ in ENC for br, i, _ in BRANCHES) + ("bridge.0.bias", "bridge.3.bias")
             + tuple(f"{name}.0.bias" for name, _, _ in DEC))


def module_spec():
    """(name, shape, kind) in the reference's registration order; conv shapes are [cout, cin, k, k], transposed ones [cin, cout, 2, 2]"""
    s = []
    for name, cin, cout in ENC:
        for br, i, k in BRANCHES:
            s += [(f"{name}.{br}.{i}", (cout // 4, cin, k, k), "conv"), (f"{name}.{br}.{i + 1}", cout // 4, "bn")]
    s += [("bridge.0", (1024, 512, 3, 3), "conv"), ("bridge.1", 1024, "bn"), ("bridge.3", (1024, 1024, 3, 3), "conv"), ("bridge.4", 1024, "bn")]
    for (up, ucin, ucout), (name, cin, cout) in zip(UPS, DEC):
        s += [(up, (ucin, ucout, 2, 2), "convt"), (f"{name}.0", (cout, cin, 3, 3), "conv"), (f"{name}.1", cout, "bn")]
    s += [("outc.0", (1, 64, 1, 1), "conv")]
    return s


def init_state(seed=0, perturb_bn=True):
    """torch's default initialisation DISTRIBUTIONS (the reference class defines no initialiser) from the portable generator: conv weights
    and biases U(-1/sqrt(fan_in), +) (fan_in of a transposed convolution: its second dimension times the kernel), BatchNorm gamma = 1 /
    beta = 0 (jittered when perturb_bn)."""
    st = OrderedDict()
    for name, shape, kind in module_spec():
        s = lambda k: _rng.name_seed(f"mswnet.{name}.{k}", seed)     # noqa: E731
        if kind == "bn":
            c = shape
            st[f"{name}.weight"] = torch.from_numpy(_rng.normal_f32((c,), s("weight"), 0.1, 1.0)) if perturb_bn else torch.ones(c)
            st[f"{name}.bias"] = torch.from_numpy(_rng.normal_f32((c,), s("bias"), 0.1, 0.0)) if perturb_bn else torch.zeros(c)
            st[f"{name}.running_mean"], st[f"{name}.running_var"] = torch.zeros(c), torch.ones(c)
            st[f"{name}.num_batches_tracked"] = torch.zeros((), dtype=torch.int64)
        else:
            bound = 1.0 / math.sqrt(shape[1] * shape[2] * shape[3])
            st[f"{name}.weight"] = torch.from_numpy(_rng.uniform_f32(shape, s("weight"), -bound, bound))
            st[f"{name}.bias"] = torch.from_numpy(_rng.uniform_f32((shape[1] if kind == "convt" else shape[0],), s("bias"), -bound, bound))
    return st


def param_names():
    return [k for k in init_state(0, False) if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]


def _conv(P, name, x, padding=0):
    return F.conv2d(x, P[f"{name}.weight"], P.get(f"{name}.bias"), 1, padding)


def _bn(P, name, x, training):
    y = F.batch_norm(x, P[f"{name}.running_mean"], P[f"{name}.running_var"], P[f"{name}.weight"], P[f"{name}.bias"], training, BN_MOMENTUM, BN_EPS)
    if training:
        P[f"{name}.num_batches_tracked"] += 1
    return y


def _cbr(P, name, i, x, training):
    return F.relu(_bn(P, f"{name}.{i + 1}", _conv(P, f"{name}.{i}", x, padding=1), training))


def multi_scale_block(P, name, x, training=True, on_image=False):
    """x [N, Cin, H, W] -> [N, Cout, H, W]; on_image: the 3x3 pool's winners are no decision (the input carries no gradient)"""
    outs = []
    for br, i, k in BRANCHES:
        v = x
        if br == "branch4":
            v = torch.max_pool2d(x, 3, 1, 1) if on_image else F.max_pool2d(x, 3, 1, 1)
        outs.append(F.relu(_bn(P, f"{name}.{br}.{i + 1}", _conv(P, f"{name}.{br}.{i}", v, padding=k // 2), training)))
    return torch.cat(outs, 1)


def forward(P, x, training=True):
    """x [N, 3, H, W] -> probabilities [N, 1, H, W]"""
    skips, cur = [], x
    for lvl, (name, _, _) in enumerate(ENC, 1):
        e = multi_scale_block(P, name, cur, training, on_image=lvl == 1)
        skips.append(e)
        cur = F.max_pool2d(e, 2)
    b = _cbr(P, "bridge", 3, _cbr(P, "bridge", 0, cur, training), training)
    for (up, _, _), (name, _, _), e in zip(UPS, DEC, reversed(skips)):
        u = F.conv_transpose2d(b, P[f"{up}.weight"], P[f"{up}.bias"], stride=2)
        b = _cbr(P, name, 0, torch.cat([u, e], 1), training)
    return torch.sigmoid(_conv(P, "outc.0", b))


def step(st, x, y, forced=None, dtype=torch.float64, training=True):
    """One BCE loss + backward from the state `st` in `dtype`.  forced: the decisions to take instead of the restatement's own, in
    DECISION_SITES order (bool masks [n, c, h, w] for "relu", ATen flat indices into the input plane [n, c, ho, wo] for "pool").
    -> (log [(kind, decision, values)], {parameter name: gradient}, probabilities, loss)"""
    import decisions_seq as DS
    names = param_names()
    P = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in st.items()}
    for k in names:
        P[k].requires_grad_(True)
    out = {}

    def run(rec):
        out["p"] = forward(P, x.to(dtype), training)
        return (lambda q: out.setdefault("loss", bce_mean(q, y.to(dtype)))), out["p"], None
    log, prob = DS.run_oracle(sys.modules[__name__], run, forced)
    return log, {k: P[k].grad for k in names}, prob, out["loss"].detach()
