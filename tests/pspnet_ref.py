"""CPU restatement of the reference's PSPNet baseline (TEST INFRASTRUCTURE ONLY -- never imported by the product path).

Functional form, on stock torch CPU ops over a flat name -> tensor state (fp32, or float64 when the state is), of `PSPNet` and `PyramidPooling`
in the reference's comne.py:214-299, written from the model's description: four Conv2d 3x3 stride 2 with bias -> BatchNorm2d -> ReLU stages
(3 -> 64 -> 128 -> 256 -> 512, the H/16 map), a pyramid pooling module (AdaptiveAvgPool2d to 1 / 2 / 3 / 6 bins -> Conv2d 1x1 512 -> 128 ->
BatchNorm2d -> ReLU -> bilinear resize, concatenated behind the input: 1024 channels), Conv2d 3x3 1024 -> 512 -> BatchNorm2d -> ReLU ->
Dropout2d(0.1) -> Conv2d 1x1 512 -> 1, a bilinear resize to the input size and a sigmoid - in the reference's order of operations (every tensor
materialised, a real torch.cat), not the folded order of the HIP kernels.  Trained there with nn.BCELoss.  Pinned by
tests/golden/pspnet_*.npz, which tests/golden/make_golden_pspnet.py produced from the reference class itself.

`F` is looked up at module level on every call, so tests/decisions_seq.py's recorder can log (and force) the discrete decisions in call order
(DECISION_SITES): the ReLU masks only - the four backbone stages, the four pyramid branches, final_conv.2.  `step(..., forced=...)` evaluates
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

BACKBONE = (("conv1", 3, 64), ("conv2", 64, 128), ("conv3", 128, 256), ("conv4", 256, 512))
BINS = (1, 2, 3, 6)
C, CQ, DROP_P = 512, 128, 0.1
# every discrete decision the recorder sees, in call order (all are ReLU masks)
DECISION_SITES = (tuple(("relu", f"{n}.2") for n, _, _ in BACKBONE) + tuple(("relu", f"ppm.convs.{j}.3") for j in range(4))
                  + (("relu", "final_conv.2"),))
# the parameters whose gradient is analytically zero (a constant that a train-mode BatchNorm removes): every conv bias in front of a BatchNorm
ZERO_GRAD = tuple(f"{n}.0.bias" for n, _, _ in BACKBONE) + tuple(f"ppm.convs.{j}.1.bias" for j in range(4)) + ("final_conv.0.bias",)


def module_spec():
    """(name, shape, kind) in the reference's registration order; kind "conv": a Conv2d with bias [cout, cin, k, k], "bn": BatchNorm2d"""
    s = []
    for name, cin, cout in BACKBONE:
        s += [(f"{name}.0", (cout, cin, 3, 3), "conv"), (f"{name}.1", cout, "bn")]
    for j in range(4):
        s += [(f"ppm.convs.{j}.1", (CQ, C, 1, 1), "conv"), (f"ppm.convs.{j}.2", CQ, "bn")]
    s += [("final_conv.0", (C, 2 * C, 3, 3), "conv"), ("final_conv.1", C, "bn"), ("final_conv.4", (1, C, 1, 1), "conv")]
    return s


def init_state(seed=0, perturb_bn=True):
    """torch's default initialisation DISTRIBUTIONS (the reference class defines no initialiser) from the portable generator: conv weights
    and biases U(-1/sqrt(fan_in), +), BatchNorm gamma = 1 / beta = 0 (jittered when perturb_bn)."""
    st = OrderedDict()
    for name, shape, kind in module_spec():
        s = lambda k: _rng.name_seed(f"pspnet.{name}.{k}", seed)     # noqa: E731
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


def dropout_masks(n, seed=0):
    """{"final_conv.3": [n, 512] keep-mask already divided by 1 - p} from the portable generator"""
    return {"final_conv.3": torch.from_numpy(_rng.bernoulli_keep((n, C), _rng.name_seed("pspnet.final_conv.3.dropout", seed), DROP_P)) / (1.0 - DROP_P)}


def _bn(P, name, x, training):
    y = F.batch_norm(x, P[f"{name}.running_mean"], P[f"{name}.running_var"], P[f"{name}.weight"], P[f"{name}.bias"], training, BN_MOMENTUM, BN_EPS)
    if training:
        P[f"{name}.num_batches_tracked"] += 1
    return y


def ppm(P, x, training=True):
    """PyramidPooling: x [N, 512, h, w] -> [N, 1024, h, w]"""
    out = [x]
    for j, b in enumerate(BINS):
        v = F.conv2d(F.adaptive_avg_pool2d(x, b), P[f"ppm.convs.{j}.1.weight"], P[f"ppm.convs.{j}.1.bias"])
        v = F.relu(_bn(P, f"ppm.convs.{j}.2", v, training))
        out.append(F.interpolate(v, size=x.shape[2:], mode="bilinear", align_corners=False))
    return torch.cat(out, 1)


def forward(P, x, training=True, masks=None):
    """x [N, 3, H, W] -> probabilities [N, 1, H, W]; masks: dropout_masks(...) or None (no dropout)"""
    a = x
    for name, _, _ in BACKBONE:
        a = F.relu(_bn(P, f"{name}.1", F.conv2d(a, P[f"{name}.0.weight"], P[f"{name}.0.bias"], 2, 1), training))
    a = F.conv2d(ppm(P, a, training), P["final_conv.0.weight"], P["final_conv.0.bias"], 1, 1)
    a = F.relu(_bn(P, "final_conv.1", a, training))
    if training and masks is not None:
        a = a * masks["final_conv.3"].to(a.dtype)[:, :, None, None]
    z = F.conv2d(a, P["final_conv.4.weight"], P["final_conv.4.bias"])
    return torch.sigmoid(F.interpolate(z, size=x.shape[2:], mode="bilinear", align_corners=False))


def step(st, x, y, forced=None, dtype=torch.float64, training=True, masks=None):
    """One BCE loss + backward from the state `st` in `dtype`.  forced: the decisions to take instead of the restatement's own, in
    DECISION_SITES order (bool masks [n, c, h, w]).  -> (log [(kind, decision, values)], {parameter name: gradient}, probabilities, loss)"""
    import decisions_seq as DS
    names = param_names()
    P = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in st.items()}
    for k in names:
        P[k].requires_grad_(True)
    out = {}

    def run(rec):
        out["p"] = forward(P, x.to(dtype), training, masks)
        return (lambda q: out.setdefault("loss", bce_mean(q, y.to(dtype)))), out["p"], None
    log, prob = DS.run_oracle(sys.modules[__name__], run, forced)
    return log, {k: P[k].grad for k in names}, prob, out["loss"].detach()
