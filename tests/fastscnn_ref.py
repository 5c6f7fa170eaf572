"""CPU restatement of the reference's Fast-SCNN baseline (TEST INFRASTRUCTURE ONLY -- never imported by the product path).

Functional form, on stock torch CPU ops over a flat name -> tensor state (fp32, or float64 when the state is), of `FastSCNN` and its sub-modules
in the reference's comne.py:305-476, written from the model's description: a stem (Conv2d 3 -> 32, 3x3 stride 2, no bias -> BatchNorm2d -> ReLU),
thirteen depthwise-separable layers (depthwise 3x3 without bias -> pointwise 1x1 without bias -> BatchNorm2d -> ReLU; 32 -> 48 s2, 48 -> 64 s2,
64 -> 64 x 3, 64 -> 96 s2, 96 -> 96 x 2, 96 -> 128, 128 -> 128 x 2, and the classifier's 128 -> 128 x 2), a pyramid pooling module on the H/16 map
(AdaptiveAvgPool2d to 1 / 2 / 3 / 6 bins -> Conv2d 1x1 128 -> 32 -> BatchNorm2d -> ReLU -> bilinear resize, concatenated behind the input), a
feature fusion (BatchNorm(Conv1x1 64 -> 128) of the H/8 map + the bilinear resize of BatchNorm(Conv1x1 256 -> 128) of the pyramid, ReLU), and
a Conv2d 1x1 128 -> 1 head resized to the input and passed through a sigmoid - in the reference's order of operations (every tensor
materialised, a real torch.cat), not the fused order of the HIP kernels.  Trained there with nn.BCELoss.  Pinned by tests/golden/fastscnn_*.npz,
which tests/golden/make_golden_fastscnn.py produced from the reference class itself.

`F` is looked up at module level on every call, so tests/decisions_seq.py's recorder can log (and force) the discrete decisions in call order
(DECISION_SITES): the ReLU masks only - stem, thirteen separable layers, four pyramid branches, the fusion.  `step(..., forced=...)` evaluates
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

LTD, GFE, FFM, CLS = "learning_to_downsample", "global_feature_extractor", "feature_fusion", "classifier"
# the separable layers in forward order: (name, cin, cout, stride)
SEP_HEAD = ((f"{LTD}.dsconv1", 32, 48, 2), (f"{LTD}.dsconv2", 48, 64, 2))
SEP_TRUNK = ((f"{GFE}.block1.0", 64, 64, 1), (f"{GFE}.block1.1", 64, 64, 1), (f"{GFE}.block1.2", 64, 64, 1),
             (f"{GFE}.block2.0", 64, 96, 2), (f"{GFE}.block2.1", 96, 96, 1), (f"{GFE}.block2.2", 96, 96, 1),
             (f"{GFE}.block3.0", 96, 128, 1), (f"{GFE}.block3.1", 128, 128, 1), (f"{GFE}.block3.2", 128, 128, 1))
SEP_TAIL = ((f"{CLS}.conv1", 128, 128, 1), (f"{CLS}.conv2", 128, 128, 1))
BINS = (1, 2, 3, 6)
# every discrete decision the recorder sees, in call order (all are ReLU masks)
DECISION_SITES = ((("relu", f"{LTD}.conv1.2"),) + tuple(("relu", f"{n}.relu") for n, _, _, _ in SEP_HEAD + SEP_TRUNK)
                  + tuple(("relu", f"{GFE}.ppm.convs.{j}.3") for j in range(4)) + (("relu", f"{FFM}.relu"),)
                  + tuple(("relu", f"{n}.relu") for n, _, _, _ in SEP_TAIL))
# the parameters whose gradient is analytically zero (a constant that a train-mode BatchNorm removes): the pyramid branches' conv biases
ZERO_GRAD = tuple(f"{GFE}.ppm.convs.{j}.1.bias" for j in range(4))


def module_spec():
    """(name, shape, kind) in the reference's registration order; kind "conv" has a bias, "conv0" has none, conv shapes are [cout, cin / groups, k, k]"""
    s = [(f"{LTD}.conv1.0", (32, 3, 3, 3), "conv0"), (f"{LTD}.conv1.1", 32, "bn")]

    def sep(name, cin, cout):
        return [(f"{name}.depthwise", (cin, 1, 3, 3), "conv0"), (f"{name}.pointwise", (cout, cin, 1, 1), "conv0"), (f"{name}.bn", cout, "bn")]
    for name, cin, cout, _ in SEP_HEAD + SEP_TRUNK:
        s += sep(name, cin, cout)
    for j in range(4):
        s += [(f"{GFE}.ppm.convs.{j}.1", (32, 128, 1, 1), "conv"), (f"{GFE}.ppm.convs.{j}.2", 32, "bn")]
    s += [(f"{FFM}.conv_low.0", (128, 64, 1, 1), "conv0"), (f"{FFM}.conv_low.1", 128, "bn"),
          (f"{FFM}.conv_high.0", (128, 256, 1, 1), "conv0"), (f"{FFM}.conv_high.1", 128, "bn")]
    for name, cin, cout, _ in SEP_TAIL:
        s += sep(name, cin, cout)
    s += [(f"{CLS}.conv3", (1, 128, 1, 1), "conv")]
    return s


def init_state(seed=0, perturb_bn=True):
    """torch's default initialisation DISTRIBUTIONS (the reference class defines no initialiser) from the portable generator: conv weights
    and biases U(-1/sqrt(fan_in), +), BatchNorm gamma = 1 / beta = 0 (jittered when perturb_bn)."""
    st = OrderedDict()
    for name, shape, kind in module_spec():
        s = lambda k: _rng.name_seed(f"fastscnn.{name}.{k}", seed)     # noqa: E731
        if kind == "bn":
            c = shape
            st[f"{name}.weight"] = torch.from_numpy(_rng.normal_f32((c,), s("weight"), 0.1, 1.0)) if perturb_bn else torch.ones(c)
            st[f"{name}.bias"] = torch.from_numpy(_rng.normal_f32((c,), s("bias"), 0.1, 0.0)) if perturb_bn else torch.zeros(c)
            st[f"{name}.running_mean"], st[f"{name}.running_var"] = torch.zeros(c), torch.ones(c)
            st[f"{name}.num_batches_tracked"] = torch.zeros((), dtype=torch.int64)
        else:
            bound = 1.0 / math.sqrt(shape[1] * shape[2] * shape[3])
            st[f"{name}.weight"] = torch.from_numpy(_rng.uniform_f32(shape, s("weight"), -bound, bound))
            if kind == "conv":
                st[f"{name}.bias"] = torch.from_numpy(_rng.uniform_f32((shape[0],), s("bias"), -bound, bound))
    return st


def param_names():
    return [k for k in init_state(0, False) if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]


def _bn(P, name, x, training):
    y = F.batch_norm(x, P[f"{name}.running_mean"], P[f"{name}.running_var"], P[f"{name}.weight"], P[f"{name}.bias"], training, BN_MOMENTUM, BN_EPS)
    if training:
        P[f"{name}.num_batches_tracked"] += 1
    return y


def dwsep(P, name, x, stride, training=True):
    """DepthwiseSeparableConv: x [N, Cin, H, W] -> [N, Cout, ceil(H / stride), ceil(W / stride)]"""
    d = F.conv2d(x, P[f"{name}.depthwise.weight"], None, stride, 1, 1, x.shape[1])
    return F.relu(_bn(P, f"{name}.bn", F.conv2d(d, P[f"{name}.pointwise.weight"]), training))


def ppm(P, name, x, training=True):
    """PyramidPoolingFastSCNN: x [N, C, H, W] -> [N, 2C, H, W]"""
    out = [x]
    for j, b in enumerate(BINS):
        v = F.conv2d(F.adaptive_avg_pool2d(x, b), P[f"{name}.convs.{j}.1.weight"], P[f"{name}.convs.{j}.1.bias"])
        v = F.relu(_bn(P, f"{name}.convs.{j}.2", v, training))
        out.append(F.interpolate(v, size=x.shape[2:], mode="bilinear", align_corners=False))
    return torch.cat(out, 1)


def ffm(P, name, x_high, x_low, training=True):
    lo = _bn(P, f"{name}.conv_low.1", F.conv2d(x_low, P[f"{name}.conv_low.0.weight"]), training)
    hi = _bn(P, f"{name}.conv_high.1", F.conv2d(x_high, P[f"{name}.conv_high.0.weight"]), training)
    return F.relu(lo + F.interpolate(hi, size=lo.shape[2:], mode="bilinear", align_corners=False))


def forward(P, x, training=True):
    """x [N, 3, H, W] -> probabilities [N, 1, H, W]"""
    a = F.relu(_bn(P, f"{LTD}.conv1.1", F.conv2d(x, P[f"{LTD}.conv1.0.weight"], None, 2, 1), training))
    for name, _, _, stride in SEP_HEAD:
        a = dwsep(P, name, a, stride, training)
    x_low = a
    for name, _, _, stride in SEP_TRUNK:
        a = dwsep(P, name, a, stride, training)
    a = ffm(P, FFM, ppm(P, f"{GFE}.ppm", a, training), x_low, training)
    for name, _, _, stride in SEP_TAIL:
        a = dwsep(P, name, a, stride, training)
    z = F.conv2d(a, P[f"{CLS}.conv3.weight"], P[f"{CLS}.conv3.bias"])
    return torch.sigmoid(F.interpolate(z, size=x.shape[2:], mode="bilinear", align_corners=False))


def step(st, x, y, forced=None, dtype=torch.float64, training=True):
    """One BCE loss + backward from the state `st` in `dtype`.  forced: the decisions to take instead of the restatement's own, in
    DECISION_SITES order (bool masks [n, c, h, w]).  -> (log [(kind, decision, values)], {parameter name: gradient}, probabilities, loss)"""
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
