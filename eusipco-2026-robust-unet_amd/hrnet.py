"""HRNet-Water baseline of the reference (Extended_Baseline_Comparison.py:554-616) on the gfx950 kernels.

Drop-in for the reference's `HRNetWater` (trained there by ModelEvaluator.train_model: nn.BCELoss, Adam 1e-4, weight decay 1e-4, :780-837):
same constructor, attribute tree and state_dict (79 keys, 822 593 parameters).  `stem` (Conv2d 3x3 s2 -> BatchNorm2d -> ReLU -> Conv2d 3x3 ->
BatchNorm2d -> ReLU, 64 channels at H/2), three branches of the same two-convolution form - `hr_branch` (48 channels at H/2), `mr_branch`
(stride 2, 96 channels at H/4, from the stem), `lr_branch` (stride 2, 192 channels at H/8, from mr) -, the fusions `mr_to_hr` / `lr_to_hr`
(Conv2d 1x1 -> 48, BatchNorm2d, Upsample x2 / x4, no activation), torch.cat([hr, mr_up, lr_up]) and `head` (Conv2d 3x3 144 -> 64, BatchNorm2d,
ReLU, Upsample x2, Conv2d 1x1 64 -> 1, Sigmoid).  forward(x [N, 3, H, W]) -> sigmoid probabilities [N, 1, H, W].

One autograd node with an explicit backward, NHWC inside (baseline.py):
  convolutions   3x3 stride 1 and 1x1 through ops.conv_fwd / conv_dgrad / conv_wgrad (BatchNorm statistics from the convolution's epilogue where
                 the kernel offers them), the three stride-2 ones through runet_conv2d_general / runet_conv_wgrad_general (the stem's reads
                 the RGB input padded to 4 channels, cin_w = 3); BatchNorm + ReLU as the U-Net's (runet_bn_apply, ReLU mask recomputed from
                 the BatchNorm input in the backward)
  concat         never copied: hr_branch's last BatchNorm + ReLU writes channels [0, 48) of the 144-channel buffer, the fusion kernels
                 [48, 96) and [96, 144); the backward reads the matching slices of the head convolution's data gradient
  fusions        runet_bn_bilinear_nhwc_fwd: the 1x1 convolution's raw output interpolated into the slice with the BatchNorm affine as one FMA
                 per output (the affine commutes with the interpolation); backward runet_bilinear_nhwc_bwd_sums (gather adjoint + the
                 BatchNorm-backward sums in one pass) and runet_bn_bwd_apply
  head           runet_hr_head_fwd + runet_up2_sigmoid_fwd: BatchNorm + ReLU + the 64 -> 1 convolution at H/2 from the 3x3 convolution's raw
                 output, then the one-channel logit plane upsampled and squashed (the 1x1 convolution commutes with the interpolation): the
                 [N, H, W, 64] map of the reference's order (268 MB at 16 x 256^2), its gradient and the H/2 activation never exist;
                 backward runet_up2_sigmoid_bwd, runet_hr_head_bwd_reduce, runet_hr_head_bwd_apply
The stem output and mr have several consumers: their gradients are accumulated by the data-gradient kernels (`accumulate`).
The conv biases in front of a BatchNorm are kept and trained as the reference does (their gradient is the channel sum).
Every gradient is summed in a fixed order (no float atomics): two steps from the same state give the same bits.

A/B switches (blocks.py): RUNET_NO_FUSED_HR_HEAD=1 (bn_apply + runet_bilinear_nhwc_fwd to 64 channels at full size + runet_outc_*),
RUNET_NO_FUSED_BN_UPSAMPLE=1 (bn_apply + runet_bilinear_nhwc_fwd / _bwd + bn_backward), RUNET_NO_EPILOGUE_STATS=1 (runet_bn_stats passes).

Bounds: n_classes = 1 only, H and W multiples of 8 (the reference's own concat fails on other sizes), fp32 only, per-rank BatchNorm
statistics only.
"""
from __future__ import annotations

import torch.nn as nn

from . import blocks as B
from . import ops
from .baseline import FusedNet, ReLU, Sigmoid, check_image, conv_bn_relu
from .model import BatchNorm2d, Conv2d, _Holder

# the four Sequentials of the form Conv2d 3x3 -> BatchNorm2d -> ReLU, twice: (attribute, ((cin, cout, stride), (cin, cout, stride)))
BRANCHES = (("stem", ((3, 64, 2), (64, 64, 1))), ("hr_branch", ((64, 48, 1), (48, 48, 1))), ("mr_branch", ((64, 96, 2), (96, 96, 1))),
            ("lr_branch", ((96, 192, 2), (192, 192, 1))))
# the fusions Conv2d 1x1 -> BatchNorm2d -> Upsample: (attribute, cin, scale factor), in the concat's channel order behind hr's [0, 48)
FUSIONS = (("mr_to_hr", 96, 2), ("lr_to_hr", 192, 4))
HR, CAT, HEAD = 48, 144, 64


class _Upsample(_Holder):
    """nn.Upsample(scale_factor, mode='bilinear', align_corners=False) stand-in (no parameters; fused into the neighbouring kernels)."""

    def __init__(self, scale_factor):
        super().__init__()
        self.scale_factor, self.mode, self.align_corners = scale_factor, "bilinear", False


class HRNetWater(FusedNet):
    FP32_ONLY = "the head and fusion kernels are fp32"

    def __init__(self, n_classes=1):
        super().__init__()
        if n_classes != 1:
            raise ValueError("the fused head implements the reference's n_classes=1 sigmoid head")
        self.n_classes = n_classes
        for name, convs in BRANCHES:
            mods = []
            for cin, cout, stride in convs:
                mods += [Conv2d(cin, cout, 3, padding=1, stride=stride), BatchNorm2d(cout), ReLU()]
            setattr(self, name, nn.Sequential(*mods))
        for name, cin, s in FUSIONS:
            setattr(self, name, nn.Sequential(Conv2d(cin, HR, 1), BatchNorm2d(HR), _Upsample(s)))
        self.head = nn.Sequential(Conv2d(CAT, HEAD, 3, padding=1), BatchNorm2d(HEAD), ReLU(), _Upsample(2), Conv2d(HEAD, n_classes, 1), Sigmoid())

    def _check_input(self, x):
        check_image(x, 8, "three stride-2 convolutions whose outputs are upsampled x2 / x4 into one concat")

    def _passes(self):
        return hrnet_forward, hrnet_backward


def hrnet_forward(net: HRNetWater, x, save=True):
    tr = net.training
    sm = B.Small(x.device)
    n = x.shape[0]
    C = {} if save else None
    ops.branches_pay(n, x.shape[2], x.shape[3])
    if save:
        ops.prefetch_derived()
    feats = {}
    cur = B.to_nhwc_pad(x, 4)
    cat = None
    for name, _ in BRANCHES:
        seq = getattr(net, name)
        src = cur if name == "stem" else feats["mr_branch" if name == "lr_branch" else "stem"]
        a = conv_bn_relu(seq, 0, src, tr, sm, C, f"{name}.0")
        if name == "hr_branch":
            cat = ops.empty_nhwc(n, a.shape[1], a.shape[2], CAT, a)
        feats[name] = conv_bn_relu(seq, 3, a, tr, sm, C, f"{name}.3", out=cat[..., :HR] if name == "hr_branch" else None)
    for j, (name, _, s) in enumerate(FUSIONS):
        seq = getattr(net, name)
        f = feats["mr_branch" if name == "mr_to_hr" else "lr_branch"]
        w = ops.hwio(seq[0].weight)
        fs = {} if tr else None
        t = ops.conv_fwd(f, w, seq[0].bias, stats=fs)
        sc, sh, mean, invstd, _ = B.bn_coeff(t, seq[1].state(), tr, sm, fused=fs)
        B.bn_bilinear_forward(t, sc, sh, cat[..., HR * (j + 1):HR * (j + 2)], s)
        if save:
            C[name] = dict(x=f, w=w, t=t, s=sc, mean=mean, invstd=invstd, scale=s)
    hconv, hbn, oconv = net.head[0], net.head[1], net.head[4]
    wh = ops.hwio(hconv.weight)
    fs = {} if tr else None
    t = ops.conv_fwd(cat, wh, hconv.bias, stats=fs)
    sc, sh, mean, invstd, _ = B.bn_coeff(t, hbn.state(), tr, sm, fused=fs)
    wo = ops.hwio(oconv.weight)
    prob, saved = B.hr_head_forward(t, sc, sh, wo, oconv.bias)
    if save:
        C["head"] = dict(x=cat, w=wh, t=t, s=sc, h=sh, mean=mean, invstd=invstd, wo=wo, prob=prob, saved=saved)
        C["training"] = tr
    return prob, C


def hrnet_backward(net: HRNetWater, C, dprob):
    """-> {parameter name: gradient in the parameter's PHYSICAL layout (conv weights HWIO)}"""
    G = {}
    dev = dprob.device
    tr = C["training"]

    def conv_grads(name, cx, dt):
        """weight and bias gradient of the stride-1 convolution that produced cx["t"] (dt: the gradient of that output)"""
        k = cx["w"].shape[0]
        G[name + ".weight"] = ops.conv_wgrad(cx["x"], dt, k, k)
        G[name + ".bias"] = B.chan_sum(dt, B.vec(dt.shape[3], dev))

    def bn_relu_back(seq, i, dy):
        cx = C[f"{seq}.{i}"]
        return cx, B.conv_bn_relu_backward(cx, dy, G, seq, i, tr)

    def pair_back(seq, dy, dsrc=None):
        """backward of a two-convolution Sequential; its input's gradient goes into dsrc (+=) when given.  -> that gradient"""
        cx, dt = bn_relu_back(seq, 3, dy)
        da = ops.conv_dgrad(dt, cx["w"])
        del dt
        cx, dt = bn_relu_back(seq, 0, da)
        if seq == "stem":
            return None
        if cx["stride"] == 1:
            return ops.conv_dgrad(dt, cx["w"], out=dsrc, accumulate=dsrc is not None)
        return ops.conv_general_dgrad(dt, cx["w"], cx["x"].shape[1], cx["x"].shape[2], cx["stride"], 1, out=dsrc, accumulate=dsrc is not None)

    # ---- head
    hc = C["head"]
    c = hc["t"].shape[3]
    dt, out = B.hr_head_backward(dprob, hc["prob"], hc["t"], hc["s"], hc["h"], hc["wo"], hc["mean"], hc["invstd"], saved=hc["saved"], training=tr)
    G["head.1.weight"], G["head.1.bias"] = out[:c], out[c:2 * c]
    G["head.4.weight"], G["head.4.bias"] = out[2 * c:3 * c].view(1, 1, c, 1), out[3 * c:]
    conv_grads("head.0", hc, dt)
    dcat = ops.conv_dgrad(dt, hc["w"])
    del dt
    # ---- fusion branches: gradients of lr and mr from their 1x1 projections
    dfeat = {}
    for j, (name, _, s) in enumerate(FUSIONS):
        fx = C[name]
        sums = B.vec(2 * HR, dev)
        dt = B.bn_bilinear_backward(dcat[..., HR * (j + 1):HR * (j + 2)], fx["t"], fx["mean"], fx["invstd"], fx["s"], sums, s, training=tr)
        G[f"{name}.1.weight"], G[f"{name}.1.bias"] = sums[:HR], sums[HR:]
        conv_grads(f"{name}.0", fx, dt)
        dfeat[name] = ops.conv_dgrad(dt, fx["w"])
        del dt
    # ---- lr -> mr (+=), then mr and hr -> stem (the second +=), then the stem
    dmr = pair_back("lr_branch", dfeat["lr_to_hr"], dsrc=dfeat["mr_to_hr"])
    dstem = pair_back("mr_branch", dmr)
    pair_back("hr_branch", dcat[..., :HR], dsrc=dstem)
    pair_back("stem", dstem)
    return G
