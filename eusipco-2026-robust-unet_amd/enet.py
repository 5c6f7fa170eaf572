"""ENet baseline of the reference (comne.py:482-608) on the gfx950 kernels.

Drop-in for the reference's `ENet` and its sub-modules `InitialBlock` and `BottleneckBlock` (trained there with nn.BCELoss and Adam 1e-4, weight
decay 1e-4): same constructor, attribute tree and state_dict (280 entries, 142 parameter tensors, 257 680 parameters).
forward(x [N, 3, H, W]) -> sigmoid probabilities [N, 1, H, W].

  initial   cat([Conv2d 3 -> 13, 3x3 stride 2, no bias; MaxPool2d(2)]) -> BatchNorm2d(16) -> ReLU: the H/2 map
  encoder1  BottleneckBlock(16 -> 64, downsample), 3 x BottleneckBlock(64 -> 64), Dropout2d p = 0.01: H/4
  encoder2  BottleneckBlock(64 -> 128, downsample), then 128 -> 128: plain, dilation 2, asymmetric, dilation 4, plain, dilation 8, asymmetric,
            dilation 16, Dropout2d p = 0.1: H/8
  decoder   ConvTranspose2d(128 -> 64, k3 s2 p1 op1) + BatchNorm2d + ReLU, ConvTranspose2d(64 -> 16, the same) + BatchNorm2d + ReLU,
            ConvTranspose2d(16 -> 1, k2 s2), sigmoid
A BottleneckBlock(cin, cout) works at ci = cin // 4 channels: conv1 (1x1, stride 2 when downsampling) -> conv2 (3x3 with padding = dilation, or
(5, 1) then (1, 5)) -> conv3 (1x1 ci -> cout, BatchNorm2d, Dropout2d), each convolution without bias and followed by BatchNorm2d (+ ReLU in
conv1 / conv2); out = relu(conv3 + identity), identity = x or BatchNorm2d(Conv1x1(MaxPool2d(2)(x))).

One autograd node with an explicit backward, NHWC inside (baseline.py):
  initial   blocks.enet_initial_forward / _backward: runet_enet_initial_fwd writes the 16-wide cat(convolution, pool) and its BatchNorm
            partials in one pass over the NCHW image (the pool window is part of the convolution's patch), runet_enet_initial_wgrad the
            13-column weight gradient; the shared BatchNorm kernels behind it
  1x1, 3x3  ops.conv_fwd / conv_dgrad / conv_wgrad (dilation 1..16), BatchNorm statistics from the 1x1 epilogues where offered; stride 2
            through ops.conv_general_*
  (5,1),(1,5) ops.conv_rect_* (runet_conv2d_rect / runet_conv_wgrad_rect)
  tail      blocks.enet_tail_forward / _backward (runet_enet_tail_*): BatchNorm-apply, Dropout2d, add and ReLU in one pass; the plain block's
            identity gradient goes straight into the block's dx buffer and conv1's data gradient accumulates onto it (identity first)
  decoder.0 / .3   ops.convt3_*: the forward as four parity-class GEMMs over the input pixels (runet_convt3_fwd; its partner: the data gradient
            of a stride-2 3x3 convolution), the data gradient that stride-2 convolution itself, the weight gradient its weight gradient
  decoder.6 blocks.enet_head_forward / _backward (runet_enet_head_*)
The biases of decoder.0 / decoder.3 stand in front of a BatchNorm: they are kept and trained as the reference does (their gradient is zero
up to rounding in training mode).  Every gradient is summed in a fixed order (no float atomics): two steps from the same state give the same bits.

A/B switches (blocks.py): RUNET_NO_FUSED_ENET_INITIAL=1 (the initial block from runet_to_nhwc_pad, runet_conv2d_general with the weight
zero-padded to 16 columns, runet_maxpool2_fwd and runet_copy_nhwc), RUNET_NO_FUSED_ENET_TAIL=1 (the tail from runet_bn_apply,
runet_add_inplace and runet_relu_mask_nhwc); ops.py: RUNET_NO_CONVT3_CLASSES=1 (the transposed forwards through runet_conv2d_general).

Bounds: n_classes = 1 only, H and W multiples of 8, more than one value per channel at H/8 in training mode (the reference raises there too),
fp32 only, per-rank BatchNorm statistics only.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import blocks as B
from . import ops
from .baseline import FusedNet, MaxPool2d, ReLU, check_image
from .model import BatchNorm2d, Conv2d, ConvTranspose2d, Dropout2d, _Holder


class Conv2dRect(_Holder):
    """nn.Conv2d(cin, cout, (kh, kw), padding=(ph, pw), bias=False) parameter holder: weight logical [cout, cin, kh, kw], memory HWIO."""

    def __init__(self, in_channels, out_channels, kernel_size, padding=(0, 0)):
        super().__init__()
        kh, kw = kernel_size
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, (kh, kw)
        self.padding, self.dilation, self.stride = tuple(padding), (1, 1), (1, 1)
        self.weight = nn.Parameter(torch.empty(kh, kw, in_channels, out_channels).permute(3, 2, 0, 1))
        self.register_parameter("bias", None)
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))


class ConvTranspose2dK3(_Holder):
    """nn.ConvTranspose2d(cin, cout, 3, stride=2, padding=1, output_padding=1) parameter holder; weight logical [cin, cout, 3, 3], memory
    [3][3][cin][cout]."""

    TRANSPOSED_WEIGHT = True

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=2, padding=1, output_padding=1):
        super().__init__()
        assert (kernel_size, stride, padding, output_padding) == (3, 2, 1, 1)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight = nn.Parameter(torch.empty(3, 3, in_channels, out_channels).permute(2, 3, 0, 1))
        self.bias = nn.Parameter(torch.empty(out_channels))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        bound = 1.0 / math.sqrt(out_channels * 9)
        nn.init.uniform_(self.bias, -bound, bound)


class InitialBlock(_Holder):
    """Parameter layout of the reference module (:482-497); ENet carries its pass (blocks.enet_initial_forward / _backward)."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        if (in_channels, out_channels) != (3, 16):
            raise ValueError("the initial block's kernels take the reference's InitialBlock(3, 16)")
        self.conv = Conv2d(in_channels, out_channels - in_channels, 3, padding=1, bias=False, stride=2)
        self.maxpool = MaxPool2d(2, stride=2)
        self.bn = BatchNorm2d(out_channels)


class BottleneckBlock(_Holder):
    """Parameter layout of the reference module (:500-557); ENet carries its passes."""

    def __init__(self, in_channels, out_channels, dilation=1, asymmetric=False, downsample=False, dropout_prob=0.1):
        super().__init__()
        ci = in_channels // 4
        if in_channels % 16 or out_channels % 4 or ci < 4:
            raise ValueError("the kernels take an internal width in_channels // 4 that is a multiple of 4, and out_channels a multiple of 4")
        if not downsample and in_channels != out_channels:
            raise ValueError("a block that does not downsample adds its input to its output: in_channels must equal out_channels")
        self.downsample, self.in_channels, self.out_channels = downsample, in_channels, out_channels
        if downsample:
            self.maxpool = MaxPool2d(2, stride=2)
            self.conv_down = nn.Sequential(Conv2d(in_channels, out_channels, 1, bias=False), BatchNorm2d(out_channels))
        self.conv1 = nn.Sequential(Conv2d(in_channels, ci, 1, bias=False, stride=2 if downsample else 1), BatchNorm2d(ci), ReLU())
        if asymmetric:
            self.conv2 = nn.Sequential(Conv2dRect(ci, ci, (5, 1), padding=(2, 0)), BatchNorm2d(ci), ReLU(),
                                       Conv2dRect(ci, ci, (1, 5), padding=(0, 2)), BatchNorm2d(ci), ReLU())
        else:
            self.conv2 = nn.Sequential(Conv2d(ci, ci, 3, padding=dilation, dilation=dilation, bias=False), BatchNorm2d(ci), ReLU())
        self.conv3 = nn.Sequential(Conv2d(ci, out_channels, 1, bias=False), BatchNorm2d(out_channels), Dropout2d(dropout_prob))

    def handles(self):
        conv2 = [(ops.hwio(self.conv2[i].weight), self.conv2[i + 1].state(), self.conv2[i].padding, self.conv2[i].dilation)
                 for i in range(0, len(self.conv2), 3)]
        wd, bnd = (ops.hwio(self.conv_down[0].weight), self.conv_down[1].state()) if self.downsample else (None, None)
        return B.BottleneckParams(ops.hwio(self.conv1[0].weight), self.conv1[1].state(), conv2, ops.hwio(self.conv3[0].weight),
                                  self.conv3[1].state(), wd, bnd, self.conv3[2], self.out_channels)


class ENet(FusedNet):
    FP32_ONLY = "the initial-block, tail and head kernels are fp32"

    def __init__(self, n_classes=1):
        super().__init__()
        if n_classes != 1:
            raise ValueError("the fused head implements the reference's n_classes=1 sigmoid head")
        self.n_classes = n_classes
        self.initial = InitialBlock(3, 16)
        self.encoder1 = nn.Sequential(BottleneckBlock(16, 64, downsample=True, dropout_prob=0.01),
                                      *[BottleneckBlock(64, 64, dropout_prob=0.01) for _ in range(3)])
        self.encoder2 = nn.Sequential(BottleneckBlock(64, 128, downsample=True), BottleneckBlock(128, 128), BottleneckBlock(128, 128, dilation=2),
                                      BottleneckBlock(128, 128, asymmetric=True), BottleneckBlock(128, 128, dilation=4), BottleneckBlock(128, 128),
                                      BottleneckBlock(128, 128, dilation=8), BottleneckBlock(128, 128, asymmetric=True),
                                      BottleneckBlock(128, 128, dilation=16))
        self.decoder = nn.Sequential(ConvTranspose2dK3(128, 64), BatchNorm2d(64), ReLU(), ConvTranspose2dK3(64, 16), BatchNorm2d(16), ReLU(),
                                     ConvTranspose2d(16, n_classes, 2, stride=2))

    def blocks(self):
        """{block name: BottleneckBlock} in forward order"""
        return {f"{enc}.{i}": blk for enc in ("encoder1", "encoder2") for i, blk in enumerate(getattr(self, enc))}

    def set_dropout_masks(self, masks):
        """masks: {block name ("encoder1.0" ...): [N, cout] keep-mask already divided by 1 - p} or None to restore random draws."""
        for k, blk in self.blocks().items():
            blk.conv3[2].mask = None if masks is None else masks[k]

    def _check_input(self, x):
        check_image(x, 8, "three stride-2 stages that the decoder's three transposed convolutions undo", fp32=True)
        if self.training and x.shape[0] * (x.shape[2] // 8) * (x.shape[3] // 8) <= 1:
            raise ValueError("Expected more than 1 value per channel when training: encoder2's BatchNorms see N * H/8 * W/8 values per channel "
                             "(use a larger batch or image, or eval mode)")

    def _passes(self):
        return enet_forward, enet_backward


def _conv2_square(w, pad, dil):
    return w.shape[0] == w.shape[1] == 3 and pad[0] == pad[1] == dil[0] == dil[1]


def _bottleneck_forward(a, p: B.BottleneckParams, tr, sm, mask):
    """-> (out, context)"""
    down = p.wd is not None
    cx = dict(x=a, p=p, mask=mask)
    if down:
        pooled, idx = B.maxpool_forward(a)
        fs = {} if tr else None
        idn = ops.conv_fwd(pooled, p.wd, None, stats=fs)
        sd, hd, md, ivd, _ = B.bn_coeff(idn, p.bnd, tr, sm, fused=fs)
        cx.update(pooled=pooled, idx=idx, idn=idn, sd=sd, hd=hd, md=md, ivd=ivd)
        fs = None
        t = ops.conv_general_fwd(a, p.w1, None, 2, 0)
    else:
        fs = {} if tr else None
        t = ops.conv_fwd(a, p.w1, None, stats=fs)
    s, h, mean, invstd, _ = B.bn_coeff(t, p.bn1, tr, sm, fused=fs)
    stages = [dict(x=a, t=t, s=s, h=h, mean=mean, invstd=invstd)]
    b = B.bn_apply(t, s, h, None, relu=True)
    for w, bn, pad, dil in p.conv2:
        if _conv2_square(w, pad, dil):
            t = ops.conv_fwd(b, w, None, dil=dil[0])
        else:
            t = ops.conv_rect_fwd(b, w, None, 1, pad, dil)
        s, h, mean, invstd, _ = B.bn_coeff(t, bn, tr, sm)
        stages.append(dict(x=b, t=t, s=s, h=h, mean=mean, invstd=invstd))
        b = B.bn_apply(t, s, h, None, relu=True)
    fs = {} if tr else None
    t3 = ops.conv_fwd(b, p.w3, None, stats=fs)
    s3, h3, m3, i3, _ = B.bn_coeff(t3, p.bn3, tr, sm, fused=fs)
    out = B.enet_tail_forward(t3, (s3, h3), cx["idn"] if down else a, (cx["sd"], cx["hd"]) if down else None, mask)
    cx.update(stages=stages, a2=b, t3=t3, s3=s3, m3=m3, i3=i3, out=out)
    return out, cx


def _bottleneck_backward(cx, dout, G, pre, tr):
    """dout: gradient of the block's output -> gradient of its input"""
    p = cx["p"]
    down = p.wd is not None
    dev = dout.device
    dt3, did, sums3, sums_d = B.enet_tail_backward(dout, cx["out"], cx["t3"], (cx["m3"], cx["i3"], cx["s3"]), cx["idn"] if down else None,
                                                   (cx["md"], cx["ivd"], cx["sd"]) if down else None, cx["mask"], tr)
    c = p.cout
    G[pre + "conv3.1.weight"], G[pre + "conv3.1.bias"] = sums3[:c], sums3[c:]
    G[pre + "conv3.0.weight"] = ops.conv_wgrad(cx["a2"], dt3, 1, 1)
    da = ops.conv_dgrad(dt3, p.w3)
    stages = cx["stages"]
    for j in range(len(p.conv2), 0, -1):
        w, _, pad, dil = p.conv2[j - 1]
        st = stages[j]
        ci = w.shape[3]
        sums = B.vec(2 * ci, dev)
        dt = B.bn_backward(da, st["t"], st["mean"], st["invstd"], st["s"], sums, relu_shift=st["h"], out=da, training=tr)
        i = 3 * (j - 1)
        G[f"{pre}conv2.{i + 1}.weight"], G[f"{pre}conv2.{i + 1}.bias"] = sums[:ci], sums[ci:]
        if _conv2_square(w, pad, dil):
            G[f"{pre}conv2.{i}.weight"] = ops.conv_wgrad(st["x"], dt, 3, 3, dil=dil[0])
            da = ops.conv_dgrad(dt, w, dil=dil[0])
        else:
            kh, kw = w.shape[0], w.shape[1]
            G[f"{pre}conv2.{i}.weight"] = ops.conv_rect_wgrad(st["x"], dt, kh, kw, 1, pad, dil)
            da = ops.conv_rect_dgrad(dt, w, st["x"].shape[1], st["x"].shape[2], 1, pad, dil)
    st = stages[0]
    ci = p.w1.shape[3]
    sums = B.vec(2 * ci, dev)
    dt1 = B.bn_backward(da, st["t"], st["mean"], st["invstd"], st["s"], sums, relu_shift=st["h"], out=da, training=tr)
    G[pre + "conv1.1.weight"], G[pre + "conv1.1.bias"] = sums[:ci], sums[ci:]
    x = cx["x"]
    if not down:
        G[pre + "conv1.0.weight"] = ops.conv_wgrad(x, dt1, 1, 1)
        return ops.conv_dgrad(dt1, p.w1, out=did, accumulate=True)      # did holds the identity's gradient: identity first, main branch added
    G[pre + "conv1.0.weight"] = ops.conv_general_wgrad(x, dt1, 1, 1, 2, 0)
    G[pre + "conv_down.1.weight"], G[pre + "conv_down.1.bias"] = sums_d[:c], sums_d[c:]
    G[pre + "conv_down.0.weight"] = ops.conv_wgrad(cx["pooled"], did, 1, 1)
    dx = B.maxpool_backward(ops.conv_dgrad(did, p.wd), cx["idx"])
    return ops.conv_general_dgrad(dt1, p.w1, x.shape[1], x.shape[2], 2, 0, out=dx, accumulate=True)


def _convt_bn_relu(seq, i, a, tr, sm):
    w = ops.hwio_t(seq[i].weight)
    t = ops.convt3_fwd(a, w, seq[i].bias)
    s, h, mean, invstd, _ = B.bn_coeff(t, seq[i + 1].state(), tr, sm)
    return B.bn_apply(t, s, h, None, relu=True), dict(x=a, w=w, t=t, s=s, h=h, mean=mean, invstd=invstd)


def enet_forward(net: ENet, x, save=True):
    tr = net.training
    sm = B.Small(x.device)
    n = x.shape[0]
    if save:
        ops.prefetch_derived()
    ini = net.initial
    a, icx = B.enet_initial_forward(x, ops.hwio(ini.conv.weight), ini.bn.state(), tr, sm, save=save)
    L = {}
    for name, blk in net.blocks().items():
        mask = blk.conv3[2].draw(n, blk.out_channels, x.device) if tr else None
        a, cx = _bottleneck_forward(a, blk.handles(), tr, sm, mask)
        if save:
            L[name] = cx
    dec = net.decoder
    a, d0 = _convt_bn_relu(dec, 0, a, tr, sm)
    a, d3 = _convt_bn_relu(dec, 3, a, tr, sm)
    w6 = ops.hwio_t(dec[6].weight)
    prob = B.enet_head_forward(a, w6, dec[6].bias)
    C = dict(initial=icx, blocks=L, d0=d0, d3=d3, head=(a, w6, prob), training=tr) if save else None
    return prob, C


def enet_backward(net: ENet, C, dprob):
    """-> {parameter name: gradient in the parameter's PHYSICAL layout (conv weights HWIO, the transposed ones [kh, kw, cin, cout])}"""
    dev = dprob.device
    tr = C["training"]
    sink = B.DictSink(dev)
    G = sink.g
    a, w6, prob = C["head"]
    da = B.enet_head_backward(dprob, prob, a, w6, sink, "decoder.6.")
    for i, key in ((3, "d3"), (0, "d0")):
        cx = C[key]
        c = cx["t"].shape[3]
        sums = B.vec(2 * c, dev)
        dt = B.bn_backward(da, cx["t"], cx["mean"], cx["invstd"], cx["s"], sums, relu_shift=cx["h"], out=da, training=tr)
        G[f"decoder.{i + 1}.weight"], G[f"decoder.{i + 1}.bias"] = sums[:c], sums[c:]
        G[f"decoder.{i}.weight"] = ops.convt3_wgrad(cx["x"], dt)
        G[f"decoder.{i}.bias"] = B.chan_sum(dt, B.vec(c, dev))
        da = ops.convt3_dgrad(dt, cx["w"])
    for name in reversed(list(C["blocks"])):
        da = _bottleneck_backward(C["blocks"][name], da, G, name + ".", tr)
    B.enet_initial_backward(C["initial"], da, G, "initial.", tr)
    return G
