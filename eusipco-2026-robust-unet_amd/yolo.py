"""YOLOSeg baseline of the reference (Main_Final.py:436-510) on the gfx950 kernels.

Drop-in for the reference's `YOLOSeg` (trained there like the other baselines: nn.BCELoss, Adam 1e-4, weight decay 1e-4,
Main_Final.py:551-552): same constructor, attribute tree and state_dict.  `backbone` is a Sequential of Conv2d -> BatchNorm2d ->
LeakyReLU(0.1) triples in four stages, each ending in MaxPool2d(2, 2) (3x3 convolutions, plus two 1x1 -> 3x3 pairs in stages 3 and 4);
`seg_head` is four ConvTranspose2d(k4, s2, p1) -> BatchNorm2d -> LeakyReLU(0.1) triples and Conv2d(16, n_classes, 3).
forward(x [N, 3, H, W]) -> sigmoid probabilities [N, 1, H, W].

One autograd node with an explicit backward, NHWC inside (baseline.py):
  stage end     the last BatchNorm + LeakyReLU and the pool that is its only consumer in one pass (runet_bn_leaky_maxpool2_fwd): the
                full-resolution activation is never written; backward through the pooled-gradient BatchNorm kernels
                (runet_bn_bwd_reduce_pooled_leaky / _apply_pooled_leaky), so its full-resolution gradient never exists either
  seg_head      runet_convt4_igemm_stats: the transposed convolution leaves the BatchNorm statistics partials in its epilogue, so the
                output is not read again for them (not for the last, 32 -> 16 channels, where the separate pass measured faster: ops.convt4_fwd);
                then runet_bn_apply_leaky
  head          the last conv + sigmoid = runet_head3x3_fwd / _bwd (the DeepLabV3+ head kernel)
Every other BatchNorm + LeakyReLU is runet_bn_apply_leaky forward and runet_bn_bwd_reduce_leaky / _apply_leaky backward (factor from x).
The conv biases in front of a BatchNorm are kept and trained as the reference does (their gradient is the channel sum).

A/B switches: RUNET_NO_FUSED_LEAKY_POOL=1 (apply + runet_maxpool2_fwd at the stage ends), RUNET_NO_EPILOGUE_STATS=1 (runet_bn_stats passes).

Bounds: n_classes = 1 only, H and W multiples of 16, fp32 only (the k4 transposed convolution has no bf16 / fp16 path), per-rank
BatchNorm statistics only.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import blocks as B
from . import ops
from ._lib import check, lib
from .baseline import FusedNet, MaxPool2d, check_image
from .deeplab import ConvTranspose2dK4
from .model import BatchNorm2d, Conv2d, _Act

SLOPE = 0.1         # nn.LeakyReLU(0.1) (Main_Final.py:447 etc.)

# backbone: stages of (cin, cout, kernel) convolutions, each followed by BatchNorm2d + LeakyReLU; a MaxPool2d(2, 2) ends every stage
STAGES = (((3, 32, 3),), ((32, 64, 3),), ((64, 128, 3), (128, 64, 1), (64, 128, 3)), ((128, 256, 3), (256, 128, 1), (128, 256, 3)))
DEC = ((256, 128), (128, 64), (64, 32), (32, 16))


class _LeakyReLU(_Act):
    """nn.LeakyReLU(0.1, inplace=True) stand-in (no parameters; fused into the BatchNorm kernels)."""

    def __init__(self, negative_slope=SLOPE, inplace=True):
        super().__init__()
        self.negative_slope, self.inplace = negative_slope, inplace


def _layout():
    """-> backbone index of every (conv, bn) of every stage, and of the stage's pool"""
    stages, i = [], 0
    for convs in STAGES:
        layers = []
        for _ in convs:
            layers.append((i, i + 1))
            i += 3
        stages.append((layers, i))
        i += 1
    return stages


LAYOUT = _layout()


class YOLOSeg(FusedNet):
    FP32_ONLY = "the k4 transposed convolution has no bf16 / fp16 kernels"

    def __init__(self, n_classes=1):
        super().__init__()
        if n_classes != 1:
            raise ValueError("the fused head implements the reference's n_classes=1 sigmoid head")
        self.n_classes = n_classes
        mods = []
        for convs in STAGES:
            for cin, cout, k in convs:
                mods += [Conv2d(cin, cout, k, padding=k // 2), BatchNorm2d(cout), _LeakyReLU()]
            mods.append(MaxPool2d(2))
        self.backbone = nn.Sequential(*mods)
        head = []
        for cin, cout in DEC:
            head += [ConvTranspose2dK4(cin, cout), BatchNorm2d(cout), _LeakyReLU()]
        head.append(Conv2d(16, n_classes, 3, padding=1))
        self.seg_head = nn.Sequential(*head)

    def _check_input(self, x):
        check_image(x, 16, "four 2x2 poolings")

    def _passes(self):
        return yolo_forward, yolo_backward


def yolo_forward(net: YOLOSeg, x, save=True):
    tr = net.training
    dev = x.device
    sm = B.Small(dev)
    n = x.shape[0]
    C = {}
    ops.branches_pay(n, x.shape[2], x.shape[3])
    if save:
        ops.prefetch_derived()
    cur = B.to_nhwc_pad(x, 4)
    bb = net.backbone
    for si, (layers, _) in enumerate(LAYOUT):
        for li, (ci, bi) in enumerate(layers):
            conv, bn = bb[ci], bb[bi]
            t, s, h, cx = B.conv_bn_coeff(cur, ops.hwio(conv.weight), conv.bias, bn.state(), tr, sm, save=save)
            if save:
                C[ci] = cx
                cx["cin_w"] = cx["w"].shape[2]
            if li + 1 < len(layers):
                cur = B.bn_apply_leaky(t, s, h, SLOPE)
            else:
                cur, idx = B.bn_leaky_maxpool_forward(t, s, h, SLOPE)
                if save:
                    cx["idx"] = idx
    sh = net.seg_head
    for i in range(len(DEC)):
        ct, bn = sh[3 * i], sh[3 * i + 1]
        w = ops.hwio_t(ct.weight)
        fs = {} if tr else None
        raw = ops.convt4_fwd(cur, w, ct.bias, stats=fs)
        s, h, mean, invstd, _ = B.bn_coeff(raw, bn.state(), tr, sm, fused=fs)
        if save:
            C[f"dec{i}"] = dict(x=cur, w=w, t=raw, s=s, h=h, mean=mean, invstd=invstd)
        cur = B.bn_apply_leaky(raw, s, h, SLOPE)
    head = sh[3 * len(DEC)]
    wh = ops.hwio(head.weight)
    _, hh, ww, c = cur.shape
    prob = torch.empty((n, 1, hh, ww), device=dev, dtype=torch.float32)
    check(lib.runet_head3x3_fwd(cur.data_ptr(), ops.ld(cur), wh.data_ptr(), head.bias.data_ptr(), prob.data_ptr(), n, hh, ww, c, ops.stream()))
    if save:
        C["head"] = (cur, wh, prob)
        C["training"] = tr
    return prob, (C if save else None)


def yolo_backward(net: YOLOSeg, C, dprob):
    """-> {parameter name: gradient in the parameter's PHYSICAL layout (conv weights HWIO, transposed-conv weights [4, 4, cin, cout])}"""
    G = {}
    dev = dprob.device
    tr = C["training"]
    y, wh, prob = C["head"]
    n, hh, ww, c = y.shape
    dy = ops.empty_nhwc(n, hh, ww, c, y)
    dwdb = B.vec(9 * c + 1, dev)
    wsb = B.scratch(lib.runet_head3x3_bwd_workspace_floats(n, hh, ww, c), dev)
    check(lib.runet_head3x3_bwd(dprob.data_ptr(), prob.data_ptr(), y.data_ptr(), ops.ld(y), wh.data_ptr(), dy.data_ptr(), ops.ld(dy), wsb.data_ptr(),
                                dwdb.data_ptr(), n, hh, ww, c, ops.stream()))
    hi = 3 * len(DEC)
    G[f"seg_head.{hi}.weight"] = dwdb[:9 * c].view(3, 3, c, 1)
    G[f"seg_head.{hi}.bias"] = dwdb[9 * c:]
    for i in reversed(range(len(DEC))):
        cx = C[f"dec{i}"]
        cout = cx["t"].shape[3]
        sums = B.vec(2 * cout, dev)
        draw = B.bn_backward_leaky(dy, cx["t"], cx["mean"], cx["invstd"], cx["s"], sums, cx["h"], SLOPE, training=tr)
        G[f"seg_head.{3 * i + 1}.weight"], G[f"seg_head.{3 * i + 1}.bias"] = sums[:cout], sums[cout:]
        G[f"seg_head.{3 * i}.weight"] = ops.convt4_wgrad(cx["x"], draw)
        G[f"seg_head.{3 * i}.bias"] = B.chan_sum(draw, B.vec(cout, dev))
        dy = ops.convt4_dgrad(draw, cx["w"])
        del draw
    for si in reversed(range(len(LAYOUT))):
        layers, _ = LAYOUT[si]
        for li in reversed(range(len(layers))):
            ci, bi = layers[li]
            cx = C[ci]
            cout = cx["t"].shape[3]
            sums = B.vec(2 * cout, dev)
            if li + 1 == len(layers):
                dt = B.bn_backward_pooled_leaky(dy, cx["idx"], cx["t"], cx["mean"], cx["invstd"], cx["s"], sums, cx["h"], SLOPE, training=tr)
            else:
                dt = B.bn_backward_leaky(dy, cx["t"], cx["mean"], cx["invstd"], cx["s"], sums, cx["h"], SLOPE, training=tr, out=dy)
            G[f"backbone.{bi}.weight"], G[f"backbone.{bi}.bias"] = sums[:cout], sums[cout:]
            first = si == 0 and li == 0
            k = cx["w"].shape[0]
            G[f"backbone.{ci}.weight"] = ops.conv_wgrad(cx["x"], dt, k, k, cin_w=cx["cin_w"], on_side=not first)
            G[f"backbone.{ci}.bias"] = B.chan_sum(dt, B.vec(cout, dev))
            if not first:
                dy = ops.conv_dgrad(dt, cx["w"])
            del dt
    return G
