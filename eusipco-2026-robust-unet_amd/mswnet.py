"""MSWNet baseline of the reference (Extended_Baseline_Comparison.py:479-548) on the gfx950 kernels.

Drop-in for the reference's `MultiScaleBlock` and `MSWNet` (trained there by ModelEvaluator.train_model: nn.BCELoss, Adam 1e-4, weight decay
1e-4, :780-837): same constructor, attribute tree and state_dict.  `enc1..4` are MultiScaleBlocks (3 -> 64 -> 128 -> 256 -> 512): four parallel
branches on one input - Conv2d 1x1, Conv2d 3x3, Conv2d 5x5, MaxPool2d(3, 1, 1) -> Conv2d 1x1, each followed by BatchNorm2d and ReLU at a quarter
of the block's channels - concatenated; MaxPool2d(2) between the levels; `bridge` (Conv2d 3x3 -> BatchNorm2d -> ReLU twice, 512 -> 1024 -> 1024);
`up4..1` (ConvTranspose2d k2 s2) with cat([up, skip]) into `dec4..1` (one Conv2d 3x3 -> BatchNorm2d -> ReLU each); `outc` (Conv2d 1x1 64 -> 1,
Sigmoid).  forward(x [N, 3, H, W]) -> sigmoid probabilities [N, 1, H, W].

One autograd node with an explicit backward, NHWC inside (baseline.py):
  enc1          blocks.ms_stem_forward (csrc/multiscale.hip): the image -> the 64-channel activation in one pass, the pre-BatchNorm tensor
                recomputed per pixel and never written; backward runet_ms_stem_bwd_reduce / _bwd_apply, the four weight gradients from the
                apply kernel's output on a 4-channel NHWC copy of the image (no input gradient: the input is the image)
  enc2..4       blocks.ms_block_forward: the four convolutions (ops.conv_fwd, the 5x5 through ops.conv_general_fwd) write channel slices of one
                buffer, branch4 reads runet_maxpool3s1_fwd of the input; one BatchNorm + ReLU apply and one BatchNorm backward over the concat
                (the four BatchNorms' vectors back to back); the input gradient summed in a fixed order (1x1, 3x3, 5x5, the pool's gather)
  concats       never copied: the transposed convolution writes channels [0, c) of the decoder's input buffer, the encoder block's BatchNorm +
                ReLU channels [c, 2c); the 2x2 pools read that half
  bridge, dec   3x3 through ops.conv_fwd / conv_dgrad / conv_wgrad, BatchNorm statistics from the convolution's epilogue where offered
  head          blocks.outc_forward / outc_backward
The conv biases in front of a BatchNorm are kept and trained as the reference does.  Every gradient is summed in a fixed order (no float
atomics): two steps from the same state give the same bits.

A/B switch (blocks.py): RUNET_NO_FUSED_MS_STEM=1 (enc1 takes enc2..4's path on a 4-channel NHWC copy of the image).

Bounds: n_classes = 1 only, H and W multiples of 16 (the reference's own concats fail on other sizes), fp32 only, per-rank BatchNorm statistics
only.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import blocks as B
from . import ops
from .baseline import FusedNet, MaxPool2d, ReLU, Sigmoid, check_image, conv_bn_relu
from .model import BatchNorm2d, Conv2d, ConvTranspose2d, _require_cuda

CH = (64, 128, 256, 512)
BRIDGE = 1024


class MultiScaleBlock(nn.Module):
    """Parameter layout of the reference module (:479-494).  On its own: x [N, Cin, H, W] -> [N, Cout, H, W], forward only (inside MSWNet the
    same kernels also write the concat buffers and run the backward)."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        if out_channels % 4 or out_channels < 4:
            raise ValueError("out_channels must be a positive multiple of 4 (four branches of out_channels // 4)")
        q = out_channels // 4
        self.in_channels, self.out_channels = in_channels, out_channels
        self.branch1 = nn.Sequential(Conv2d(in_channels, q, 1), BatchNorm2d(q), ReLU())
        self.branch2 = nn.Sequential(Conv2d(in_channels, q, 3, padding=1), BatchNorm2d(q), ReLU())
        self.branch3 = nn.Sequential(Conv2d(in_channels, q, 5, padding=2), BatchNorm2d(q), ReLU())
        self.branch4 = nn.Sequential(MaxPool2d(3, stride=1, padding=1), Conv2d(in_channels, q, 1), BatchNorm2d(q), ReLU())

    def handles(self):
        convs = (self.branch1[0], self.branch2[0], self.branch3[0], self.branch4[1])
        bns = (self.branch1[1], self.branch2[1], self.branch3[1], self.branch4[2])
        return B.MSBlockParams([ops.hwio(c.weight) for c in convs], [c.bias for c in convs], [b.state() for b in bns])

    def forward(self, x):
        _require_cuda(x)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError("MultiScaleBlock on its own is forward-only (torch.no_grad()); MSWNet carries its backward")
        if x.dim() != 4 or x.shape[1] != self.in_channels or x.dtype != torch.float32:
            raise ValueError(f"expected a float32 x [N, {self.in_channels}, H, W]")
        sm = B.Small(x.device)
        with ops.precision("f32"):
            if self.in_channels == 3 and self.out_channels == B.MS_STEM_C:
                e, _ = B.ms_stem_forward(x, self.handles(), self.training, sm, save=False)
            else:
                c_pad = (self.in_channels + 3) // 4 * 4
                e, _ = B.ms_block_forward(B.to_nhwc_pad(x, c_pad), self.handles(), self.training, sm, save=False)
        return e.permute(0, 3, 1, 2)


def _cbr(cin, cout):
    return [Conv2d(cin, cout, 3, padding=1), BatchNorm2d(cout), ReLU()]


class MSWNet(FusedNet):
    FP32_ONLY = "the multi-scale stem and pool kernels are fp32"

    def __init__(self, n_classes=1):
        super().__init__()
        if n_classes != 1:
            raise ValueError("the fused head implements the reference's n_classes=1 sigmoid head")
        self.n_classes = n_classes
        self.enc1 = MultiScaleBlock(3, 64)
        self.enc2 = MultiScaleBlock(64, 128)
        self.enc3 = MultiScaleBlock(128, 256)
        self.enc4 = MultiScaleBlock(256, 512)
        self.pool = MaxPool2d(2)
        self.bridge = nn.Sequential(*_cbr(512, BRIDGE), *_cbr(BRIDGE, BRIDGE))
        self.up4, self.dec4 = ConvTranspose2d(1024, 512, 2, stride=2), nn.Sequential(*_cbr(1024, 512))
        self.up3, self.dec3 = ConvTranspose2d(512, 256, 2, stride=2), nn.Sequential(*_cbr(512, 256))
        self.up2, self.dec2 = ConvTranspose2d(256, 128, 2, stride=2), nn.Sequential(*_cbr(256, 128))
        self.up1, self.dec1 = ConvTranspose2d(128, 64, 2, stride=2), nn.Sequential(*_cbr(128, 64))
        self.outc = nn.Sequential(Conv2d(64, n_classes, 1), Sigmoid())

    def _check_input(self, x):
        check_image(x, 16, "four 2x2 poolings whose skips are concatenated with the upsampled path", fp32=True)

    def _passes(self):
        return mswnet_forward, mswnet_backward


def mswnet_forward(net: MSWNet, x, save=True):
    tr = net.training
    sm = B.Small(x.device)
    n, _, h, w = x.shape
    C = {} if save else None
    ops.branches_pay(n, h, w)
    if save:
        ops.prefetch_derived()
    cats, pools, encs = {}, {}, {}
    cur = None
    for lvl, ch in enumerate(CH, 1):
        hl, wl = h >> (lvl - 1), w >> (lvl - 1)
        cats[lvl] = torch.empty((n, hl, wl, 2 * ch), device=x.device, dtype=torch.float32)
        skip = cats[lvl][..., ch:]
        p = getattr(net, f"enc{lvl}").handles()
        if lvl == 1:
            _, encs[lvl] = B.ms_stem_forward(x, p, tr, sm, out=skip, save=save)
        else:
            _, encs[lvl] = B.ms_block_forward(cur, p, tr, sm, out=skip, save=save)
        cur, pools[lvl] = B.maxpool_forward(skip)
    y = conv_bn_relu(net.bridge, 0, cur, tr, sm, C, "bridge.0")
    y = conv_bn_relu(net.bridge, 3, y, tr, sm, C, "bridge.3")
    ups = {}
    for lvl in (4, 3, 2, 1):
        up = getattr(net, f"up{lvl}")
        wup = ops.hwio_t(up.weight)
        ops.convt_fwd(y, wup, up.bias, out=cats[lvl][..., :CH[lvl - 1]])
        ups[lvl] = (y, wup)
        y = conv_bn_relu(getattr(net, f"dec{lvl}"), 0, cats[lvl], tr, sm, C, f"dec{lvl}.0")
    wo = ops.hwio(net.outc[0].weight)
    prob, _ = B.outc_forward(y, wo, net.outc[0].bias)
    if save:
        C.update(encs=encs, pools=pools, ups=ups, head=(y, wo, prob), training=tr)
    return prob, C


def mswnet_backward(net: MSWNet, C, dprob):
    """-> {parameter name: gradient in the parameter's PHYSICAL layout (conv weights HWIO, transposed-conv weights [2, 2, cin, cout])}"""
    dev = dprob.device
    tr = C["training"]
    sink = B.DictSink(dev)
    G = sink.g

    def cbr_back(seq, i, dy):
        cx = C[f"{seq}.{i}"]
        return cx, B.conv_bn_relu_backward(cx, dy, G, seq, i, tr, out=dy)

    y, wo, prob = C["head"]
    dy = B.outc_backward(dprob, prob, y, wo, sink, pre="outc.0.")
    dskip = {}
    for lvl in (1, 2, 3, 4):
        ch = CH[lvl - 1]
        cx, dt = cbr_back(f"dec{lvl}", 0, dy)
        dcat = ops.conv_dgrad(dt, cx["w"])
        del dt
        dup, dskip[lvl] = dcat[..., :ch], dcat[..., ch:]
        yin, wup = C["ups"][lvl]
        G[f"up{lvl}.weight"] = ops.convt_wgrad(yin, dup)
        G[f"up{lvl}.bias"] = B.chan_sum(dup, B.vec(ch, dev))
        dy = ops.convt_dgrad(dup, wup)
    cx, dt = cbr_back("bridge", 3, dy)
    da = ops.conv_dgrad(dt, cx["w"])
    del dt
    cx, dt = cbr_back("bridge", 0, da)
    dcur = ops.conv_dgrad(dt, cx["w"])
    del dt
    for lvl in (4, 3, 2, 1):
        B.maxpool_backward(dcur, C["pools"][lvl], dx=dskip[lvl])          # adds the pooled path's gradient to the skip's
        if lvl > 1:
            dcur = B.ms_block_backward(C["encs"][lvl], dskip[lvl], G, pre=f"enc{lvl}.")
        else:
            B.ms_stem_backward(C["encs"][lvl], dskip[lvl], G, pre="enc1.")
    return G
