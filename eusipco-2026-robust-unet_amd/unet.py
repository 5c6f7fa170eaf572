"""Plain 2-class U-Net of the reference's older trainer on the gfx950 kernels.

Drop-in for `UNet` in /root/reference/train_water_segmentation.py:209-288 (the model `predict_coastline.py:351` loads): same
constructor, attribute tree and state_dict (enc1..4 / bottleneck / dec4..1 = Sequential(Conv2d(3x3, bias), BatchNorm2d, ReLU, Conv2d,
BatchNorm2d, ReLU), upconv4..1 = ConvTranspose2d(k2, s2), final = Conv2d(64, n_classes, 1), pool), forward(x [N, 3, H, W]) ->
logits [N, n_classes, H, W]; trained with nn.CrossEntropyLoss on int64 masks (:304) - `ops.cross_entropy` is the fused equivalent.

Built from the Robust U-Net path's kernels: 3x3 convolutions (Winograd / implicit GEMM / bf16), BatchNorm +
ReLU, 2x2 max-pool, k2-s2 transposed convolution.  As there, the whole network is ONE autograd node with an explicit backward (baseline.py);
`torch.cat([upsampled, skip])` is never materialised: the encoder block writes its output straight into the right half of the
decoder's input buffer and the transposed convolution into the left half.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import blocks as B
from . import ops
from ._lib import check, lib
from .baseline import FusedNet
from .model import BatchNorm2d, Conv2d, ConvTranspose2d, _Act

CH = (64, 128, 256, 512)


def _conv_block(cin, cout):
    return nn.Sequential(Conv2d(cin, cout, 3, padding=1), BatchNorm2d(cout), _Act(), Conv2d(cout, cout, 3, padding=1), BatchNorm2d(cout), _Act())


class _Pool(nn.Module):
    def __init__(self):
        super().__init__()
        self.kernel_size, self.stride = 2, 2

    def forward(self, x):
        from .model import MaxPool2d
        return MaxPool2d(2)(x)


class UNet(FusedNet):
    PRECISIONS = ops.PRECISIONS

    def __init__(self, n_channels=3, n_classes=2):
        super().__init__()
        if not 1 <= n_classes <= 4:
            # the reference takes any n_classes; this head is a 64 -> 4 padded 1x1 GEMM (channel quads) and ops.cross_entropy takes 2..8
            # classes, so 1..4 run here (the reference trains 2); INTEGRATION.md states the bound
            raise ValueError("the fused head handles 1..4 classes (the reference uses 2)")
        self.n_channels, self.n_classes = n_channels, n_classes
        self.enc1 = _conv_block(n_channels, 64)
        self.enc2 = _conv_block(64, 128)
        self.enc3 = _conv_block(128, 256)
        self.enc4 = _conv_block(256, 512)
        self.bottleneck = _conv_block(512, 1024)
        self.upconv4 = ConvTranspose2d(1024, 512, 2, stride=2)
        self.dec4 = _conv_block(1024, 512)
        self.upconv3 = ConvTranspose2d(512, 256, 2, stride=2)
        self.dec3 = _conv_block(512, 256)
        self.upconv2 = ConvTranspose2d(256, 128, 2, stride=2)
        self.dec2 = _conv_block(256, 128)
        self.upconv1 = ConvTranspose2d(128, 64, 2, stride=2)
        self.dec1 = _conv_block(128, 64)
        self.final = Conv2d(64, n_classes, 1)
        self.pool = _Pool()

    def _check_input(self, x):
        if x.shape[2] % 16 or x.shape[3] % 16:                # no channel check: n_channels is a constructor argument
            raise ValueError("H and W must be multiples of 16 (four 2x2 poolings)")

    def _passes(self):
        return unet_forward, unet_backward


# ------------------------------------------------------------------------------------------------------------ blocks
def _triples(seq):
    """(conv, bn) of each Conv2d(3x3) -> BatchNorm2d -> ReLU triple at the start of a Sequential (a trailing conv without BatchNorm is
    the caller's)."""
    k = sum(isinstance(m, BatchNorm2d) for m in seq)
    return [(seq[3 * i], seq[3 * i + 1]) for i in range(k)]


def _block_forward(x, seq, training, sm, out=None, save=True, tail=None):
    """Any number of Conv3x3 -> BatchNorm -> ReLU triples.  The last BatchNorm + ReLU is bn_apply into `out`, or tail(t, scale, shift) when
    given (a fused consumer: SegNet's encoder ends pool there).  ctx keys: x, w1.., t1.., a1.. (all but the last activation), s/h/mean/invstd1.."""
    layers = _triples(seq)
    k = len(layers)
    ctx = dict(x=x, training=training, k=k) if save else None
    cur = x
    for i, (conv, bn) in enumerate(layers, 1):
        w = ops.hwio(conv.weight)
        t = ops.conv_fwd(cur, w, conv.bias)
        s, h, mean, invstd, _ = B.bn_coeff(t, bn.state(), training, sm)
        if i < k:
            cur = B.bn_apply(t, s, h, None, relu=True)
        elif tail is not None:
            cur = tail(t, s, h)
        else:
            cur = B.bn_apply(t, s, h, None, relu=True, out=out)
        if save:
            ctx.update({f"w{i}": w, f"t{i}": t, f"s{i}": s, f"h{i}": h, f"mean{i}": mean, f"invstd{i}": invstd})
            if i == 1:
                ctx["cin_w"] = w.shape[2]
            if i < k:
                ctx[f"a{i}"] = cur
    return cur, ctx


def _block_backward(c, dout, G, pre, need_dx=True, tail_bwd=None):
    """Backward of _block_forward: parameter gradients (physical layouts) into G under `pre`.  tail_bwd(dout, t, mean, invstd, scale, sums,
    shift, training) -> dt replaces the last BatchNorm + ReLU backward when the forward fused its consumer."""
    dev = dout.device
    k = c["k"]
    d = dout
    for i in range(k, 0, -1):
        cout = c[f"w{i}"].shape[3]
        sums = B.vec(2 * cout, dev)
        if i == k and tail_bwd is not None:
            dt = tail_bwd(d, c[f"t{i}"], c[f"mean{i}"], c[f"invstd{i}"], c[f"s{i}"], sums, c[f"h{i}"], c["training"])
        elif i == k:
            dt = B.bn_backward(d, c[f"t{i}"], c[f"mean{i}"], c[f"invstd{i}"], c[f"s{i}"], sums, relu_shift=c[f"h{i}"], training=c["training"])
        else:
            dt = B.bn_backward(d, c[f"t{i}"], c[f"mean{i}"], c[f"invstd{i}"], c[f"s{i}"], sums, relu_shift=c[f"h{i}"], out=d, training=c["training"])
        G[f"{pre}.{3 * i - 2}.weight"], G[f"{pre}.{3 * i - 2}.bias"] = sums[:cout], sums[cout:]
        if i > 1:
            G[f"{pre}.{3 * i - 3}.weight"] = ops.conv_wgrad(c[f"a{i - 1}"], dt, 3, 3)
            G[f"{pre}.{3 * i - 3}.bias"] = B.chan_sum(dt, B.vec(cout, dev))
            d = ops.conv_dgrad(dt, c[f"w{i}"])
            del dt
        else:
            G[f"{pre}.0.weight"] = ops.conv_wgrad(c["x"], dt, 3, 3, cin_w=c["cin_w"], on_side=need_dx)
            G[f"{pre}.0.bias"] = B.chan_sum(dt, B.vec(cout, dev))
            return ops.conv_dgrad(dt, c["w1"]) if need_dx else None


def _head_weights(net):
    """final (64 -> n_classes, 1x1) zero-padded to 4 output channels: the implicit-GEMM kernels work on channel quads."""
    w = ops.hwio(net.final.weight)                      # [1, 1, 64, classes]
    w4 = torch.zeros((1, 1, w.shape[2], 4), device=w.device, dtype=torch.float32)
    w4[..., :net.n_classes].copy_(w)
    b4 = torch.zeros(4, device=w.device, dtype=torch.float32)
    b4[:net.n_classes].copy_(net.final.bias.detach())
    return w4, b4


def unet_forward(net: UNet, x, save=True, nhwc=False):
    """nhwc=False: x [N, C, H, W] -> logits [N, classes, H, W] (what UNet.forward returns).  nhwc=True (the prediction path, predict.py):
    x is the stem's own input, [N, H, W, channels padded to 4] as runet_scene_to_tiles writes it, and the head's NHWC output z4
    [N, H, W, 4] (n_classes valid) is returned as it stands - no NCHW tensor on either side."""
    tr = net.training
    dev = x.device
    sm = B.Small(dev)
    n = x.shape[0]
    C = {}
    c_pad = (net.n_channels + 3) // 4 * 4
    if nhwc:
        if x.dim() != 4 or x.shape[3] != c_pad or not x.is_contiguous() or x.dtype != torch.float32:
            raise ValueError(f"nhwc input must be a contiguous float32 [N, H, W, {c_pad}] tensor")
        if x.shape[1] % 16 or x.shape[2] % 16:
            raise ValueError("H and W must be multiples of 16 (four 2x2 poolings)")
    ops.branches_pay(n, *(x.shape[1:3] if nhwc else x.shape[2:4]))
    if save:
        ops.prefetch_derived()
    cur = x if nhwc else B.to_nhwc_pad(x, c_pad)
    cats = {}
    for lvl, ch in enumerate(CH, 1):
        _, h, w, _ = cur.shape
        cat = ops.empty_nhwc(n, h, w, 2 * ch, cur)
        skip = cat[..., ch:]
        _, C[f"enc{lvl}"] = _block_forward(cur, getattr(net, f"enc{lvl}"), tr, sm, out=skip, save=save)
        cats[lvl] = cat
        cur, C[f"pool{lvl}"] = B.maxpool_forward(skip)
    y, C["bottleneck"] = _block_forward(cur, net.bottleneck, tr, sm, save=save)
    for lvl in (4, 3, 2, 1):
        up = getattr(net, f"upconv{lvl}")
        ch = CH[lvl - 1]
        wup = ops.hwio_t(up.weight)
        ops.convt_fwd(y, wup, up.bias, out=cats[lvl][..., :ch])
        if save:
            C[f"up{lvl}"] = (y, wup)
        y, C[f"dec{lvl}"] = _block_forward(cats[lvl], getattr(net, f"dec{lvl}"), tr, sm, save=save)
    w4, b4 = _head_weights(net)
    z4 = ops.conv_fwd(y, w4, b4)
    if nhwc:
        return z4, None
    _, h, w, _ = z4.shape
    logits = torch.empty((n, net.n_classes, h, w), device=dev, dtype=torch.float32)
    check(lib.runet_nhwc_to_nchw(z4.data_ptr(), 4, logits.data_ptr(), n, net.n_classes, h * w, ops.stream()))
    if save:
        C["head"] = (y, w4)
    return logits, (C if save else None)


def unet_backward(net: UNet, C, dlogits):
    """-> {parameter name: gradient in the parameter's PHYSICAL layout}"""
    G = {}
    dev = dlogits.device
    y, w4 = C["head"]
    k = net.n_classes
    dz4 = B.to_nhwc_pad(dlogits.contiguous(), 4)
    G["final.weight"] = ops.conv_wgrad(y, dz4, 1, 1, on_side=False)[..., :k].contiguous()
    G["final.bias"] = B.chan_sum(dz4, B.vec(4, dev))[:k]
    dy = ops.conv_dgrad(dz4, w4)
    dskip = {}
    for lvl in (1, 2, 3, 4):
        ch = CH[lvl - 1]
        dcat = _block_backward(C[f"dec{lvl}"], dy, G, f"dec{lvl}")
        dup, dskip[lvl] = dcat[..., :ch], dcat[..., ch:]
        yin, wup = C[f"up{lvl}"]
        G[f"upconv{lvl}.weight"] = ops.convt_wgrad(yin, dup)
        G[f"upconv{lvl}.bias"] = B.chan_sum(dup, B.vec(ch, dev))
        dy = ops.convt_dgrad(dup, wup)
    dcur = _block_backward(C["bottleneck"], dy, G, "bottleneck")
    for lvl in (4, 3, 2, 1):
        B.maxpool_backward(dcur, C[f"pool{lvl}"], dx=dskip[lvl])          # adds the pooled path's gradient to the skip's
        dcur = _block_backward(C[f"enc{lvl}"], dskip[lvl], G, f"enc{lvl}", need_dx=lvl > 1)
    return G
