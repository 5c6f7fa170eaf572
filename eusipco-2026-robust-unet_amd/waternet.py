"""WaterNet baseline of the reference (Extended_Baseline_Comparison.py:378-473) on the gfx950 kernels.

Drop-in for the reference's `WaterIndexModule` and `WaterNet` (trained there by ModelEvaluator.train_model: nn.BCELoss, Adam 1e-4, weight decay
1e-4, :780-837): same constructor, attribute tree and state_dict.  `water_index.index_conv` (Conv2d 1x1 3 -> 16, BatchNorm2d, ReLU, Conv2d 1x1
16 -> 4, Sigmoid: four learnable NDWI / MNDWI style indices), torch.cat([x, idx]) -> a three-level U-Net on the 7 channels: `enc1..3` and
`bottleneck` (Conv2d 3x3 -> BatchNorm2d -> ReLU, twice; 64 / 128 / 256 / 512 channels, MaxPool2d(2) between), `water_attention` (the CBAM
ChannelAttention on the bottleneck), `up3..1` (ConvTranspose2d k2 s2) with cat([up, skip]) into `dec3..1`, `outc` (Conv2d 1x1 64 -> 1,
Sigmoid).  forward(x [N, 3, H, W]) -> sigmoid probabilities [N, 1, H, W].

One autograd node with an explicit backward, NHWC inside (baseline.py):
  front end     blocks.water_index_forward (csrc/water_index.hip): the image -> the 8-channel buffer [R, G, B, s0..s3, 0] in one pass, the
                16-channel tensors of the index branch recomputed per pixel in registers; backward runet_water_index_bwd_reduce / _bwd_apply
                from the gradient of channels 3..6 alone (no input gradient: the input is the image)
  enc1          its first convolution reads that buffer with cin_w = 7; its data gradient is taken for the four index channels only (the
                weight rows 3..6)
  convolutions  3x3 through ops.conv_fwd / conv_dgrad / conv_wgrad, BatchNorm statistics from the convolution's epilogue where the kernel
                offers them; BatchNorm + ReLU as the U-Net's (ReLU mask recomputed from the BatchNorm input in the backward)
  concats       never copied: the transposed convolution writes channels [0, c) of the decoder's input buffer, the encoder's last
                BatchNorm + ReLU channels [c, 2c); the pools read that half (it is needed at full resolution as the skip, so the fused
                BatchNorm + ReLU + max-pool kernel has nothing to save here)
  attention     blocks.ca_forward / ca_backward;  head blocks.outc_forward / outc_backward
The conv biases in front of a BatchNorm are kept and trained as the reference does.  Every gradient is summed in a fixed order (no float
atomics): two steps from the same state give the same bits.

A/B switch (blocks.py): RUNET_NO_FUSED_WATER_INDEX=1 (the front end in the reference's order on the shared kernels).

Bounds: n_classes = 1 only, H and W multiples of 8 (the reference's own concats fail on other sizes), fp32 only, per-rank BatchNorm statistics
only.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import blocks as B
from . import ops
from .baseline import FusedNet, MaxPool2d, ReLU, Sigmoid, check_image, conv_bn_relu
from .model import BatchNorm2d, ChannelAttention, Conv2d, ConvTranspose2d, _require_cuda

CH = (64, 128, 256)
BOTTLENECK = 512
INDEX_MID, N_INDEX = B.WI_MID, B.WI_OUT
CAT_IN = 3 + N_INDEX                  # channels enc1 sees; the buffer it reads pads them to 8
# every Sequential of the form Conv2d 3x3 -> BatchNorm2d -> ReLU, twice, in registration order: (attribute, cin, cout)
PAIRS = (("enc1", CAT_IN, 64), ("enc2", 64, 128), ("enc3", 128, 256), ("bottleneck", 256, 512), ("dec3", 512, 256), ("dec2", 256, 128),
         ("dec1", 128, 64))


def _pair(cin, cout):
    return nn.Sequential(Conv2d(cin, cout, 3, padding=1), BatchNorm2d(cout), ReLU(), Conv2d(cout, cout, 3, padding=1), BatchNorm2d(cout), ReLU())


class WaterIndexModule(nn.Module):
    """Parameter layout of the reference module (:378-393).  On its own: x [N, 3, H, W] -> the four indices [N, 4, H, W] (forward only; inside
    WaterNet the same kernels also write the concat and run the backward)."""

    def __init__(self, in_channels=3):
        super().__init__()
        if in_channels != 3:
            raise ValueError("the fused front end reads an RGB image (in_channels = 3, the reference's only use)")
        self.index_conv = nn.Sequential(Conv2d(in_channels, INDEX_MID, 1), BatchNorm2d(INDEX_MID), ReLU(), Conv2d(INDEX_MID, N_INDEX, 1), Sigmoid())

    def handles(self):
        s = self.index_conv
        return B.WaterIndexParams(ops.hwio(s[0].weight), s[0].bias, s[1].state(), ops.hwio(s[3].weight), s[3].bias)

    def forward(self, x):
        _require_cuda(x)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError("WaterIndexModule on its own is forward-only (torch.no_grad()); WaterNet carries its backward")
        buf, _ = B.water_index_forward(x, self.handles(), self.training, B.Small(x.device))
        return buf[..., 3:3 + N_INDEX].permute(0, 3, 1, 2)


class WaterNet(FusedNet):
    FP32_ONLY = "the front-end kernels are fp32"

    def __init__(self, n_classes=1):
        super().__init__()
        if n_classes != 1:
            raise ValueError("the fused head implements the reference's n_classes=1 sigmoid head")
        self.n_classes = n_classes
        self.water_index = WaterIndexModule(3)
        self.enc1, self.pool1 = _pair(CAT_IN, 64), MaxPool2d(2)
        self.enc2, self.pool2 = _pair(64, 128), MaxPool2d(2)
        self.enc3, self.pool3 = _pair(128, 256), MaxPool2d(2)
        self.bottleneck = _pair(256, BOTTLENECK)
        self.water_attention = ChannelAttention(BOTTLENECK)
        self.up3, self.dec3 = ConvTranspose2d(512, 256, 2, stride=2), _pair(512, 256)
        self.up2, self.dec2 = ConvTranspose2d(256, 128, 2, stride=2), _pair(256, 128)
        self.up1, self.dec1 = ConvTranspose2d(128, 64, 2, stride=2), _pair(128, 64)
        self.outc = nn.Sequential(Conv2d(64, n_classes, 1), Sigmoid())

    def _check_input(self, x):
        check_image(x, 8, "three 2x2 poolings whose skips are concatenated with the upsampled path", fp32=True)

    def _passes(self):
        return waternet_forward, waternet_backward


def _pair_forward(seq, x, key, tr, sm, C, out=None):
    """Conv2d 3x3 -> BatchNorm2d -> ReLU, twice; the last activation goes to `out` (a concat half) when given"""
    a = conv_bn_relu(seq, 0, x, tr, sm, C, f"{key}.0")
    return conv_bn_relu(seq, 3, a, tr, sm, C, f"{key}.3", out=out)


def waternet_forward(net: WaterNet, x, save=True):
    tr = net.training
    sm = B.Small(x.device)
    n = x.shape[0]
    C = {} if save else None
    ops.branches_pay(n, x.shape[2], x.shape[3])
    if save:
        ops.prefetch_derived()
    cur, wi = B.water_index_forward(x, net.water_index.handles(), tr, sm)
    cats, pools = {}, {}
    for lvl, ch in enumerate(CH, 1):
        _, h, w, _ = cur.shape
        cats[lvl] = ops.empty_nhwc(n, h, w, 2 * ch, cur)
        skip = cats[lvl][..., ch:]
        _pair_forward(getattr(net, f"enc{lvl}"), cur, f"enc{lvl}", tr, sm, C, out=skip)
        cur, pools[lvl] = B.maxpool_forward(skip)
    y = _pair_forward(net.bottleneck, cur, "bottleneck", tr, sm, C)
    fc = net.water_attention.fc
    y, ca = B.ca_forward(y, ops.hwio(fc[0].weight), ops.hwio(fc[2].weight), save=save)
    ups = {}
    for lvl in (3, 2, 1):
        up = getattr(net, f"up{lvl}")
        wup = ops.hwio_t(up.weight)
        ops.convt_fwd(y, wup, up.bias, out=cats[lvl][..., :CH[lvl - 1]])
        ups[lvl] = (y, wup)
        y = _pair_forward(getattr(net, f"dec{lvl}"), cats[lvl], f"dec{lvl}", tr, sm, C)
    wo = ops.hwio(net.outc[0].weight)
    prob, _ = B.outc_forward(y, wo, net.outc[0].bias)
    if save:
        C.update(wi=wi, pools=pools, ups=ups, ca=ca, head=(y, wo, prob), training=tr)
    return prob, C


def waternet_backward(net: WaterNet, C, dprob):
    """-> {parameter name: gradient in the parameter's PHYSICAL layout (conv weights HWIO, transposed-conv weights [2, 2, cin, cout])}"""
    dev = dprob.device
    tr = C["training"]
    sink = B.DictSink(dev)
    G = sink.g

    def conv_bn_relu_back(seq, i, dy, out=None):
        cx = C[f"{seq}.{i}"]
        return cx, B.conv_bn_relu_backward(cx, dy, G, seq, i, tr, out=out)

    def pair_back(seq, dy):
        """backward of a two-convolution Sequential -> (ctx of its first convolution, gradient of that convolution's output)"""
        cx, dt = conv_bn_relu_back(seq, 3, dy)
        da = ops.conv_dgrad(dt, cx["w"])
        del dt
        return conv_bn_relu_back(seq, 0, da, out=da)

    y, wo, prob = C["head"]
    dy = B.outc_backward(dprob, prob, y, wo, sink, pre="outc.0.")
    dskip = {}
    for lvl in (1, 2, 3):
        ch = CH[lvl - 1]
        cx, dt = pair_back(f"dec{lvl}", dy)
        dcat = ops.conv_dgrad(dt, cx["w"])
        del dt
        dup, dskip[lvl] = dcat[..., :ch], dcat[..., ch:]
        yin, wup = C["ups"][lvl]
        G[f"up{lvl}.weight"] = ops.convt_wgrad(yin, dup)
        G[f"up{lvl}.bias"] = B.chan_sum(dup, B.vec(ch, dev))
        dy = ops.convt_dgrad(dup, wup)
    dy = B.ca_backward(C["ca"], dy, sink, pre="water_attention.")
    cx, dt = pair_back("bottleneck", dy)
    dcur = ops.conv_dgrad(dt, cx["w"])
    del dt
    for lvl in (3, 2, 1):
        B.maxpool_backward(dcur, C["pools"][lvl], dx=dskip[lvl])          # adds the pooled path's gradient to the skip's
        cx, dt = pair_back(f"enc{lvl}", dskip[lvl])
        if lvl > 1:
            dcur = ops.conv_dgrad(dt, cx["w"])
            del dt
    # enc1's first convolution: the data gradient of the four index channels only (rows 3..6 of its weight); R, G, B are the image
    g = ops.conv_dgrad(dt, cx["w"][:, :, 3:3 + N_INDEX, :].contiguous())
    red, app = B.water_index_backward(C["wi"], g)
    pre = "water_index.index_conv."
    G[pre + "1.weight"], G[pre + "1.bias"] = red[:INDEX_MID], red[INDEX_MID:2 * INDEX_MID]
    k = 2 * INDEX_MID + INDEX_MID * N_INDEX
    G[pre + "3.weight"], G[pre + "3.bias"] = red[2 * INDEX_MID:k].view(1, 1, INDEX_MID, N_INDEX), red[k:]
    G[pre + "0.weight"], G[pre + "0.bias"] = app[:3 * INDEX_MID].view(1, 1, 3, INDEX_MID), app[3 * INDEX_MID:]
    return G
