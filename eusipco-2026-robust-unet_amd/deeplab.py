"""`DeepLabV3Plus` baseline of the reference (Main_Final.py:325-433, duplicated in Extended_Baseline_Comparison.py:293-337) on the same
gfx950 kernels as the Robust U-Net path (BASELINE.json config 4: "shared implicit-GEMM conv kernels").  Same constructor, attribute tree and
state_dict keys as the reference; the forward returns sigmoid probabilities like the reference's `torch.sigmoid(x)`.

Geometry beyond the U-Net's: Conv2d 7x7 stride 2, 3x3 stride 2, 3x3 dilation 6/12/18, MaxPool2d(3, s2, p1),
global-average-pool -> 1x1 conv -> bilinear upsample of a 1x1 map (= broadcast), ConvTranspose2d(k4, s2, p1) and a
Conv2d(16, 1, 3) head.  One autograd node with an explicit backward, NHWC fp32 inside (baseline.py); conv1..conv4 are the shared
Conv2d -> BatchNorm2d -> ReLU step with the BatchNorm statistics from bn_coeff's own pass (stats=False).  `ASPP` is also callable on its own.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import blocks as B
from . import ops
from ._lib import check, lib
from .baseline import FusedNet, check_image, conv_bn_relu
from .model import BatchNorm2d, Conv2d, _Act, _Holder, _logical, _require_cuda


class ConvTranspose2dK4(_Holder):
    """ConvTranspose2d(cin, cout, 4, stride=2, padding=1) parameter holder; weight logical [cin, cout, 4, 4], memory [4][4][cin][cout]."""

    TRANSPOSED_WEIGHT = True

    def __init__(self, in_channels, out_channels, kernel_size=4, stride=2, padding=1):
        super().__init__()
        assert (kernel_size, stride, padding) == (4, 2, 1)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight = nn.Parameter(torch.empty(4, 4, in_channels, out_channels).permute(2, 3, 0, 1))
        self.bias = nn.Parameter(torch.empty(out_channels))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        bound = 1.0 / math.sqrt(out_channels * 16)
        nn.init.uniform_(self.bias, -bound, bound)


class _MaxPool3(_Holder):
    pass


class ASPP(nn.Module):
    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv1 = Conv2d(in_channels, out_channels, 1)
        self.conv2 = Conv2d(in_channels, out_channels, 3, padding=6, dilation=6)
        self.conv3 = Conv2d(in_channels, out_channels, 3, padding=12, dilation=12)
        self.conv4 = Conv2d(in_channels, out_channels, 3, padding=18, dilation=18)
        self.global_pool = _Act()
        self.conv5 = Conv2d(in_channels, out_channels, 1)
        self.conv_out = Conv2d(out_channels * 5, out_channels, 1)
        self.bn = BatchNorm2d(out_channels)

    def forward(self, x):
        """Standalone call (inside DeepLabV3Plus the same kernel sequence runs as part of the network's single autograd node)."""
        _require_cuda(x)
        return _ASPPFn.apply(x, self, *[p for _, p in self.named_parameters()])


class _ASPPFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mod, *params):
        xn = x.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)
        out, ctx.c = aspp_forward(mod, xn, mod.training, B.Small(x.device))
        ctx.mod = mod
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dy):
        G = {}
        dx = aspp_backward(ctx.c, dy.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1), G, "")
        ctx.c = None
        return (dx.permute(0, 3, 1, 2), None) + tuple(_logical(G[k], False) for k, _ in ctx.mod.named_parameters())


class DeepLabV3Plus(FusedNet):
    """forward(x: float32 [N, 3, H, W], H and W multiples of 16) -> sigmoid probabilities [N, 1, H, W]."""

    FP32_ONLY = "the general-geometry, transposed k4 and head kernels are fp32"
    DEC = ((256, 128), (128, 64), (64, 32), (32, 16))

    def __init__(self, n_classes=1):
        super().__init__()
        if n_classes != 1:
            raise ValueError("the fused head implements the reference's n_classes=1 sigmoid head")
        self.conv1 = nn.Sequential(Conv2d(3, 64, 7, padding=3, stride=2), BatchNorm2d(64), _Act())
        self.conv2 = nn.Sequential(_MaxPool3(), Conv2d(64, 128, 3, padding=1), BatchNorm2d(128), _Act())
        self.conv3 = nn.Sequential(Conv2d(128, 256, 3, padding=1, stride=2), BatchNorm2d(256), _Act())
        self.conv4 = nn.Sequential(Conv2d(256, 512, 3, padding=1, stride=2), BatchNorm2d(512), _Act())
        self.aspp = ASPP(512, 256)
        dec = []
        for cin, cout in self.DEC:
            dec += [ConvTranspose2dK4(cin, cout), BatchNorm2d(cout), _Act()]
        dec.append(Conv2d(16, n_classes, 3, padding=1))
        self.decoder = nn.Sequential(*dec)

    def _check_input(self, x):
        check_image(x, 16, "four stride-2 stages that the decoder's four transposed convolutions undo")

    def _passes(self):
        return deeplab_forward, deeplab_backward


def _bn_relu(x, w, t, bn, tr, sm):
    """t = (transposed) conv of x by w -> BatchNorm2d `bn` -> ReLU.  -> (activation, context: blocks.conv_bn_relu_forward's keys)"""
    s, h, mean, invstd, _ = B.bn_coeff(t, bn.state(), tr, sm)
    return B.bn_apply(t, s, h, None, relu=True), dict(x=x, w=w, t=t, s=s, h=h, mean=mean, invstd=invstd)


def _bn_relu_backward(cx, dy, G, bn, tr, out=None):
    """Backward of _bn_relu's BatchNorm + ReLU: the BatchNorm's gradients into G as {bn}.weight / .bias, -> gradient of t (out=dy: in place)"""
    c = cx["t"].shape[3]
    sums = B.vec(2 * c, dy.device)
    dt = B.bn_backward(dy, cx["t"], cx["mean"], cx["invstd"], cx["s"], sums, relu_shift=cx["h"], out=out, training=tr)
    G[bn + ".weight"], G[bn + ".bias"] = sums[:c], sums[c:]
    return dt


def _conv_grads(G, name, dw, dt):
    """Files a convolution's gradients into G: its weight gradient dw (physical layout) and its bias gradient, dt summed per channel."""
    G[name + ".weight"] = dw
    G[name + ".bias"] = B.chan_sum(dt, B.vec(dt.shape[3], dt.device))


def aspp_forward(asp: ASPP, a4, tr, sm):
    """ASPP (Main_Final.py:325-357) on an NHWC tensor: four parallel convolutions (1x1, 3x3 dilation 6 / 12 / 18) + the image-pooling branch,
    written into fifths of one buffer, then the 1x1 output convolution + BatchNorm + ReLU.  -> (out, ctx)"""
    n, h4, w4, c4 = a4.shape
    q = asp.conv1.out_channels
    cat = ops.empty_nhwc(n, h4, w4, 5 * q, a4)
    ws = [ops.hwio(c.weight) for c in (asp.conv1, asp.conv2, asp.conv3, asp.conv4, asp.conv5, asp.conv_out)]
    ops.conv_fwd(a4, ws[0], asp.conv1.bias, out=cat[..., 0:q])
    for i, (cv, d) in enumerate(((asp.conv2, 6), (asp.conv3, 12), (asp.conv4, 18))):
        ops.conv_general_fwd(a4, ws[1 + i], cv.bias, 1, d, d, out=cat[..., (1 + i) * q:(2 + i) * q])
    pooled, m2 = sm.f(n * c4), sm.f(n * c4)
    wsp = B._ws(n, h4 * w4, c4, a4.device)
    check(lib.runet_chan_stats(a4.data_ptr(), ops.ld(a4), n, h4 * w4, c4, wsp.data_ptr(), pooled.data_ptr(), m2.data_ptr(), None, None, None, None, 0,
                               ops.stream()))
    pooled4 = pooled.view(n, 1, 1, c4)
    x5 = ops.conv_fwd(pooled4, ws[4], asp.conv5.bias)                       # [n,1,1,q]
    check(lib.runet_broadcast_nc(x5.data_ptr(), cat[..., 4 * q:].data_ptr(), ops.ld(cat), n, h4 * w4, q, ops.stream()))
    out, cx = _bn_relu(cat, ws[5], ops.conv_fwd(cat, ws[5], asp.conv_out.bias), asp.bn, tr, sm)
    cx.update(a4=a4, pooled4=pooled4, ws=ws, training=tr)
    return out, cx


def aspp_backward(a, dy, G, pre):
    """Backward of aspp_forward: parameter gradients into G under `pre` (physical layouts), -> gradient of the input."""
    dev, st = dy.device, ops.stream()
    sm = B.Small(dev)
    ws, cat, a4 = a["ws"], a["x"], a["a4"]
    q = ws[0].shape[3]
    dco = _bn_relu_backward(a, dy, G, pre + "bn", a["training"])
    _conv_grads(G, pre + "conv_out", ops.conv_wgrad(cat, dco, 1, 1), dco)
    dcat = ops.conv_dgrad(dco, ws[5])
    n4, h4, w4, c4 = a4.shape
    da4 = ops.conv_dgrad(dcat[..., 0:q], ws[0])
    _conv_grads(G, pre + "conv1", ops.conv_wgrad(a4, dcat[..., 0:q], 1, 1), dcat[..., 0:q])
    for i, d in enumerate((6, 12, 18)):
        sl = dcat[..., (1 + i) * q:(2 + i) * q]
        _conv_grads(G, pre + f"conv{2 + i}", ops.conv_general_wgrad(a4, sl, 3, 3, 1, d, d), sl)
        ops.conv_general_dgrad(sl, ws[1 + i], h4, w4, 1, d, d, out=da4, accumulate=True)
    # image-pooling branch: d(x5)[n,c] = sum over pixels of the broadcast slice; then 1x1 conv backward; then the mean's backward
    dx5 = torch.empty((n4, 1, 1, q), device=dev, dtype=torch.float32)
    sl5 = dcat[..., 4 * q:]
    mean_nc, m2_nc = sm.f(n4 * q), sm.f(n4 * q)
    wsp = B._ws(n4, h4 * w4, q, dev)
    check(lib.runet_chan_stats(sl5.data_ptr(), ops.ld(sl5), n4, h4 * w4, q, wsp.data_ptr(), mean_nc.data_ptr(), m2_nc.data_ptr(), None, None, None,
                               None, 0, st))
    # dx5 = mean * HW (sum over pixels): fold the HW factor into bn_apply-style scale
    ones = torch.full((q,), float(h4 * w4), device=dev, dtype=torch.float32)
    zeros = torch.zeros(q, device=dev, dtype=torch.float32)
    B.bn_apply(mean_nc.view(n4, 1, 1, q), ones, zeros, None, relu=False, out=dx5)
    _conv_grads(G, pre + "conv5", ops.conv_wgrad(a["pooled4"], dx5, 1, 1), dx5)
    dpooled = ops.conv_dgrad(dx5, ws[4])                                   # [n,1,1,512]; each pixel gets dpooled / HW
    inv = torch.full((c4,), 1.0 / float(h4 * w4), device=dev, dtype=torch.float32)
    dpool_s = ops.empty_nhwc(n4, 1, 1, c4, a4)
    B.bn_apply(dpooled, inv, torch.zeros(c4, device=dev, dtype=torch.float32), None, relu=False, out=dpool_s)
    bc = ops.empty_nhwc(n4, h4, w4, c4, a4)
    check(lib.runet_broadcast_nc(dpool_s.data_ptr(), bc.data_ptr(), ops.ld(bc), n4, h4 * w4, c4, st))
    check(lib.runet_add_inplace(da4.data_ptr(), bc.data_ptr(), da4.numel(), st))      # da4 += the broadcast (both dense NHWC)
    return da4


def deeplab_forward(net: DeepLabV3Plus, x, save=True):
    tr = net.training
    dev = x.device
    sm = B.Small(dev)
    n = x.shape[0]
    C = dict(training=tr) if save else None
    if save:
        ops.prefetch_derived(allow_side=False)      # the stale split-operand weights in one launch (DeepLabV3+ has no forward branches)
    a1 = conv_bn_relu(net.conv1, 0, B.to_nhwc_pad(x, 4), tr, sm, C, "conv1", stats=False)
    _, h1, w1, c1 = a1.shape
    ho, wo = (h1 + 2 - 3) // 2 + 1, (w1 + 2 - 3) // 2 + 1
    y = ops.empty_nhwc(n, ho, wo, c1, a1)
    idx = torch.empty((n, ho, wo, c1), device=dev, dtype=torch.uint8)
    check(lib.runet_maxpool3s2_fwd(a1.data_ptr(), ops.ld(a1), y.data_ptr(), ops.ld(y), idx.data_ptr(), n, h1, w1, c1, ops.stream()))
    for key, i in (("conv2", 1), ("conv3", 0), ("conv4", 0)):
        y = conv_bn_relu(getattr(net, key), i, y, tr, sm, C, key, stats=False)
    K = C if save else {}      # the ASPP and decoder steps hand their contexts back either way
    K["pool"] = (idx, h1, w1)
    y, K["aspp"] = aspp_forward(net.aspp, y, tr, sm)
    for i in range(4):
        ct = net.decoder[3 * i]
        w = ops.hwio_t(ct.weight)
        y, K[f"dec{i}"] = _bn_relu(y, w, ops.convt4_fwd(y, w, ct.bias), net.decoder[3 * i + 1], tr, sm)
    head = net.decoder[12]
    wh = ops.hwio(head.weight)
    _, hh, ww, ch = y.shape
    prob = torch.empty((n, 1, hh, ww), device=dev, dtype=torch.float32)
    check(lib.runet_head3x3_fwd(y.data_ptr(), ops.ld(y), wh.data_ptr(), head.bias.data_ptr(), prob.data_ptr(), n, hh, ww, ch, ops.stream()))
    K["head"] = (y, wh, prob)
    return prob, C


def deeplab_backward(net: DeepLabV3Plus, C, dprob):
    """-> {parameter name: gradient in the parameter's PHYSICAL layout (conv weights HWIO, the transposed ones [4, 4, cin, cout])}.
    Takes each step's context out of C, so what a step saved is released when the step is done."""
    G = {}
    dev, st, tr = dprob.device, ops.stream(), C["training"]
    y, wh, prob = C.pop("head")
    n, hh, ww, ch = y.shape
    dy = ops.empty_nhwc(n, hh, ww, ch, y)
    dwdb = B.vec(9 * ch + 1, dev)
    wsb = B.scratch(lib.runet_head3x3_bwd_workspace_floats(n, hh, ww, ch), dev)
    check(lib.runet_head3x3_bwd(dprob.data_ptr(), prob.data_ptr(), y.data_ptr(), ops.ld(y), wh.data_ptr(), dy.data_ptr(), ops.ld(dy), wsb.data_ptr(),
                                dwdb.data_ptr(), n, hh, ww, ch, st))
    G["decoder.12.weight"] = dwdb[:9 * ch].view(3, 3, ch, 1)
    G["decoder.12.bias"] = dwdb[9 * ch:]
    del y, prob
    for i in (3, 2, 1, 0):
        cx = C.pop(f"dec{i}")
        dt = _bn_relu_backward(cx, dy, G, f"decoder.{3 * i + 1}", tr, out=dy)      # in place: dy is this pass's own tensor, not read again
        _conv_grads(G, f"decoder.{3 * i}", ops.convt4_wgrad(cx["x"], dt), dt)
        dy = ops.convt4_dgrad(dt, cx["w"])
    dy = aspp_backward(C.pop("aspp"), dy, G, "aspp.")
    for seq, i in (("conv4", 0), ("conv3", 0), ("conv2", 1), ("conv1", 0)):
        cx = C.pop(seq)
        dt = B.conv_bn_relu_backward(cx, dy, G, seq, i, tr, out=dy)
        if seq == "conv2":      # behind MaxPool2d(3, 2, 1): the winners get the pooled map's gradient
            dp = ops.conv_dgrad(dt, cx["w"])
            idx, h1, w1 = C["pool"]
            dy = ops.empty_nhwc(n, h1, w1, dp.shape[3], dp)
            check(lib.runet_maxpool3s2_bwd(dp.data_ptr(), ops.ld(dp), idx.data_ptr(), dy.data_ptr(), ops.ld(dy), n, h1, w1, dp.shape[3], st))
        elif seq != "conv1":    # the image needs no gradient
            dy = ops.conv_general_dgrad(dt, cx["w"], cx["x"].shape[1], cx["x"].shape[2], 2, 1)
    return G
