"""PSPNet baseline of the reference (comne.py:214-299) on the gfx950 kernels.

Drop-in for the reference's `PSPNet` and its sub-module `PyramidPooling` (trained there with nn.BCELoss and Adam 1e-4, weight decay 1e-4):
same constructor, attribute tree and state_dict (65 entries, 38 parameter tensors, 6 537 217 parameters).
forward(x [N, 3, H, W]) -> sigmoid probabilities [N, 1, H, W].

  conv1..conv4  Conv2d 3 -> 64 -> 128 -> 256 -> 512, 3x3 stride 2 with bias -> BatchNorm2d -> ReLU: the H/16 map
  ppm           PyramidPooling(512): AdaptiveAvgPool2d to 1 / 2 / 3 / 6 bins -> Conv2d 1x1 512 -> 128 -> BatchNorm2d -> ReLU -> bilinear resize
                to the H/16 map, cat([x, the four]) = 1024 channels
  final_conv    Conv2d 1024 -> 512, 3x3 -> BatchNorm2d -> ReLU -> Dropout2d(0.1) -> Conv2d 1x1 512 -> 1; bilinear x16 to the input size; sigmoid

One autograd node with an explicit backward, NHWC inside (baseline.py):
  backbone      baseline.conv_bn_relu (runet_conv2d_general, stride 2) from a 4-channel NHWC copy of the image; conv4 writes channels [0, 512)
                of the [n, h, w, 1024] concat buffer
  pyramid       blocks.ppm_forward / ppm_backward: Fast-SCNN's pooling and resize launches, the shared 1x1 convolution and BatchNorm on dense
                [n, b, b, c] views (c = 512, 128 per branch)
  final_conv.0  ops.conv_fwd / conv_dgrad / conv_wgrad, 3x3 1024 -> 512 with bias
  head          runet_bn_apply(mask, relu), runet_outc_fwd's logit plane at H/16 -> runet_up_sigmoid_fwd / _bwd (factor 16) -> runet_outc_bwd on the
                logit's gradient
The seven convolution biases in front of a BatchNorm are kept and trained as the reference does (their gradient is zero up to rounding in
training mode).  Every gradient is summed in a fixed order (no float atomics): two steps from the same state give the same bits.

Opt-in fusions (blocks.py, read at import; both tested against the same goldens as the default path):
  RUNET_FUSED_PSP_TAPS=1  final_conv.0 as tap planes (blocks.psp_taps_forward / _backward, runet_psp_taps_*): the convolution and the resize are
                linear, so the pyramid half of the 1024 input channels is multiplied on the 50 cells per image (four small GEMMs through the
                shared 1x1 entries; their data gradient through runet_psp_taps_dp) and the shifted, resized planes are added onto the 3x3
                convolution of the 512 dense channels: no concat buffer, no upsampled channels, half of the layer's matrix work in all three
                passes.  The two halves of the weight reach the shared kernels as split copies (blocks.psp_split_weights), refreshed when the
                parameter changes.  0.03 - 0.04 ms ahead in the 4.5 ms 16 x 256^2 step, inside the round-to-round spread: the layer is far from
                matrix-bound on the 16 x 16 map, and the small GEMMs, the split and the join take back most of what the halved layer saves.
  RUNET_FUSED_PSP_HEAD=1  blocks.psp_head_forward / _backward on runet_psp_head_*: BatchNorm, ReLU, Dropout2d and the 1x1 convolution in one pass,
                the activated tensor and its gradient never written.  Its gain in the step stayed inside the round-to-round spread.
RUNET_NO_FUSED_PSP_TAPS=1 / RUNET_NO_FUSED_PSP_HEAD=1 force the default path.

Bounds: n_classes = 1 only; pool_sizes (1, 2, 3, 6) over a multiple of 16 channels; H and W multiples of 16 (the head kernel resizes by the
integer factor 16; the reference takes any size); more than one image per batch in training mode (the 1-bin branch's BatchNorm sees N values
per channel; the reference raises there too); fp32 only; per-rank BatchNorm statistics only.
"""
from __future__ import annotations

import torch.nn as nn

from . import blocks as B
from . import ops
from .baseline import FusedNet, ReLU, check_image, conv_bn_relu
from .fastscnn import AdaptiveAvgPool2d
from .model import BatchNorm2d, Conv2d, Dropout2d, _Holder

BACKBONE = (("conv1", 3, 64), ("conv2", 64, 128), ("conv3", 128, 256), ("conv4", 256, 512))
PPM_C = 512


class PyramidPooling(_Holder):
    """Parameter layout of the reference module (:214-240); PSPNet carries its passes (blocks.ppm_cells_forward / ppm_cells_backward)."""

    def __init__(self, in_channels, pool_sizes=(1, 2, 3, 6)):
        super().__init__()
        if tuple(pool_sizes) != B.PYR_BINS:
            raise ValueError("the pyramid kernels pool to 1 / 2 / 3 / 6 bins: pool_sizes must be [1, 2, 3, 6]")
        if in_channels <= 0 or in_channels % 16 or in_channels > 1024:
            raise ValueError("the pyramid kernels take a multiple of 16 channels, at most 1024 (in_channels // 4 per branch, a multiple of 4 up to 256)")
        self.pool_sizes = list(pool_sizes)
        q = in_channels // len(self.pool_sizes)
        self.convs = nn.ModuleList([nn.Sequential(AdaptiveAvgPool2d(b), Conv2d(in_channels, q, 1), BatchNorm2d(q), ReLU()) for b in pool_sizes])

    def handles(self):
        return B.PPMParams([ops.hwio(s[1].weight) for s in self.convs], [s[1].bias for s in self.convs], [s[2].state() for s in self.convs])


class PSPNet(FusedNet):
    FP32_ONLY = "the pyramid, tap-plane and head kernels are fp32"

    def __init__(self, n_classes=1):
        super().__init__()
        if n_classes != 1:
            raise ValueError("the fused head implements the reference's n_classes=1 sigmoid head")
        self.n_classes = n_classes
        for name, cin, cout in BACKBONE:
            setattr(self, name, nn.Sequential(Conv2d(cin, cout, 3, padding=1, stride=2), BatchNorm2d(cout), ReLU()))
        self.ppm = PyramidPooling(PPM_C, pool_sizes=[1, 2, 3, 6])
        self.final_conv = nn.Sequential(Conv2d(2 * PPM_C, PPM_C, 3, padding=1), BatchNorm2d(PPM_C), ReLU(), Dropout2d(0.1), Conv2d(PPM_C, n_classes, 1))
        self._split = {}          # blocks.psp_split_weights' copies of final_conv.0's two halves

    def set_dropout_masks(self, masks):
        """masks: {"final_conv.3": [N, 512] keep-mask already divided by 1 - p} or None to restore random draws."""
        self.final_conv[3].mask = None if masks is None else masks["final_conv.3"]

    def _check_input(self, x):
        check_image(x, 16, "four stride-2 stages, and the head kernel resizes by the integer factor 16", fp32=True)
        if self.training and x.shape[0] == 1:
            raise ValueError("Expected more than 1 value per channel when training: the pyramid's 1-bin branch feeds a BatchNorm N values "
                             "per channel (use a batch of at least 2, or eval mode)")

    def _passes(self):
        return pspnet_forward, pspnet_backward


def pspnet_forward(net: PSPNet, x, save=True):
    tr = net.training
    sm = B.Small(x.device)
    n, _, H, W = x.shape
    C = {} if save else None
    fc = net.final_conv
    c = fc[1].num_features
    w_full = ops.hwio(fc[0].weight)
    taps = B.FUSED_PSP_TAPS
    wx, wp = B.psp_split_weights(w_full, net._split) if taps else (None, None)      # in front of the prefetch: its refills read the copies
    ops.branches_pay(n, H, W)
    if save:
        ops.prefetch_derived()
    a = B.to_nhwc_pad(x, 4)
    for name, _, _ in BACKBONE[:3]:
        a = conv_bn_relu(getattr(net, name), 0, a, tr, sm, C, name, stats=False)
    p = net.ppm.handles()
    if taps:
        src = conv_bn_relu(net.conv4, 0, a, tr, sm, C, "conv4", stats=False)
        ppm = B.ppm_cells_forward(src, p, tr, sm)
        t = ops.conv_fwd(src, wx, fc[0].bias)
        B.psp_taps_forward(t, ppm["acts"], wp)
    else:
        src = ops.empty_nhwc(n, H // 16, W // 16, 2 * c, a)
        conv_bn_relu(net.conv4, 0, a, tr, sm, C, "conv4", stats=False, out=src[..., :c])
        ppm = B.ppm_forward(src, p, tr, sm, save=True)
        t = ops.conv_fwd(src, w_full, fc[0].bias)
    s, hh, mean, invstd, _ = B.bn_coeff(t, fc[1].state(), tr, sm)
    mask = fc[3].draw(n, c, x.device) if tr else None
    wo = ops.hwio(fc[4].weight)
    prob, saved = B.psp_head_forward(t, s, hh, mask, wo, fc[4].bias)
    if save:
        C.update(ppm=ppm, training=tr, fin=dict(x=src, t=t, s=s, h=hh, mean=mean, invstd=invstd, mask=mask, wo=wo, prob=prob, saved=saved, taps=taps,
                                                w=w_full, wx=wx, wp=wp))
    return prob, C


def pspnet_backward(net: PSPNet, C, dprob):
    """-> {parameter name: gradient in the parameter's PHYSICAL layout (conv weights HWIO)}"""
    dev = dprob.device
    tr = C["training"]
    G = {}
    f = C["fin"]
    t = f["t"]
    c = t.shape[3]
    dt, out = B.psp_head_backward(dprob, f["prob"], t, f["s"], f["h"], f["mask"], f["wo"], f["mean"], f["invstd"], f["saved"], tr)
    G["final_conv.1.weight"], G["final_conv.1.bias"] = out[:c], out[c:2 * c]
    G["final_conv.4.weight"], G["final_conv.4.bias"] = out[2 * c:3 * c].view(1, 1, c, 1), out[3 * c:]
    G["final_conv.0.bias"] = B.chan_sum(dt, B.vec(c, dev))
    if f["taps"]:
        dwx = ops.conv_wgrad(f["x"], dt, 3, 3)
        dacts, dwp = B.psp_taps_backward(dt, C["ppm"]["acts"], f["wp"])
        G["final_conv.0.weight"] = B.psp_join_wgrad(dwx, dwp)
        da = B.ppm_cells_backward(C["ppm"], dacts, ops.conv_dgrad(dt, f["wx"]), G, "ppm.", tr)
    else:
        G["final_conv.0.weight"] = ops.conv_wgrad(f["x"], dt, 3, 3)
        da = B.ppm_backward(C["ppm"], ops.conv_dgrad(dt, f["w"]), G, "ppm.", tr)
    for name, _, _ in reversed(BACKBONE):
        cx = C[name]
        dtt = B.conv_bn_relu_backward(cx, da, G, name, 0, tr, out=da)
        if name != "conv1":          # the image needs no gradient
            da = ops.conv_general_dgrad(dtt, cx["w"], cx["x"].shape[1], cx["x"].shape[2], 2, 1)
    return G
