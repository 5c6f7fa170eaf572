"""Fast-SCNN baseline of the reference (comne.py:305-476) on the gfx950 kernels.

Drop-in for the reference's `FastSCNN` and its sub-modules `DepthwiseSeparableConv`, `LearningToDownsample`, `PyramidPoolingFastSCNN`,
`GlobalFeatureExtractor`, `FeatureFusionModule` and `Classifier` (trained there with nn.BCELoss and Adam 1e-4, weight decay 1e-4): same
constructor, attribute tree and state_dict (139 entries, 191 281 parameters).  forward(x [N, 3, H, W]) -> sigmoid probabilities [N, 1, H, W].

  learning_to_downsample   conv1 (Conv2d 3 -> 32, 3x3 stride 2, no bias -> BatchNorm2d -> ReLU), dsconv1 (32 -> 48, stride 2), dsconv2 (48 -> 64,
                           stride 2): the H/8 map x_low
  global_feature_extractor block1 (64 -> 64 x 3), block2 (64 -> 96 stride 2, 96 -> 96 x 2), block3 (96 -> 128, 128 -> 128 x 2) at H/16, then
                           ppm: AdaptiveAvgPool2d to 1 / 2 / 3 / 6 bins -> Conv2d 1x1 128 -> 32 -> BatchNorm2d -> ReLU -> bilinear resize,
                           cat([x, the four]) = 256 channels
  feature_fusion           relu(BatchNorm(Conv1x1 64 -> 128 (x_low)) + upsample x2 (BatchNorm(Conv1x1 256 -> 128 (x_high))))
  classifier               conv1, conv2 (DepthwiseSeparableConv 128 -> 128), conv3 (Conv2d 1x1 128 -> 1); bilinear x8 to the input size; sigmoid
A DepthwiseSeparableConv is depthwise 3x3 (no bias) -> pointwise 1x1 (no bias) -> BatchNorm2d -> ReLU; the model has thirteen of them.

One autograd node with an explicit backward, NHWC inside (baseline.py):
  stem            baseline.conv_bn_relu (runet_conv2d_general, stride 2) on a 4-channel NHWC copy of the image
  separable       blocks.dwsep_forward / dwsep_backward: runet_dw3_fwd, the shared 1x1 convolution (BatchNorm statistics from its epilogue where
                  offered) and weight gradient, runet_dw3_wgrad / runet_dw3_dgrad behind the shared 1x1 data gradient.  Opt-in: runet_dwsep_fwd
                  multiplies the depthwise outputs of a pixel tile by the pointwise weight from LDS and emits the statistics partials,
                  runet_dwsep_wgrad_pw recomputes them for the pointwise weight gradient - the depthwise tensor exists in neither pass
  pyramid         blocks.ppm_forward / ppm_backward: one pooling launch for the four bin sizes, the shared 1x1 convolution and BatchNorm on
                  dense [n, b, b, c] views, one launch for the four resizes into channel slices [128, 256) of the concat buffer whose first
                  half block3's last layer wrote (no copy)
  fusion          blocks.ffm_forward: runet_ffm_fwd, the upsampled high branch never exists; backward through runet_relu_mask_nhwc,
                  runet_bilinear_nhwc_bwd_sums and the shared BatchNorm backward
  head            runet_outc_fwd's logit plane at H/8 -> runet_up_sigmoid_fwd / _bwd (factor 8) -> runet_outc_bwd on the logit's gradient
The conv biases of the pyramid branches (in front of a BatchNorm) are kept and trained as the reference does.  Every gradient is summed in a
fixed order (no float atomics): two steps from the same state give the same bits.

A/B switches (blocks.py): RUNET_FUSED_DWSEP=1 (the fused separable kernels: measured slower in the 16 x 256^2 step, so opt-in;
RUNET_NO_FUSED_DWSEP=1 forces the default path), RUNET_NO_FUSED_FFM=1 (the fusion from runet_bn_apply, runet_bn_bilinear_nhwc_fwd and
runet_add_inplace).

Bounds: n_classes = 1 only, H and W multiples of 32, more than one image per batch in training mode (the 1-bin pyramid branch's BatchNorm
sees N values per channel; the reference raises there too), fp32 only, per-rank BatchNorm statistics only.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import blocks as B
from . import ops
from ._lib import check, lib
from .baseline import FusedNet, ReLU, check_image, conv_bn_relu
from .model import BatchNorm2d, Conv2d, _Holder

LOW_C, HIGH_C, FUSE_C = 64, 128, 128
FFM_SCALE, HEAD_SCALE = 2, 8
# the separable layers in forward order: (attribute path, cin, cout, stride)
LAYERS = (("learning_to_downsample.dsconv1", 32, 48, 2), ("learning_to_downsample.dsconv2", 48, 64, 2),
          ("global_feature_extractor.block1.0", 64, 64, 1), ("global_feature_extractor.block1.1", 64, 64, 1),
          ("global_feature_extractor.block1.2", 64, 64, 1), ("global_feature_extractor.block2.0", 64, 96, 2),
          ("global_feature_extractor.block2.1", 96, 96, 1), ("global_feature_extractor.block2.2", 96, 96, 1),
          ("global_feature_extractor.block3.0", 96, 128, 1), ("global_feature_extractor.block3.1", 128, 128, 1),
          ("global_feature_extractor.block3.2", 128, 128, 1), ("classifier.conv1", 128, 128, 1), ("classifier.conv2", 128, 128, 1))
TRUNK = LAYERS[2:11]         # x_low -> the pyramid's input


class DepthwiseConv3x3(_Holder):
    """nn.Conv2d(c, c, 3, stride, padding=1, groups=c, bias=False) parameter holder: weight logical [c, 1, 3, 3], memory [3][3][1][c] (HWIO)."""

    def __init__(self, channels, stride=1):
        super().__init__()
        self.in_channels = self.out_channels = self.groups = channels
        self.kernel_size, self.padding, self.stride = (3, 3), (1, 1), (stride, stride)
        self.weight = nn.Parameter(torch.empty(3, 3, 1, channels).permute(3, 2, 0, 1))
        self.register_parameter("bias", None)
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))


class AdaptiveAvgPool2d(_Holder):
    """nn.AdaptiveAvgPool2d stand-in (runet_pyramid_pool_fwd pools the four bin sizes at once)."""

    def __init__(self, output_size):
        super().__init__()
        self.output_size = output_size


class DepthwiseSeparableConv(_Holder):
    """Parameter layout of the reference module (:305-320); FastSCNN carries its passes (blocks.dwsep_forward / dwsep_backward)."""

    def __init__(self, in_channels, out_channels, stride=1):
        super().__init__()
        if stride not in (1, 2):
            raise ValueError("the depthwise kernels take stride 1 or 2")
        self.depthwise = DepthwiseConv3x3(in_channels, stride)
        self.pointwise = Conv2d(in_channels, out_channels, 1, bias=False)
        self.bn = BatchNorm2d(out_channels)
        self.relu = ReLU()

    def handles(self):
        return B.DWSepParams(ops.hwio(self.depthwise.weight), ops.hwio(self.pointwise.weight), self.bn.state(), self.depthwise.stride[0])


class LearningToDownsample(_Holder):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Sequential(Conv2d(3, 32, 3, padding=1, bias=False, stride=2), BatchNorm2d(32), ReLU())
        self.dsconv1 = DepthwiseSeparableConv(32, 48, stride=2)
        self.dsconv2 = DepthwiseSeparableConv(48, 64, stride=2)


class PyramidPoolingFastSCNN(_Holder):
    def __init__(self, in_channels, pool_sizes=(1, 2, 3, 6)):
        super().__init__()
        if tuple(pool_sizes) != B.PYR_BINS or in_channels % 16:
            raise ValueError("the pyramid kernels pool to 1 / 2 / 3 / 6 bins over a multiple of 16 channels")
        self.pool_sizes = list(pool_sizes)
        q = in_channels // 4
        self.convs = nn.ModuleList([nn.Sequential(AdaptiveAvgPool2d(b), Conv2d(in_channels, q, 1), BatchNorm2d(q), ReLU()) for b in pool_sizes])

    def handles(self):
        return B.PPMParams([ops.hwio(s[1].weight) for s in self.convs], [s[1].bias for s in self.convs], [s[2].state() for s in self.convs])


class GlobalFeatureExtractor(_Holder):
    def __init__(self):
        super().__init__()
        self.block1 = self._make_bottleneck(64, 64, 3, 1)
        self.block2 = self._make_bottleneck(64, 96, 3, 2)
        self.block3 = self._make_bottleneck(96, 128, 3, 1)
        self.ppm = PyramidPoolingFastSCNN(128, pool_sizes=[1, 2, 3, 6])

    @staticmethod
    def _make_bottleneck(in_channels, out_channels, repeats, stride):
        return nn.Sequential(DepthwiseSeparableConv(in_channels, out_channels, stride),
                             *[DepthwiseSeparableConv(out_channels, out_channels, 1) for _ in range(repeats - 1)])


class FeatureFusionModule(_Holder):
    def __init__(self, high_channels, low_channels, out_channels):
        super().__init__()
        self.conv_low = nn.Sequential(Conv2d(low_channels, out_channels, 1, bias=False), BatchNorm2d(out_channels))
        self.conv_high = nn.Sequential(Conv2d(high_channels, out_channels, 1, bias=False), BatchNorm2d(out_channels))
        self.relu = ReLU()


class Classifier(_Holder):
    def __init__(self, in_channels, n_classes):
        super().__init__()
        self.conv1 = DepthwiseSeparableConv(in_channels, in_channels, 1)
        self.conv2 = DepthwiseSeparableConv(in_channels, in_channels, 1)
        self.conv3 = Conv2d(in_channels, n_classes, 1)


class FastSCNN(FusedNet):
    FP32_ONLY = "the depthwise, pyramid and fusion kernels are fp32"

    def __init__(self, n_classes=1):
        super().__init__()
        if n_classes != 1:
            raise ValueError("the fused head implements the reference's n_classes=1 sigmoid head")
        self.n_classes = n_classes
        self.learning_to_downsample = LearningToDownsample()
        self.global_feature_extractor = GlobalFeatureExtractor()
        self.feature_fusion = FeatureFusionModule(high_channels=2 * HIGH_C, low_channels=LOW_C, out_channels=FUSE_C)
        self.classifier = Classifier(FUSE_C, n_classes)

    def _check_input(self, x):
        check_image(x, 32, "four stride-2 stages whose H/16 map is resized onto the H/8 one, and the pyramid on top", fp32=True)
        if self.training and x.shape[0] == 1:
            raise ValueError("Expected more than 1 value per channel when training: the pyramid's 1-bin branch feeds a BatchNorm N values "
                             "per channel (use a batch of at least 2, or eval mode)")

    def _passes(self):
        return fastscnn_forward, fastscnn_backward


def _layer(net, path):
    m = net
    for part in path.split("."):
        m = getattr(m, part)
    return m


def _conv1x1_bn(seq, x, training, sm):
    """seq = (Conv2d 1x1 without bias, BatchNorm2d) -> the raw convolution output, its context"""
    w = ops.hwio(seq[0].weight)
    fs = {} if training else None
    t = ops.conv_fwd(x, w, None, stats=fs)
    s, h, mean, invstd, _ = B.bn_coeff(t, seq[1].state(), training, sm, fused=fs)
    return t, dict(x=x, w=w, t=t, s=s, h=h, mean=mean, invstd=invstd)


def fastscnn_forward(net: FastSCNN, x, save=True):
    tr = net.training
    sm = B.Small(x.device)
    n, _, H, W = x.shape
    C = {} if save else None
    ops.branches_pay(n, H, W)
    if save:
        ops.prefetch_derived()
    L = {}

    def sep(path, a, out=None):
        y, cx = B.dwsep_forward(a, _layer(net, path).handles(), tr, sm, out=out, save=save)
        L[path] = cx
        return y

    a = conv_bn_relu(net.learning_to_downsample.conv1, 0, B.to_nhwc_pad(x, 4), tr, sm, C, "stem", stats=False)
    a = sep(LAYERS[0][0], a)
    x_low = sep(LAYERS[1][0], a)
    a = x_low
    cat = None
    for path, _, cout, stride in TRUNK:
        if path == TRUNK[-1][0]:
            cat = ops.empty_nhwc(n, a.shape[1], a.shape[2], 2 * HIGH_C, a)
            sep(path, a, out=cat[..., :HIGH_C])
        else:
            a = sep(path, a)
    ppm = B.ppm_forward(cat, net.global_feature_extractor.ppm.handles(), tr, sm, save=save)
    ff = net.feature_fusion
    t_low, low = _conv1x1_bn(ff.conv_low, x_low, tr, sm)
    t_high, high = _conv1x1_bn(ff.conv_high, cat, tr, sm)
    y = B.ffm_forward(t_low, (low["s"], low["h"]), t_high, (high["s"], high["h"]), FFM_SCALE)
    a = sep("classifier.conv1", y)
    a = sep("classifier.conv2", a)
    conv3 = net.classifier.conv3
    wo = ops.hwio(conv3.weight)
    _, logit = B.outc_forward(a, wo, conv3.bias, want_logit=True)
    prob = B.up_sigmoid_forward(logit.view(n, a.shape[1], a.shape[2]), HEAD_SCALE)
    if save:
        C.update(sep=L, ppm=ppm, low=low, high=high, y=y, head=(a, wo, prob), training=tr)
    return prob, C


def fastscnn_backward(net: FastSCNN, C, dprob):
    """-> {parameter name: gradient in the parameter's PHYSICAL layout (conv weights HWIO, the depthwise ones [3, 3, 1, c])}"""
    dev = dprob.device
    tr = C["training"]
    sink = B.DictSink(dev)
    G = sink.g
    L = C["sep"]
    st = ops.stream()

    def sep_back(path, da, need_dx=True):
        return B.dwsep_backward(L[path], da, G, path + ".", tr, need_dx=need_dx)

    # ---- head: dprob -> the logit plane's gradient -> conv3
    a, wo, prob = C["head"]
    n, h, w, c = a.shape
    dz = B.up_sigmoid_backward(dprob, prob, HEAD_SCALE)
    da = ops.empty_nhwc(n, h, w, c, a)
    dw_db = sink.buf("classifier.conv3.", [("weight", (1, 1, c, 1)), ("bias", (1,))])
    check(lib.runet_outc_bwd(dz.data_ptr(), None, a.data_ptr(), ops.ld(a), wo.data_ptr(), da.data_ptr(), ops.ld(da), B._ws(n, h * w, c, dev).data_ptr(),
                             dw_db.data_ptr(), n * h * w, c, st))
    dy = sep_back("classifier.conv1", sep_back("classifier.conv2", da))
    # ---- feature fusion
    low, high = C["low"], C["high"]
    sums_l, sums_h = B.vec(2 * FUSE_C, dev), B.vec(2 * FUSE_C, dev)
    dt_low, dt_high = B.ffm_backward(dy, C["y"], low["t"], (low["mean"], low["invstd"], low["s"]), high["t"],
                                     (high["mean"], high["invstd"], high["s"]), FFM_SCALE, sums_l, sums_h, training=tr)
    for name, cx, dt, sums in (("conv_low", low, dt_low, sums_l), ("conv_high", high, dt_high, sums_h)):
        G[f"feature_fusion.{name}.1.weight"], G[f"feature_fusion.{name}.1.bias"] = sums[:FUSE_C], sums[FUSE_C:]
        G[f"feature_fusion.{name}.0.weight"] = ops.conv_wgrad(cx["x"], dt, 1, 1)
    dx_low = ops.conv_dgrad(dt_low, low["w"])
    dcat = ops.conv_dgrad(dt_high, high["w"])
    # ---- pyramid and trunk, then the two paths into x_low added in a fixed order (trunk + fusion)
    dg = B.ppm_backward(C["ppm"], dcat, G, "global_feature_extractor.ppm.", tr)
    for path, _, _, _ in reversed(TRUNK):
        dg = sep_back(path, dg)
    check(lib.runet_add_inplace(dg.data_ptr(), dx_low.data_ptr(), dg.numel(), st))
    da = sep_back(LAYERS[0][0], sep_back(LAYERS[1][0], dg))
    # ---- stem (no input gradient: the input is the image)
    cx = C["stem"]
    sums = B.vec(64, dev)
    dt = B.bn_backward(da, cx["t"], cx["mean"], cx["invstd"], cx["s"], sums, relu_shift=cx["h"], out=da, training=tr)
    G["learning_to_downsample.conv1.1.weight"], G["learning_to_downsample.conv1.1.bias"] = sums[:32], sums[32:]
    G["learning_to_downsample.conv1.0.weight"] = ops.conv_general_wgrad(cx["x"], dt, 3, 3, 2, 1, cin_w=3)
    return G
