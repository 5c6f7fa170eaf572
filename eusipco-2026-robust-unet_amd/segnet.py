"""SegNet baseline of the reference's second comparison script on the gfx950 kernels.

Drop-in for `SegNet` in the reference's comne.py:84-211 (trained there like the other baselines: nn.BCELoss, Adam 1e-4, weight decay 1e-4,
comne.py:650-653): same constructor, attribute tree and state_dict (enc1..4 / dec4..1 = Sequential of Conv2d(3x3, bias) -> BatchNorm2d -> ReLU
triples, dec1 ending in Conv2d(64, 1, 3); pool = MaxPool2d(2, 2, return_indices=True), unpool = MaxUnpool2d(2, 2), no parameters),
forward(x [N, 3, H, W]) -> sigmoid probabilities [N, 1, H, W].

One autograd node with an explicit backward, NHWC inside (baseline.py); unet.py's block helpers run every Conv-BN-ReLU stack:
  encoder end   the last BatchNorm + ReLU and the pool that is its only consumer in one pass (runet_bn_relu_maxpool2_fwd): the
                full-resolution activation is never written; backward through the pooled-gradient BatchNorm kernels
                (runet_bn_bwd_reduce_pooled / _apply_pooled), so its full-resolution gradient never exists either
  unpool        forward = the max-pool backward scatter (runet_maxpool2_bwd, no accumulation); backward = the gather runet_maxunpool2_bwd
  head          dec1's last conv + sigmoid = runet_head3x3_fwd / _bwd (the DeepLabV3+ head kernel)

Bounds: n_classes = 1 only (the reference's default and the only value comne.py trains), H and W multiples of 16 (the
reference reaches other sizes through MaxUnpool2d's output_size; this port does not), per-rank BatchNorm statistics only.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import blocks as B
from . import ops
from ._lib import check, lib
from .baseline import FusedNet, check_image
from .model import BatchNorm2d, Conv2d, _Act, _Holder
from .unet import _block_backward, _block_forward

# (block, convolutions as (cin, cout)) in registration order; dec1's second entry is the head conv (no BatchNorm behind it)
ENC = (("enc1", ((3, 64), (64, 64))), ("enc2", ((64, 128), (128, 128))), ("enc3", ((128, 256), (256, 256), (256, 256))),
       ("enc4", ((256, 512), (512, 512), (512, 512))))
DEC = (("dec4", ((512, 512), (512, 512), (512, 256))), ("dec3", ((256, 256), (256, 256), (256, 128))), ("dec2", ((128, 128), (128, 64))),
       ("dec1", ((64, 64),)))


def _stack(convs, head=None):
    mods = []
    for cin, cout in convs:
        mods += [Conv2d(cin, cout, 3, padding=1), BatchNorm2d(cout), _Act()]
    if head is not None:
        mods.append(Conv2d(head[0], head[1], 3, padding=1))
    return nn.Sequential(*mods)


class _MaxPool2dIdx(_Holder):
    """nn.MaxPool2d(2, 2, return_indices=True) stand-in (no parameters; the network's forward runs the fused kernels)."""

    def __init__(self):
        super().__init__()
        self.kernel_size, self.stride, self.return_indices = 2, 2, True


class _MaxUnpool2d(_Holder):
    """nn.MaxUnpool2d(2, 2) stand-in."""

    def __init__(self):
        super().__init__()
        self.kernel_size, self.stride = 2, 2


class SegNet(FusedNet):
    PRECISIONS = ops.PRECISIONS

    def __init__(self, n_classes=1):
        super().__init__()
        if n_classes != 1:
            raise ValueError("the fused head implements the reference's n_classes=1 sigmoid head")
        self.n_classes = n_classes
        for name, convs in ENC:
            setattr(self, name, _stack(convs))
        for name, convs in DEC:
            setattr(self, name, _stack(convs, head=(64, n_classes) if name == "dec1" else None))
        self.pool = _MaxPool2dIdx()
        self.unpool = _MaxUnpool2d()

    def _check_input(self, x):
        check_image(x, 16, "four 2x2 poolings")

    def _passes(self):
        return segnet_forward, segnet_backward


def segnet_forward(net: SegNet, x, save=True):
    tr = net.training
    dev = x.device
    sm = B.Small(dev)
    n = x.shape[0]
    C = {}
    ops.branches_pay(n, x.shape[2], x.shape[3])
    if save:
        ops.prefetch_derived()
    cur = B.to_nhwc_pad(x, 4)
    for lvl, (name, _) in enumerate(ENC, 1):
        (cur, idx), C[name] = _block_forward(cur, getattr(net, name), tr, sm, save=save, tail=B.bn_relu_maxpool_forward)
        C[f"idx{lvl}"] = idx
    for lvl, (name, _) in zip((4, 3, 2, 1), DEC):
        u = B.maxunpool_forward(cur, C[f"idx{lvl}"])
        cur, C[name] = _block_forward(u, getattr(net, name), tr, sm, save=save)
    head = net.dec1[3]
    wh = ops.hwio(head.weight)
    _, h, w, c = cur.shape
    prob = torch.empty((n, 1, h, w), device=dev, dtype=torch.float32)
    check(lib.runet_head3x3_fwd(cur.data_ptr(), ops.ld(cur), wh.data_ptr(), head.bias.data_ptr(), prob.data_ptr(), n, h, w, c, ops.stream()))
    if save:
        C["head"] = (cur, wh, prob)
    return prob, (C if save else None)


def segnet_backward(net: SegNet, C, dprob):
    """-> {parameter name: gradient in the parameter's PHYSICAL layout (conv weights HWIO)}"""
    G = {}
    dev = dprob.device
    y, wh, prob = C["head"]
    n, h, w, c = y.shape
    dy = ops.empty_nhwc(n, h, w, c, y)
    dwdb = B.vec(9 * c + 1, dev)
    wsb = B.scratch(lib.runet_head3x3_bwd_workspace_floats(n, h, w, c), dev)
    check(lib.runet_head3x3_bwd(dprob.data_ptr(), prob.data_ptr(), y.data_ptr(), ops.ld(y), wh.data_ptr(), dy.data_ptr(), ops.ld(dy), wsb.data_ptr(),
                                dwdb.data_ptr(), n, h, w, c, ops.stream()))
    G["dec1.3.weight"], G["dec1.3.bias"] = dwdb[:9 * c].view(3, 3, c, 1), dwdb[9 * c:]
    for lvl, (name, _) in zip((1, 2, 3, 4), reversed(DEC)):
        du = _block_backward(C[name], dy, G, name)                            # gradient of the unpooled tensor
        dy = B.maxunpool_backward(du, C[f"idx{lvl}"])                          # -> gradient of the tensor the unpool scattered
        del du
    for lvl, (name, _) in zip((4, 3, 2, 1), reversed(ENC)):
        idx = C[f"idx{lvl}"]

        def pooled(dp, t, mean, invstd, scale, sums, shift, training, idx=idx):
            return B.bn_backward_pooled(dp, idx, t, mean, invstd, scale, sums, shift, training=training)
        dy = _block_backward(C[name], dy, G, name, need_dx=lvl > 1, tail_bwd=pooled)
    return G
