"""What the single-node baseline models share (DeepLabV3Plus, UNet, SegNet, YOLOSeg, SegFormerLite, HRNetWater, WaterNet, MSWNet, ENet,
FastSCNN, PSPNet).

Each of them is ONE autograd node with an explicit backward, NHWC inside.  A model file holds the attribute tree (= the reference's state_dict),
its input check, `<model>_forward(net, x, save)` -> (output, context) and `<model>_backward(net, context, doutput)` -> {parameter name:
gradient in the parameter's PHYSICAL layout}; this module holds the module shell, the node and the one physical -> logical layout rule.
The Conv2d -> BatchNorm2d -> ReLU step they are built from is blocks.conv_bn_relu_forward / _backward.  DESIGN.md, "adding a baseline".
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import blocks as B
from . import ops
from .model import _Act, _Holder, _logical, _require_cuda


# ------------------------------------------------------------------------------------------------------------ stand-ins (no parameters)
class ReLU(_Act):
    """nn.ReLU(inplace=True) stand-in (fused into the BatchNorm kernels)."""

    def __init__(self, inplace=True):
        super().__init__()
        self.inplace = inplace


class Sigmoid(_Act):
    """nn.Sigmoid() stand-in (fused into the head kernels)."""


class MaxPool2d(_Holder):
    """nn.MaxPool2d stand-in (the enclosing forward runs the pool kernel)."""

    def __init__(self, kernel_size=2, stride=None, padding=0):
        super().__init__()
        self.kernel_size, self.stride, self.padding = kernel_size, kernel_size if stride is None else stride, padding


# ------------------------------------------------------------------------------------------------------------ module shell
class FusedNet(nn.Module):
    """Base of the baselines.  A subclass gives `_check_input(x)` (raises on an input its kernels do not take) and `_passes()` -> its
    module's (<model>_forward, <model>_backward), looked up when called: a test that wraps one of them sees its wrapper run."""

    PRECISIONS = ("f32",)
    FP32_ONLY = "some of its kernels have no bf16 / fp16 variant"
    precision = "f32"
    _transposed = None

    def __setattr__(self, name, value):
        # ddp.GradAllReducer(sync_bn=True) / set_sync_bn(True) install a cross-rank BatchNorm hook on the model; these models use per-rank
        # statistics only - refuse loudly instead of silently training a different function than the caller asked for
        if name == "sync_bn_hook" and value is not None:
            raise NotImplementedError(f"{type(self).__name__} has no SyncBatchNorm path (per-rank BatchNorm statistics only): "
                                      "construct GradAllReducer(sync_bn=False)")
        super().__setattr__(name, value)

    def set_precision(self, mode):
        if mode not in self.PRECISIONS:
            why = f" ({self.FP32_ONLY})" if self.PRECISIONS == ("f32",) else ""
            raise ValueError(f"{type(self).__name__}: precision must be one of {self.PRECISIONS}{why}")
        self.precision = mode
        return self

    def forward(self, x):
        _require_cuda(x)
        self._check_input(x)
        params = [p for _, p in self.named_parameters()]
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return _FusedFn.apply(x, self, *params)
        with ops.precision(self.precision):
            return self._passes()[0](self, x, save=False)[0]

    def logical_grad(self, name, g):
        """One entry of <model>_backward's dictionary -> the gradient shaped like the parameter.  The type of the module that owns the
        parameter decides (model._logical): the weight of a transposed convolution (a holder class with TRANSPOSED_WEIGHT) [kh, kw, cin, cout]
        -> [cin, cout, kh, kw], any other 4-D gradient HWIO -> OIHW, the rest as it is.  Views; ops.deliver_grads copies."""
        if self._transposed is None:
            self._transposed = frozenset(f"{k}.weight" for k, m in self.named_modules() if getattr(m, "TRANSPOSED_WEIGHT", False))
        return _logical(g, name in self._transposed)


def check_image(x, multiple, why, fp32=False):
    """x must be [N, 3, H, W] with H and W multiples of `multiple` (`why`: what needs that); fp32: and float32 (TypeError)"""
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError("expected x [N, 3, H, W]")
    if x.shape[2] % multiple or x.shape[3] % multiple:
        raise ValueError(f"H and W must be multiples of {multiple} ({why})")
    if fp32 and x.dtype != torch.float32:
        raise TypeError("the kernels compute in fp32")


def conv_bn_relu(seq, i, x, training, sm, C, key, stats=True, out=None):
    """seq[i] (Conv2d, stride 1 or 2) -> seq[i + 1] (BatchNorm2d) -> ReLU: blocks.conv_bn_relu_forward on the modules' handles.  The
    context goes to C[key] (C None: not kept); blocks.conv_bn_relu_backward(C[key], dy, G, seq's name, i, ...) is its backward."""
    conv, bn = seq[i], seq[i + 1]
    a, cx = B.conv_bn_relu_forward(x, ops.hwio(conv.weight), conv.bias, bn.state(), training, sm, conv.stride[0], stats, C is not None, out)
    if C is not None:
        C[key] = cx
    return a


class _FusedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, net, *params):
        with ops.precision(net.precision):
            out, C = net._passes()[0](net, x, save=True)
        ctx.C, ctx.net = C, net
        return out

    @staticmethod
    def backward(ctx, dout):
        net = ctx.net
        if ctx.C is None:
            raise RuntimeError(f"{type(net).__name__} backward called twice (activations were released after the first pass)")
        with ops.precision(net.precision), ops.wgrad_side_stream():
            G = net._passes()[1](net, ctx.C, dout.contiguous())
        ctx.C = None
        named = list(net.named_parameters())
        ops.deliver_grads(net, [p for _, p in named], [net.logical_grad(k, G[k]) for k, _ in named])   # fixed addresses, assigned here (not returned to autograd)
        return (None, None) + (None,) * len(named)
