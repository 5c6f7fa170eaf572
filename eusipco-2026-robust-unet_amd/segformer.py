"""SegFormer-Lite baseline of the reference (Extended_Baseline_Comparison.py:622-744) on the gfx950 kernels.

Drop-in for the reference's `SegFormerLite` (trained there by ModelEvaluator.train_model: nn.BCELoss, Adam 1e-4, weight decay 1e-4, :780-837):
same constructor, attribute tree and state_dict.  Four patch embeddings (Conv2d 7x7 s4 p3, then 3x3 s2 p1, each -> BatchNorm2d -> GELU), three
stages of `c = c + attn(c); c = c + ffn(c)` (EfficientSelfAttention with a key / value reduction r = 8, 4, 2 and 1, 2, 4 heads of 32
channels; MixFFN 1x1 -> depthwise 3x3 -> GELU -> 1x1), and the MLP decoder (1x1 projections, the three deeper ones resized bilinearly to c1's
size, concatenated [_c4, _c3, _c2, _c1], 1x1 fuse + BatchNorm + ReLU, 3x3 + BatchNorm + ReLU, 1x1 + sigmoid), whose probability map is
resized bilinearly to the input size.  forward(x [N, 3, H, W]) -> probabilities [N, 1, H, W].

One autograd node with an explicit backward, NHWC inside (baseline.py):
  patch embeddings   runet_conv2d_general (7x7 s4 with cin 3 padded to 4; 3x3 s2), runet_bn_apply_gelu / runet_bn_bwd_*_gelu
  attention          q / kv / proj 1x1 convolutions, the r x r stride-r reduction through runet_conv2d_general, runet_kv_attention_fwd / _bwd
                     (scores never reach HBM); proj writes on top of a copy of the stage tensor (accumulate), so the stage input survives
  MixFFN             fc1 / fc2 1x1 convolutions (fc2 accumulates like proj), runet_dwconv3x3_gelu_fwd / _bwd_wgrad / runet_dwconv3x3_bwd_data
                     (z kept from the forward; RUNET_DWCONV_RECOMPUTE_Z=1: recomputed in the weight-gradient pass)
  decoder            linear_c4 / c3 / c2 resized by runet_bilinear_nhwc_fwd straight into the 1024-channel concat buffer, linear_c1 written into
                     its slice by the convolution itself; BatchNorm + ReLU as the U-Net's; runet_outc_* (1x1 + sigmoid); runet_bilinear_* for
                     the probability map
Every gradient is summed in a fixed order (no float atomics): two steps from the same state give the same bits.

Bounds: n_classes = 1 only, H and W multiples of 32 (every stage's size and the attention's key count exact), fp32 only, per-rank BatchNorm
statistics only.
"""
from __future__ import annotations

import math
import os

import torch
import torch.nn as nn

from . import blocks as B
from . import ops
from ._lib import check, lib
from .baseline import FusedNet, ReLU, Sigmoid, check_image, conv_bn_relu
from .model import BatchNorm2d, Conv2d, _Act, _Holder

HEAD_DIM = 32
# MixFFN depthwise + GELU: z = dwconv(x) + b is kept from the forward for the backward (measured faster at every stage shape: the forward's
# extra write costs 1-2 us, recomputing z in the weight-gradient pass 12-47 us).  RUNET_DWCONV_RECOMPUTE_Z=1: the A/B
DWCONV_KEEP_Z = os.environ.get("RUNET_DWCONV_RECOMPUTE_Z", "0") != "1"
# (dim, heads, reduction ratio, MixFFN hidden) of stages 1-3 (Extended_Baseline_Comparison.py:690-697)
STAGES = ((32, 1, 8, 128), (64, 2, 4, 256), (128, 4, 2, 512))
# patch embeddings: (cin, cout, kernel, stride, padding) (:677-688)
EMBED = ((3, 32, 7, 4, 3), (32, 64, 3, 2, 1), (64, 128, 3, 2, 1), (128, 256, 3, 2, 1))


class _GELU(_Act):
    """nn.GELU() stand-in (no parameters; fused into the BatchNorm / depthwise kernels)."""


class DepthwiseConv2d(_Holder):
    """nn.Conv2d(c, c, 3, padding=1, groups=c) parameter holder: weight logical [c, 1, 3, 3], memory [3][3][1][c] (HWIO)."""

    def __init__(self, channels, kernel_size=3, padding=1):
        super().__init__()
        assert kernel_size == 3 and padding == 1
        self.in_channels = self.out_channels = self.groups = channels
        self.kernel_size, self.padding, self.stride = (3, 3), (1, 1), (1, 1)
        self.weight = nn.Parameter(torch.empty(3, 3, 1, channels).permute(3, 2, 0, 1))
        self.bias = nn.Parameter(torch.empty(channels))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        nn.init.uniform_(self.bias, -1.0 / 3.0, 1.0 / 3.0)          # fan_in = 1 * 3 * 3


class MixFFN(nn.Module):
    def __init__(self, in_features, hidden_features):
        super().__init__()
        self.fc1 = Conv2d(in_features, hidden_features, 1)
        self.dwconv = DepthwiseConv2d(hidden_features)
        self.fc2 = Conv2d(hidden_features, in_features, 1)
        self.act = _GELU()

    def forward(self, x):
        raise NotImplementedError("MixFFN is fused into SegFormerLite's single autograd node")


class EfficientSelfAttention(nn.Module):
    def __init__(self, dim, num_heads=8, reduction_ratio=4):
        super().__init__()
        if dim // num_heads != HEAD_DIM:
            raise ValueError("the attention kernels implement a head dimension of 32")
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.q = Conv2d(dim, dim, 1)
        self.kv = Conv2d(dim, dim * 2, 1)
        self.proj = Conv2d(dim, dim, 1)
        self.reduction = Conv2d(dim, dim, reduction_ratio, stride=reduction_ratio)
        self.reduction_ratio = reduction_ratio

    def forward(self, x):
        raise NotImplementedError("EfficientSelfAttention is fused into SegFormerLite's single autograd node")


class SegFormerLite(FusedNet):
    FP32_ONLY = "the attention and depthwise kernels are fp32"

    def __init__(self, n_classes=1):
        super().__init__()
        if n_classes != 1:
            raise ValueError("the fused head implements the reference's n_classes=1 sigmoid head")
        self.n_classes = n_classes
        for i, (cin, cout, k, s, p) in enumerate(EMBED, 1):
            setattr(self, f"patch_embed{i}", nn.Sequential(Conv2d(cin, cout, k, padding=p, stride=s), BatchNorm2d(cout), _GELU()))
        for i, (dim, heads, r, hidden) in enumerate(STAGES, 1):
            setattr(self, f"attn{i}", EfficientSelfAttention(dim, num_heads=heads, reduction_ratio=r))
            setattr(self, f"ffn{i}", MixFFN(dim, hidden))
        self.linear_c4 = Conv2d(256, 256, 1)
        self.linear_c3 = Conv2d(128, 256, 1)
        self.linear_c2 = Conv2d(64, 256, 1)
        self.linear_c1 = Conv2d(32, 256, 1)
        self.linear_fuse = nn.Sequential(Conv2d(256 * 4, 256, 1), BatchNorm2d(256), ReLU())
        self.head = nn.Sequential(Conv2d(256, 64, 3, padding=1), BatchNorm2d(64), ReLU(), Conv2d(64, n_classes, 1), Sigmoid())

    def _check_input(self, x):
        check_image(x, 32, "the stride-4 embedding, three stride-2 embeddings and the stage-1 reduction by 8")

    def _passes(self):
        return segformer_forward, segformer_backward


# ------------------------------------------------------------------------------------------------------------------ kernel wrappers
def bn_apply_gelu(x, scale, shift):
    n, h, w, c = x.shape
    out = ops.empty_nhwc(n, h, w, c, x)
    check(lib.runet_bn_apply_gelu(x.data_ptr(), ops.ld(x), out.data_ptr(), ops.ld(out), n * h * w, h * w, c, scale.data_ptr(), shift.data_ptr(),
                                  ops.stream()))
    return out


def bn_backward_gelu(dy, x, mean, invstd, scale, sums, shift, training=True):
    """BatchNorm + GELU backward, GELU'(z) from z = x * scale + shift.  sums: [2c] (dgamma | dbeta).  -> dx"""
    n, h, w, c = x.shape
    hw = h * w
    st = ops.stream()
    check(lib.runet_bn_bwd_reduce_gelu(dy.data_ptr(), ops.ld(dy), x.data_ptr(), ops.ld(x), n, hw, c, mean.data_ptr(), invstd.data_ptr(),
                                       B._ws(n, hw, c, x.device).data_ptr(), sums.data_ptr(), scale.data_ptr(), shift.data_ptr(), st))
    use = sums if training else B.zeros(2 * c, x.device)
    out = ops.empty_nhwc(n, h, w, c, x)
    check(lib.runet_bn_bwd_apply_gelu(dy.data_ptr(), ops.ld(dy), x.data_ptr(), ops.ld(x), out.data_ptr(), ops.ld(out), n * hw, hw, c,
                                      mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(), use.data_ptr(), 0, shift.data_ptr(), st))
    return out


def kv_attention(q, kv, heads):
    """q [n, h, w, C], kv [n, hr, wr, 2C] (NHWC views) -> (o [n, h, w, C], lse [n, heads, h * w])"""
    n, h, w, c = q.shape
    nk = kv.shape[1] * kv.shape[2]
    o = ops.empty_nhwc(n, h, w, c, q)
    lse = torch.empty((n, heads, h * w), device=q.device, dtype=torch.float32)
    check(lib.runet_kv_attention_fwd(q.data_ptr(), ops.ld(q), kv.data_ptr(), ops.ld(kv), o.data_ptr(), ops.ld(o), lse.data_ptr(), n, h * w, nk, c,
                                     heads, ops.stream()))
    return o, lse


def kv_attention_backward(q, kv, o, lse, do, heads, dlse=None):
    """dlse: optional gradient of lse [n, heads, h * w] -> (dq [n, h, w, C], dkv [n, hr, wr, 2C])"""
    n, h, w, c = q.shape
    _, hr, wr, c2 = kv.shape
    nk = hr * wr
    dq = ops.empty_nhwc(n, h, w, c, q)
    dkv = ops.empty_nhwc(n, hr, wr, c2, kv)
    nws = lib.runet_kv_attention_bwd_workspace_floats(n, h * w, nk, c, heads)
    if nws < 0:
        raise ValueError("bad attention shape")
    ws = B.scratch(nws, q.device)
    check(lib.runet_kv_attention_bwd(q.data_ptr(), ops.ld(q), kv.data_ptr(), ops.ld(kv), o.data_ptr(), ops.ld(o), do.data_ptr(), ops.ld(do),
                                     lse.data_ptr(), dlse.data_ptr() if dlse is not None else None, dq.data_ptr(), ops.ld(dq), dkv.data_ptr(), ops.ld(dkv), ws.data_ptr(), ws.numel(), n, h * w,
                                     nk, c, heads, ops.stream()))
    return dq, dkv


def dwconv_gelu(x, w3, b, keep_z=True):
    """x [n, h, w, c], w3 [3, 3, 1, c] (HWIO) -> (z or None, a = GELU(z)), z = b + dwconv3x3(x)"""
    n, h, w, c = x.shape
    a = ops.empty_nhwc(n, h, w, c, x)
    z = ops.empty_nhwc(n, h, w, c, x) if keep_z else None
    check(lib.runet_dwconv3x3_gelu_fwd(x.data_ptr(), ops.ld(x), w3.data_ptr(), b.data_ptr(), z.data_ptr() if keep_z else None,
                                       ops.ld(z) if keep_z else c, a.data_ptr(), ops.ld(a), n, h, w, c, ops.stream()))
    return z, a


def dwconv_gelu_backward(x, z, da, w3, b):
    """z: the forward's z, or None (recomputed from x, w3, b) -> (dx, dwdb [10c] = dw [3][3][c] | db [c]); da is overwritten with
    g = da * GELU'(z)"""
    n, h, w, c = x.shape
    dwdb = torch.empty(10 * c, device=x.device, dtype=torch.float32)
    ws = B.scratch(lib.runet_dwconv3x3_gelu_bwd_workspace_floats(n, h, w, c), x.device)
    st = ops.stream()
    check(lib.runet_dwconv3x3_gelu_bwd_wgrad(x.data_ptr(), ops.ld(x), w3.data_ptr(), b.data_ptr(), da.data_ptr(), ops.ld(da),
                                             z.data_ptr() if z is not None else None, ops.ld(z) if z is not None else c, da.data_ptr(), ops.ld(da),
                                             ws.data_ptr(), ws.numel(), dwdb.data_ptr(), n, h, w, c, st))
    dx = ops.empty_nhwc(n, h, w, c, x)
    check(lib.runet_dwconv3x3_bwd_data(da.data_ptr(), ops.ld(da), w3.data_ptr(), dx.data_ptr(), ops.ld(dx), n, h, w, c, st))
    return dx, dwdb


def bilinear_nhwc(x, out):
    """out (an NHWC view, possibly a channel slice) := bilinear resize of x, align_corners=False"""
    n, h, w, c = x.shape
    _, ho, wo, _ = out.shape
    check(lib.runet_bilinear_nhwc_fwd(x.data_ptr(), ops.ld(x), out.data_ptr(), ops.ld(out), n, h, w, ho, wo, c, ops.stream()))
    return out


def bilinear_nhwc_backward(dy, h, w):
    n, ho, wo, c = dy.shape
    dx = ops.empty_nhwc(n, h, w, c, dy)
    check(lib.runet_bilinear_nhwc_bwd(dy.data_ptr(), ops.ld(dy), dx.data_ptr(), ops.ld(dx), n, h, w, ho, wo, c, ops.stream()))
    return dx


# ------------------------------------------------------------------------------------------------------------------ forward / backward
def _embed(seq, x, tr, sm, save, C, key):
    conv, bn = seq[0], seq[1]
    k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
    w = ops.hwio(conv.weight)
    t = ops.conv_general_fwd(x, w, conv.bias, s, p)
    sc, sh, mean, invstd, _ = B.bn_coeff(t, bn.state(), tr, sm)
    if save:
        C[key] = dict(x=x, w=w, t=t, s=sc, h=sh, mean=mean, invstd=invstd, k=k, stride=s, pad=p)
    return bn_apply_gelu(t, sc, sh)


def _stage(net, i, c, save, C):
    at, ff = getattr(net, f"attn{i}"), getattr(net, f"ffn{i}")
    heads, r = at.num_heads, at.reduction_ratio
    wq, wkv, wp, wr = ops.hwio(at.q.weight), ops.hwio(at.kv.weight), ops.hwio(at.proj.weight), ops.hwio(at.reduction.weight)
    q = ops.conv_fwd(c, wq, at.q.bias)
    red = ops.conv_general_fwd(c, wr, at.reduction.bias, r, 0)
    kv = ops.conv_fwd(red, wkv, at.kv.bias)
    o, lse = kv_attention(q, kv, heads)
    ca = c.clone()
    ops.conv_fwd(o, wp, at.proj.bias, out=ca, accumulate=True)            # c + proj(attn)
    w1, w2, wd = ops.hwio(ff.fc1.weight), ops.hwio(ff.fc2.weight), ops.hwio(ff.dwconv.weight)
    hid = ops.conv_fwd(ca, w1, ff.fc1.bias)
    z, a = dwconv_gelu(hid, wd, ff.dwconv.bias, keep_z=save and DWCONV_KEEP_Z)
    cf = ca.clone()
    ops.conv_fwd(a, w2, ff.fc2.bias, out=cf, accumulate=True)             # c + ffn(c)
    if save:
        C[f"stage{i}"] = dict(c=c, q=q, red=red, kv=kv, o=o, lse=lse, ca=ca, hid=hid, z=z, a=a, wq=wq, wkv=wkv, wp=wp, wr=wr, w1=w1, w2=w2, wd=wd,
                              heads=heads, r=r, bd=ff.dwconv.bias)
    return cf


def segformer_forward(net: SegFormerLite, x, save=True):
    tr = net.training
    dev = x.device
    sm = B.Small(dev)
    n, _, H, W = x.shape
    C = {} if save else None
    cur = B.to_nhwc_pad(x, 4)
    feats = []
    for i in range(1, 5):
        cur = _embed(getattr(net, f"patch_embed{i}"), cur, tr, sm, save, C, f"embed{i}")
        if i < 4:
            cur = _stage(net, i, cur, save, C)
        feats.append(cur)
    c1, c2, c3, c4 = feats
    _, h1, w1, _ = c1.shape
    cat = ops.empty_nhwc(n, h1, w1, 1024, c1)
    lin = {}
    for j, (name, f) in enumerate((("linear_c4", c4), ("linear_c3", c3), ("linear_c2", c2))):
        conv = getattr(net, name)
        w = ops.hwio(conv.weight)
        l = ops.conv_fwd(f, w, conv.bias)
        bilinear_nhwc(l, cat[..., 256 * j:256 * (j + 1)])
        lin[name] = (f, w, l.shape[1], l.shape[2])
    w = ops.hwio(net.linear_c1.weight)
    ops.conv_fwd(c1, w, net.linear_c1.bias, out=cat[..., 768:1024])
    lin["linear_c1"] = (c1, w, h1, w1)
    fa = conv_bn_relu(net.linear_fuse, 0, cat, tr, sm, C, "fuse", stats=False)
    ha = conv_bn_relu(net.head, 0, fa, tr, sm, C, "head", stats=False)
    oconv = net.head[3]
    wo = ops.hwio(oconv.weight)
    psmall, _ = B.outc_forward(ha, wo, oconv.bias)
    prob = torch.empty((n, 1, H, W), device=dev, dtype=torch.float32)
    check(lib.runet_bilinear_fwd(psmall.data_ptr(), prob.data_ptr(), n, h1, w1, H, W, ops.stream()))
    if save:
        C.update(lin=lin, cat=cat, out=(ha, wo, psmall), training=tr, size=(H, W))
    return prob, C


def segformer_backward(net: SegFormerLite, C, dprob):
    """-> {parameter name: gradient in the parameter's PHYSICAL layout (conv weights HWIO, the depthwise ones [3, 3, 1, c])}"""
    G = {}
    dev = dprob.device
    tr = C["training"]

    def conv_grads(name, x, dy, k=1, stride=1, pad=0, cin_w=None):
        if stride == 1 and pad == k // 2:
            G[name + ".weight"] = ops.conv_wgrad(x, dy, k, k, cin_w=cin_w)
        else:
            G[name + ".weight"] = ops.conv_general_wgrad(x, dy, k, k, stride, pad, cin_w=cin_w)
        G[name + ".bias"] = B.chan_sum(dy, B.vec(dy.shape[3], dev))

    # ---- head
    ha, wo, psmall = C["out"]
    n, h1, w1, ch = ha.shape
    H, W = C["size"]
    dps = torch.empty((n, 1, h1, w1), device=dev, dtype=torch.float32)
    check(lib.runet_bilinear_bwd(dprob.data_ptr(), dps.data_ptr(), n, h1, w1, H, W, ops.stream()))
    dha = ops.empty_nhwc(n, h1, w1, ch, ha)
    dwdb = B.vec(ch + 1, dev)
    ws = B._ws(n, h1 * w1, ch, dev)
    check(lib.runet_outc_bwd(dps.data_ptr(), psmall.data_ptr(), ha.data_ptr(), ops.ld(ha), wo.data_ptr(), dha.data_ptr(), ops.ld(dha), ws.data_ptr(),
                             dwdb.data_ptr(), n * h1 * w1, ch, ops.stream()))
    G["head.3.weight"] = dwdb[:ch].view(1, 1, ch, 1)
    G["head.3.bias"] = dwdb[ch:]
    hc = C["head"]
    dhz = B.conv_bn_relu_backward(hc, dha, G, "head", 0, tr)
    dfa = ops.conv_dgrad(dhz, hc["w"])
    del dhz
    fc = C["fuse"]
    dfz = B.conv_bn_relu_backward(fc, dfa, G, "linear_fuse", 0, tr)
    dcat = ops.conv_dgrad(dfz, fc["w"])
    del dfz, dfa
    # ---- decoder projections: gradient of each encoder feature's decoder branch
    dfeat = {}
    for j, name in enumerate(("linear_c4", "linear_c3", "linear_c2", "linear_c1")):
        f, w, lh, lw = C["lin"][name]
        dsl = dcat[..., 256 * j:256 * (j + 1)]
        dl = dsl if name == "linear_c1" else bilinear_nhwc_backward(dsl, lh, lw)
        conv_grads(name, f, dl)
        dfeat[name[-1]] = ops.conv_dgrad(dl, w)
    # ---- encoder, deepest first: dc = gradient of stage i's output (decoder branch + the next embedding's data gradient)
    dc = dfeat["4"]
    for i in (4, 3, 2, 1):
        ec = C[f"embed{i}"]
        cout = ec["t"].shape[3]
        sums = B.vec(2 * cout, dev)
        dt = bn_backward_gelu(dc, ec["t"], ec["mean"], ec["invstd"], ec["s"], sums, ec["h"], training=tr)
        G[f"patch_embed{i}.1.weight"], G[f"patch_embed{i}.1.bias"] = sums[:cout], sums[cout:]
        conv_grads(f"patch_embed{i}.0", ec["x"], dt, ec["k"], ec["stride"], ec["pad"], cin_w=3 if i == 1 else None)
        if i == 1:
            break
        dprev = dfeat[str(i - 1)]
        ops.conv_general_dgrad(dt, ec["w"], ec["x"].shape[1], ec["x"].shape[2], ec["stride"], ec["pad"], out=dprev, accumulate=True)
        del dt
        dc = _stage_backward(C[f"stage{i - 1}"], dprev, G, f"attn{i - 1}", f"ffn{i - 1}", conv_grads)
    return G


def _stage_backward(sc, dcf, G, an, fn, conv_grads):
    """dcf: gradient of the stage output c + attn + ffn -> gradient of the stage input c"""
    # MixFFN: cf = ca + fc2(GELU(dwconv(fc1(ca))))
    da = ops.conv_dgrad(dcf, sc["w2"])
    conv_grads(fn + ".fc2", sc["a"], dcf)
    dhid, dwdb = dwconv_gelu_backward(sc["hid"], sc["z"], da, sc["wd"], sc["bd"])
    c = sc["hid"].shape[3]
    G[fn + ".dwconv.weight"] = dwdb[:9 * c].view(3, 3, 1, c)
    G[fn + ".dwconv.bias"] = dwdb[9 * c:]
    conv_grads(fn + ".fc1", sc["ca"], dhid)
    dca = dcf.clone()
    ops.conv_dgrad(dhid, sc["w1"], out=dca, accumulate=True)
    del da, dhid
    # attention: ca = c + proj(attn(q(c), kv(reduction(c))))
    do = ops.conv_dgrad(dca, sc["wp"])
    conv_grads(an + ".proj", sc["o"], dca)
    dq, dkv = kv_attention_backward(sc["q"], sc["kv"], sc["o"], sc["lse"], do, sc["heads"])
    conv_grads(an + ".kv", sc["red"], dkv)
    dred = ops.conv_dgrad(dkv, sc["wkv"])
    r = sc["r"]
    conv_grads(an + ".reduction", sc["c"], dred, r, r, 0)
    dc = dca.clone()
    x = sc["c"]
    ops.conv_general_dgrad(dred, sc["wr"], x.shape[1], x.shape[2], r, 0, out=dc, accumulate=True)
    conv_grads(an + ".q", x, dq)
    ops.conv_dgrad(dq, sc["wq"], out=dc, accumulate=True)
    return dc
