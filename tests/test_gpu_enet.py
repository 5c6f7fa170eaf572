"""GPU: the ENet baseline (the reference's comne.py:482-608, BCELoss + Adam) on the HIP kernels.

  kernels   the rectangular convolution entries ((5, 1) / (1, 5), per-axis padding: forward, data and weight gradient, and their bit-equality
            with runet_conv2d_general on symmetric arguments), the shared convolutions at the widths and dilations this model brings (4
            channels, dilation 2..16), the k3-s2 transposed convolution built on the stride-2 convolution's data gradient, the initial block
            and the bottleneck tail together with their unfused partners, and the one-channel k2-s2 transposed-convolution sigmoid head - each
            against float64 math written in the reference's order (F.conv2d, F.conv_transpose2d, F.max_pool2d, F.batch_norm and their autograd)
  model     one train step against the reference goldens (tests/golden/enet_*), the same under each RUNET_NO_FUSED_ENET_* switch,
            decision-aware gradient parity against the CPU restatement in float64 (tests/enet_ref.py), sizes and bounds, determinism and graph
            capture
The error measure is tests/test_gpu_fastscnn.py's: max |got - want| / max |want|, band 1e-5 (fp32 kernels with fp32 statistics); where the
shared matrix-core kernels carry the value, tests/test_gpu_conv.py's bands in the same measure (2e-4, weight gradients 3e-4 x
max(1, sqrt(pixels / 256))).  Two runs of every kernel must give the same bits; kernels that write channel slices of wider buffers must leave
the other channels bit-unchanged.
"""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT, load_npz

import decisions_enet as DE
import enet_ref as eref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PKG = "eusipco-2026-robust-unet_amd"
BAND = 1e-5
CONV_BAND = 2e-4
EPS = 1e-5


def _wgrad_band(pixels):
    return 3e-4 * max(1.0, (pixels / 256.0) ** 0.5)


def _mod(name):
    return importlib.import_module(f"{PKG}.{name}")


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _err(got, want):
    """max |got - want| / max |want|"""
    want = want.double().cpu()
    return float((got.double().cpu() - want).abs().max()) / max(float(want.abs().max()), 1e-30)


def _nhwc(t):
    """NCHW -> a dense NHWC tensor with canonical strides (permute().contiguous() keeps the permuted strides of size-1 dimensions, which
    ops.ld rejects)"""
    n, c, h, w = t.shape
    return torch.empty((n, h, w, c), dtype=t.dtype, device=t.device).copy_(t.permute(0, 2, 3, 1))


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _hwio(w):
    """OIHW -> a dense HWIO tensor on the device"""
    return w.permute(2, 3, 1, 0).contiguous().to(DEV)


def _in_slice(t_nhwc, lo, wide):
    """-> (a channel-slice view holding t inside a wider random buffer, the buffer)"""
    n, h, w, c = t_nhwc.shape
    buf = torch.randn((n, h, w, wide), device=DEV)
    buf[..., lo:lo + c] = t_nhwc
    return buf[..., lo:lo + c], buf


def _conv_ref(x, w, stride, pad, dil, dy_seed):
    """float64 F.conv2d and its autograd -> (y, dy, dx, dw)"""
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y = F.conv2d(x64, w64, None, stride, pad, dil)
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(dy_seed))
    y.backward(dy.double())
    return y.detach(), dy, x64.grad, w64.grad


# ------------------------------------------------------------------------------------------------------------ rectangular convolution
RECT_CASES = [(n, h, w, 32, 32, k, p, 1) for k, p in (((5, 1), (2, 0)), ((1, 5), (0, 2))) for n, h, w in ((2, 1, 1), (2, 2, 7), (2, 7, 2), (1, 9, 12))]
RECT_CASES += [(2, 9, 12, 16, 8, (5, 1), (2, 0), 2), (2, 9, 12, 16, 8, (1, 5), (0, 2), 2)]


@pytest.mark.parametrize("n,h,w,cin,cout,k,pad,stride", RECT_CASES)
def test_rect_conv_matches_float64(pkg, n, h, w, cin, cout, k, pad, stride):
    """ops.conv_rect_fwd / _dgrad / _wgrad against float64 F.conv2d and its autograd, maps shorter than the kernel included; the output and
    the data gradient written into channel slices of wider buffers, the data gradient also accumulated"""
    ops = _mod("ops")
    g = torch.Generator().manual_seed(13 * h + 7 * w + k[0] + stride)
    x, wt = torch.randn((n, cin, h, w), generator=g), torch.randn((cout, cin) + k, generator=g) / (cin * k[0] * k[1]) ** 0.5
    y64, dy, dx64, dw64 = _conv_ref(x, wt, stride, pad, 1, 5)
    xd, wd, dyd = _nhwc(x).to(DEV), _hwio(wt), _nhwc(dy).to(DEV)
    runs = []
    for _ in range(2):
        ys, ybuf = _in_slice(torch.zeros((n,) + tuple(y64.shape[2:]) + (cout,), device=DEV), 4, cout + 8)
        keep = ybuf.clone()
        ops.conv_rect_fwd(xd, wd, None, stride, pad, out=ys)
        dxs, dxbuf = _in_slice(torch.zeros((n, h, w, cin), device=DEV), 8, cin + 12)
        keepx = dxbuf.clone()
        ops.conv_rect_dgrad(dyd, wd, h, w, stride, pad, out=dxs)
        dw = ops.conv_rect_wgrad(xd, dyd, k[0], k[1], stride, pad)
        acc = torch.full((n, h, w, cin), 3.0, device=DEV)
        ops.conv_rect_dgrad(dyd, wd, h, w, stride, pad, out=acc, accumulate=True)
        torch.cuda.synchronize()
        assert _same(ybuf[..., :4], keep[..., :4]) and _same(ybuf[..., 4 + cout:], keep[..., 4 + cout:])
        assert _same(dxbuf[..., :8], keepx[..., :8]) and _same(dxbuf[..., 8 + cin:], keepx[..., 8 + cin:])
        runs.append((ys.clone(), dxs.clone(), dw, acc))
    for a, b in zip(*runs):
        assert _same(a, b)
    y, dx, dw, acc = runs[0]
    errs = dict(y=_err(_nchw(y), y64), dx=_err(_nchw(dx), dx64), dx_acc=_err(_nchw(acc) - 3.0, dx64), dw=_err(dw.permute(3, 2, 0, 1), dw64))
    print(f"\nrect {k} pad {pad} s{stride} {n}x{h}x{w} {cin}->{cout}: " + " ".join(f"{kk} {v:.1e}" for kk, v in errs.items()))
    assert max(errs["y"], errs["dx"], errs["dx_acc"]) <= CONV_BAND and errs["dw"] <= _wgrad_band(y64.shape[0] * y64.shape[2] * y64.shape[3]), errs


@pytest.mark.parametrize("k,stride,pad,dil,cin,cout", [(3, 1, 1, 1, 32, 32), (3, 2, 1, 1, 16, 8), (3, 1, 4, 4, 32, 32), (5, 1, 2, 1, 16, 8),
                                                      (2, 2, 0, 1, 16, 8)])
def test_rect_conv_equals_general_on_symmetric_arguments(pkg, k, stride, pad, dil, cin, cout):
    """equal pads and dilations: runet_conv2d_rect / runet_conv_wgrad_rect give runet_conv2d_general's / runet_conv_wgrad_general's bits"""
    ops = _mod("ops")
    n, h, w = 2, 10, 14
    g = torch.Generator().manual_seed(k + stride + dil)
    xd = torch.randn((n, h, w, cin), generator=g).to(DEV)
    wd = (torch.randn((k, k, cin, cout), generator=g) / (cin * k * k) ** 0.5).to(DEV)
    ho, wo = ops.conv_out_hw(h, w, k, stride, pad, dil)
    dyd = torch.randn((n, ho, wo, cout), generator=g).to(DEV)
    assert _same(ops.conv_rect_fwd(xd, wd, None, stride, (pad, pad), (dil, dil)), ops.conv_general_fwd(xd, wd, None, stride, pad, dil))
    assert _same(ops.conv_rect_dgrad(dyd, wd, h, w, stride, (pad, pad), (dil, dil)), ops.conv_general_dgrad(dyd, wd, h, w, stride, pad, dil))
    assert _same(ops.conv_rect_wgrad(xd, dyd, k, k, stride, (pad, pad), (dil, dil)), ops.conv_general_wgrad(xd, dyd, k, k, stride, pad, dil))


# ------------------------------------------------------------------------------------------------------------ small and dilated shared convolutions
SMALL = [("16->4 1x1 s2", 16, 4, 1, 2, 1, (2, 6, 10)), ("4->4 3x3", 4, 4, 3, 1, 1, (2, 6, 10)), ("4->64 1x1", 4, 64, 1, 1, 1, (2, 6, 10))]
SMALL += [(f"32->32 3x3 dil {d}", 32, 32, 3, 1, d, shp) for d in (2, 4, 8, 16) for shp in ((2, 8, 8), (1, 18, 17))]


@pytest.mark.parametrize("what,cin,cout,k,stride,dil,shape", SMALL, ids=[f"{c[0]} {c[6]}" for c in SMALL])
def test_shared_convs_at_enet_widths_match_float64(pkg, what, cin, cout, k, stride, dil, shape):
    """the calls the model makes - ops.conv_fwd / conv_dgrad / conv_wgrad (stride 1, padding = dilation), ops.conv_general_* (the stride-2
    1x1) - at encoder1.0's 4-channel widths and encoder2's dilations; 1 x 18 x 17 has live off-centre taps at dilation 16"""
    ops = _mod("ops")
    n, h, w = shape
    pad = dil * (k // 2)
    g = torch.Generator().manual_seed(cin + cout + dil + h)
    x, wt = torch.randn((n, cin, h, w), generator=g), torch.randn((cout, cin, k, k), generator=g) / (cin * k * k) ** 0.5
    y64, dy, dx64, dw64 = _conv_ref(x, wt, stride, pad, dil, 6)
    xd, wd, dyd = _nhwc(x).to(DEV), _hwio(wt), _nhwc(dy).to(DEV)
    runs = []
    for _ in range(2):
        if stride == 1:
            y = ops.conv_fwd(xd, wd, None, dil=dil)
            acc = torch.full((n, h, w, cin), 3.0, device=DEV)
            ops.conv_dgrad(dyd, wd, out=acc, dil=dil, accumulate=True)
            dx = ops.conv_dgrad(dyd, wd, dil=dil)
            dw = ops.conv_wgrad(xd, dyd, k, k, dil=dil)
        else:
            y = ops.conv_general_fwd(xd, wd, None, stride, pad)
            acc = torch.full((n, h, w, cin), 3.0, device=DEV)
            ops.conv_general_dgrad(dyd, wd, h, w, stride, pad, out=acc, accumulate=True)
            dx = ops.conv_general_dgrad(dyd, wd, h, w, stride, pad)
            dw = ops.conv_general_wgrad(xd, dyd, k, k, stride, pad)
        torch.cuda.synchronize()
        runs.append((y, dx, acc, dw))
    for a, b in zip(*runs):
        assert _same(a, b)
    y, dx, acc, dw = runs[0]
    errs = dict(y=_err(_nchw(y), y64), dx=_err(_nchw(dx), dx64), dx_acc=_err(_nchw(acc) - 3.0, dx64), dw=_err(dw.permute(3, 2, 0, 1), dw64))
    print(f"\n{what} {shape}: " + " ".join(f"{kk} {v:.1e}" for kk, v in errs.items()))
    assert max(errs["y"], errs["dx"], errs["dx_acc"]) <= CONV_BAND and errs["dw"] <= _wgrad_band(y64.shape[0] * y64.shape[2] * y64.shape[3]), errs


# ------------------------------------------------------------------------------------------------------------ k3-s2 transposed convolution
@pytest.mark.parametrize("n,h,w,cin,cout", [(2, 1, 1, 128, 64), (2, 3, 5, 64, 16), (1, 8, 8, 128, 64)])
def test_convt3_matches_float64(pkg, n, h, w, cin, cout):
    """ops.convt3_fwd / _dgrad / _wgrad (+ blocks.chan_sum for the bias) against float64 F.conv_transpose2d(stride 2, padding 1,
    output_padding 1) with bias and its autograd.  The forward in both forms: runet_convt3_fwd's four parity-class GEMMs (also into a channel
    slice) and the data-gradient mode of the general convolution, which adds the bias in its epilogue"""
    ops, B = _mod("ops"), _mod("blocks")
    g = torch.Generator().manual_seed(n + h + w + cin)
    x, wt, b = torch.randn((n, cin, h, w), generator=g), torch.randn((cin, cout, 3, 3), generator=g) / (cin * 9) ** 0.5, torch.randn(cout, generator=g)
    dy = torch.randn((n, cout, 2 * h, 2 * w), generator=g)
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, wt, b))
    y64 = F.conv_transpose2d(x64, w64, b64, 2, 1, 1)
    y64.backward(dy.double())
    xd, dyd, bd = _nhwc(x).to(DEV), _nhwc(dy).to(DEV), b.to(DEV)
    wp = torch.nn.Parameter(torch.empty(3, 3, cin, cout).permute(2, 3, 0, 1))       # the holder's storage: logical [cin, cout, 3, 3], memory [3][3][cin][cout]
    with torch.no_grad():
        wp.copy_(wt)
    wd = ops.hwio_t(wp.to(DEV))
    assert wd.is_contiguous() and tuple(wd.shape) == (3, 3, cin, cout)
    runs = []
    for _ in range(2):
        y = ops.convt3_fwd(xd, wd, bd, classes=True)
        ys, ybuf = _in_slice(torch.zeros((n, 2 * h, 2 * w, cout), device=DEV), 4, cout + 8)
        keep = ybuf.clone()
        ops.convt3_fwd(xd, wd, bd, out=ys, classes=True)
        assert _same(ys, y) and _same(ybuf[..., :4], keep[..., :4]) and _same(ybuf[..., 4 + cout:], keep[..., 4 + cout:])
        y_dg = ops.convt3_fwd(xd, wd, bd, classes=False)
        dx = ops.convt3_dgrad(dyd, wd)
        dw = ops.convt3_wgrad(xd, dyd)
        db = B.chan_sum(dyd, B.vec(cout, torch.device(DEV)))
        torch.cuda.synchronize()
        runs.append((y, y_dg, dx, dw, db))
    for a, c in zip(*runs):
        assert _same(a, c)
    y, y_dg, dx, dw, db = runs[0]
    assert y.shape == (n, 2 * h, 2 * w, cout) and dx.shape == (n, h, w, cin) and dw.shape == (3, 3, cin, cout)
    errs = dict(y=_err(_nchw(y), y64.detach()), y_dgrad_form=_err(_nchw(y_dg), y64.detach()), dx=_err(_nchw(dx), x64.grad), dw=_err(dw.permute(2, 3, 0, 1), w64.grad), db=_err(db, b64.grad))
    print(f"\nconvt3 {n}x{h}x{w} {cin}->{cout}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs["y"], errs["y_dgrad_form"], errs["dx"], errs["db"]) <= CONV_BAND and errs["dw"] <= _wgrad_band(n * h * w), errs


# ------------------------------------------------------------------------------------------------------------ initial block
@pytest.mark.parametrize("n,H,W,crop", [(1, 2, 2, False), (2, 2, 6, False), (2, 6, 2, False), (3, 10, 14, False), (1, 66, 34, False), (2, 12, 20, True)])
def test_initial_block_fused_and_partner_match_float64(pkg, n, H, W, crop):
    """blocks.enet_initial_forward / _backward on runet_enet_initial_* and on the shared kernels: t = cat(conv, pool), the mean / invstd
    finalised from the partials, the activation, the BatchNorm sums and the convolution's weight gradient, against float64 F.conv2d /
    F.max_pool2d / torch.cat / F.batch_norm; crop: a non-contiguous window of a larger image"""
    B = _mod("blocks")
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(3 * n + 5 * H + W)
    big = torch.randn((n, 3, H + 6, W + 10), generator=g)
    x = big[:, :, 2:2 + H, 4:4 + W] if crop else big[:, :, :H, :W].contiguous()
    wt = torch.randn((13, 3, 3, 3), generator=g) / 27 ** 0.5
    ga, be = 1 + 0.2 * torch.randn(16, generator=g), 0.2 * torch.randn(16, generator=g)
    da = torch.randn((n, 16, H // 2, W // 2), generator=g)
    w64, ga64, be64 = (t.double().requires_grad_(True) for t in (wt, ga, be))
    t64 = torch.cat([F.conv2d(x.double(), w64, None, 2, 1), F.max_pool2d(x.double(), 2, 2)], 1)
    tr = n * (H // 2) * (W // 2) > 1          # one value per channel: F.batch_norm and runet_bn_stats both refuse it in training mode - eval there
    a64 = F.relu(F.batch_norm(t64, torch.zeros(16, dtype=torch.float64), torch.ones(16, dtype=torch.float64), ga64, be64, tr, 0.1, EPS))
    a64.backward(da.double())
    xd = big.to(DEV)[:, :, 2:2 + H, 4:4 + W] if crop else x.to(DEV)
    assert xd.is_contiguous() != crop
    wd = _hwio(wt)
    res = {}
    for fused in (True, False):
        runs = []
        for _ in range(2):
            bn = B.BNState(ga.to(DEV), be.to(DEV), torch.zeros(16, device=DEV), torch.ones(16, device=DEV), torch.zeros((), dtype=torch.int64, device=DEV))
            a, cx = B.enet_initial_forward(xd, wd, bn, tr, B.Small(dev), fused=fused)
            G = {}
            B.enet_initial_backward(cx, _nhwc(da).to(DEV), G, "initial.", tr)
            torch.cuda.synchronize()
            runs.append((a, cx["t"], cx["mean"], cx["invstd"], G["initial.conv.weight"], G["initial.bn.weight"], G["initial.bn.bias"], bn.running_mean))
        for p, q in zip(*runs):
            assert _same(p, q)
        a, t, mean, invstd, dw, dga, dbe, rm = runs[0]
        assert ("x" in cx) == fused and dw.shape == (3, 3, 3, 13) and a.shape == (n, H // 2, W // 2, 16)
        errs = dict(t=_err(_nchw(t), t64.detach()), a=_err(_nchw(a), a64.detach()), dw=_err(dw.permute(3, 2, 0, 1), w64.grad),
                    dgamma=_err(dga, ga64.grad), dbeta=_err(dbe, be64.grad))
        if tr:
            errs.update(mean=_err(mean, t64.detach().mean((0, 2, 3))), running_mean=_err(rm, 0.1 * t64.detach().mean((0, 2, 3))),
                        invstd=_err(invstd, 1 / torch.sqrt(t64.detach().var((0, 2, 3), unbiased=False) + EPS)))
        print(f"\ninitial {n}x{H}x{W}{' crop' if crop else ''} ({'fused' if fused else 'partner'}): " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        dw_err = errs.pop("dw")
        assert max(errs.values()) <= BAND and dw_err <= (BAND if fused else _wgrad_band(n * (H // 2) * (W // 2))), (fused, errs, dw_err)
        res[fused] = (t, a, dw)
    assert _same(res[True][0][..., 13:], res[False][0][..., 13:])          # the pool is exact on both paths
    assert _err(res[True][0], res[False][0]) <= BAND and _err(res[True][1], res[False][1]) <= BAND
    assert _err(res[True][2], res[False][2]) <= _wgrad_band(n * (H // 2) * (W // 2))


# ------------------------------------------------------------------------------------------------------------ bottleneck tail
def _tail_case(n, h, w, c, down, training, masked, seed):
    """float64 reference of relu(mask * bn3(t3) + id) and its gradients, redrawn on the reference only until no pre-ReLU value is within 1e-5
    of zero (a mask there could differ between fp32 and float64), as test_gpu_fastscnn._ffm_case does"""
    for draw in range(64):
        g = torch.Generator().manual_seed(seed + 1000 * draw)
        t3, idn, dout = (torch.randn((n, c, h, w), generator=g) for _ in range(3))
        par = {k: (1 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g), 0.3 * torch.randn(c, generator=g),
                   0.5 + torch.rand(c, generator=g)) for k in ("3", "d")}
        mask = None
        if masked:          # p = 0.25, one channel dropped in every image (another one per image)
            mask = torch.full((n, c), 1 / 0.75)
            for i in range(n):
                mask[i, (i * 3 + 1) % c] = 0.0
        t64, i64 = t3.double().requires_grad_(True), idn.double().requires_grad_(True)
        leaf = {k: tuple(v.double().requires_grad_(i < 2) for i, v in enumerate(par[k])) for k in par}

        def bn(t, k):
            ga, be, rm, rv = leaf[k]
            return F.batch_norm(t, rm.clone(), rv.clone(), ga, be, training, 0.1, EPS)
        y3 = bn(t64, "3")
        y3.retain_grad()
        main = y3 * mask.double()[:, :, None, None] if masked else y3
        ident = bn(i64, "d") if down else i64
        ident.retain_grad()
        pre = main + ident
        if float(pre.detach().abs().min()) > 1e-5:
            out = F.relu(pre)
            out.backward(dout.double())
            return dict(t3=t3, idn=idn, dout=dout, par=par, mask=mask, out=out.detach(), dt3=t64.grad, did=i64.grad, dy3=y3.grad, dident=ident.grad,
                        leaf=leaf, draws=draw + 1)
    raise AssertionError("no draw without a pre-ReLU value within 1e-5 of zero")


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("down", [False, True], ids=["plain", "downsample"])
@pytest.mark.parametrize("c", [4, 64, 128])
@pytest.mark.parametrize("n,h,w", [(2, 1, 1), (2, 3, 5), (3, 7, 4)])
def test_tail_fused_and_partner_match_float64(pkg, n, h, w, c, down, training, masked):
    """blocks.enet_tail_forward / _backward on runet_enet_tail_* and on the shared kernels against float64 autograd: out, dt3, dt_d (downsample)
    or the identity's gradient (plain), and both BatchNorms' dgamma / dbeta, with batch and with running statistics, without and with a
    Dropout2d mask that drops one channel in every image (the kernels apply a mask whenever one is given; the model gives none in eval mode).
    2 x 1 x 1 in training mode is the two-values-per-channel BatchNorm: its input gradient cancels analytically to five orders below the
    terms it is made of (test_gpu_fastscnn.test_ffm_matches_float64), so dt3 / dt_d there are measured against the size of the cancelling
    terms, max |scale| * max |gradient of the BatchNorm's output|; every other figure keeps max |want|."""
    B = _mod("blocks")
    dev = torch.device(DEV)
    ref = _tail_case(n, h, w, c, down, training, masked, 31 * n + 7 * h + w + c + 2 * down + training)
    assert ref["draws"] <= 8, ref["draws"]
    t3, idn, dout = (_nhwc(ref[k]).to(DEV) for k in ("t3", "idn", "dout"))
    mask = ref["mask"].to(DEV) if masked else None
    res = {}
    for fused in (True, False):
        runs = []
        for _ in range(2):
            sm = B.Small(dev)
            co = {}
            for k, t in (("3", t3), ("d", idn)):
                ga, be, rm, rv = ref["par"][k]
                bn = B.BNState(ga.to(DEV), be.to(DEV), rm.clone().to(DEV), rv.clone().to(DEV), torch.zeros((), dtype=torch.int64, device=DEV))
                co[k] = B.bn_coeff(t, bn, training, sm)[:4]
            s3, h3, m3, i3 = co["3"]
            sd, hd, md, ivd = co["d"]
            out = B.enet_tail_forward(t3, (s3, h3), idn, (sd, hd) if down else None, mask, fused=fused)
            dt3, did, sums3, sums_d = B.enet_tail_backward(dout, out, t3, (m3, i3, s3), idn if down else None, (md, ivd, sd) if down else None,
                                                           mask, training, fused=fused)
            torch.cuda.synchronize()
            runs.append((out, dt3, did, sums3) + ((sums_d,) if down else ()))
        for a, b in zip(*runs):
            assert _same(a, b)
        out, dt3, did, sums3 = runs[0][:4]
        errs = dict(out=_err(_nchw(out), ref["out"]), dt3=_err(_nchw(dt3), ref["dt3"]), did=_err(_nchw(did), ref["did"] if down else ref["dident"]),
                    dgamma3=_err(sums3[:c], ref["leaf"]["3"][0].grad), dbeta3=_err(sums3[c:], ref["leaf"]["3"][1].grad))
        if down:
            errs.update(dgamma_d=_err(runs[0][4][:c], ref["leaf"]["d"][0].grad), dbeta_d=_err(runs[0][4][c:], ref["leaf"]["d"][1].grad))
        if training and n * h * w == 2:
            for key, k, tk, gk in (("dt3", "3", "t3", "dy3"), ("did", "d", "idn", "dident")):
                if key == "did" and not down:
                    continue
                ga = ref["par"][k][0]
                invstd = 1.0 / torch.sqrt(ref[tk].double().var((0, 2, 3), unbiased=False) + EPS)
                terms = max(float((ga.double() * invstd).abs().max()) * float(ref[gk].abs().max()), 1e-30)      # all of g masked off: exactly zero
                got = dt3 if key == "dt3" else did
                errs[key] = float((_nchw(got).double().cpu() - ref[key]).abs().max()) / terms
        print(f"\ntail {n}x{h}x{w} c={c} {'downsample' if down else 'plain'} {'train' if training else 'eval'} {'mask' if masked else 'nomask'} "
              f"({'fused' if fused else 'partner'}, {ref['draws']} draw(s)): " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        assert max(errs.values()) <= BAND, (fused, errs)
        res[fused] = out
    assert _err(res[True], res[False]) <= BAND


# ------------------------------------------------------------------------------------------------------------ head
@pytest.mark.parametrize("n,h,w,c", [(2, 1, 1, 16), (3, 5, 7, 16), (1, 33, 17, 16), (2, 4, 4, 4)])
def test_head_matches_float64(pkg, n, h, w, c):
    """runet_enet_head_fwd / _bwd against float64 sigmoid(F.conv_transpose2d(x, w, b, stride 2)) of a [c, 1, 2, 2] weight and its autograd;
    x and dx are channel slices of wider buffers"""
    B = _mod("blocks")
    g = torch.Generator().manual_seed(11 * n + 3 * h + w + c)
    x, wt, b = torch.randn((n, c, h, w), generator=g), torch.randn((c, 1, 2, 2), generator=g) / c ** 0.5, torch.randn(1, generator=g)
    dprob = torch.randn((n, 1, 2 * h, 2 * w), generator=g)
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, wt, b))
    p64 = torch.sigmoid(F.conv_transpose2d(x64, w64, b64, 2))
    p64.backward(dprob.double())
    xs, _ = _in_slice(_nhwc(x).to(DEV), 4, c + 8)
    wd, bd, dpd = wt.permute(2, 3, 0, 1).contiguous().to(DEV), b.to(DEV), dprob.to(DEV)
    runs = []
    for _ in range(2):
        sink = B.DictSink(torch.device(DEV))
        prob = B.enet_head_forward(xs, wd, bd)
        dx = B.enet_head_backward(dpd, prob, xs, wd, sink, "decoder.6.")
        torch.cuda.synchronize()
        runs.append((prob, dx, sink.g["decoder.6.weight"], sink.g["decoder.6.bias"]))
    for a, c_ in zip(*runs):
        assert _same(a, c_)
    prob, dx, dw, db = runs[0]
    assert prob.shape == (n, 1, 2 * h, 2 * w) and dw.shape == (2, 2, c, 1) and db.shape == (1,)
    errs = dict(prob=_err(prob, p64.detach()), dx=_err(_nchw(dx), x64.grad), dw=_err(dw.permute(2, 3, 0, 1), w64.grad), db=_err(db, b64.grad))
    print(f"\nhead {n}x{h}x{w} c={c}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= BAND, errs


# ------------------------------------------------------------------------------------------------------------ channel slices
# Every entry of csrc/enet.hip takes its sources and destinations as channel slices of wider buffers, each with a pixel stride of its own.  The
# tests above run them dense (pixel stride = c), where a swapped stride argument or a `c` in a stride's place would go unnoticed: here every
# tensor sits at another offset of a buffer of another width, the results must equal the dense run bit for bit and the buffers' other channels
# must keep their bits.
def _slices(shapes_lo_wide, fill=None):
    """{name: (shape, lo, wide)} -> ({name: slice view}, {name: buffer}, {name: the buffer's bits before the run})"""
    views, bufs = {}, {}
    for k, (shape, lo, wide) in shapes_lo_wide.items():
        src = fill[k] if fill and k in fill else torch.zeros(shape, device=DEV)
        views[k], bufs[k] = _in_slice(src, lo, wide)
    return views, bufs, {k: b.clone() for k, b in bufs.items()}


def _neighbours_kept(bufs, keep, spec):
    for k, (shape, lo, wide) in spec.items():
        c = shape[3]
        assert _same(bufs[k][..., :lo], keep[k][..., :lo]) and _same(bufs[k][..., lo + c:], keep[k][..., lo + c:]), k


@pytest.mark.parametrize("down", [False, True], ids=["plain", "downsample"])
def test_tail_kernels_take_channel_slices(pkg, down):
    """runet_enet_tail_fwd / _bwd_reduce / _bwd_apply with t3, idn and dout read from slices and out, dt3 and did written into slices, six
    different pixel strides and offsets, against the dense run of the same calls"""
    L, ops = _mod("_lib"), _mod("ops")
    lib, check, ld = L.lib, L.check, ops.ld
    n, h, w, c = 2, 3, 5, 8
    g = torch.Generator().manual_seed(41 + down)
    src = {k: torch.randn((n, h, w, c), generator=g).to(DEV) for k in ("t3", "idn", "dout")}
    v = {k: torch.randn(c, generator=g).to(DEV) for k in ("s3", "h3", "sd", "hd", "m3", "md")}
    v.update({k: (0.5 + torch.rand(c, generator=g)).to(DEV) for k in ("i3", "ivd")})
    mask = torch.full((n, c), 1 / 0.75)
    mask[0, 1], mask[1, 6] = 0.0, 0.0
    mask = mask.to(DEV)
    st = ops.stream()
    nws = lib.runet_enet_tail_bwd_workspace_floats(n, h, w, c, int(down))
    assert nws == (4 if down else 2) * c
    P = lambda t: t.data_ptr()          # noqa: E731
    D = lambda t: P(t) if down else None          # noqa: E731

    def run(T):
        ws, sums = torch.empty(nws, device=DEV), torch.empty((4 if down else 2) * c, device=DEV)
        check(lib.runet_enet_tail_fwd(P(T["t3"]), ld(T["t3"]), P(T["idn"]), ld(T["idn"]), P(v["s3"]), P(v["h3"]), D(v["sd"]), D(v["hd"]), P(mask),
                                      P(T["out"]), ld(T["out"]), n, h, w, c, st))
        check(lib.runet_enet_tail_bwd_reduce(P(T["dout"]), ld(T["dout"]), P(T["out"]), ld(T["out"]), P(T["t3"]), ld(T["t3"]), D(T["idn"]),
                                             ld(T["idn"]) if down else 0, P(v["m3"]), P(v["i3"]), D(v["md"]), D(v["ivd"]), P(mask), P(ws), nws, P(sums),
                                             n, h, w, c, st))
        check(lib.runet_enet_tail_bwd_apply(P(T["dout"]), ld(T["dout"]), P(T["out"]), ld(T["out"]), P(T["t3"]), ld(T["t3"]), D(T["idn"]),
                                            ld(T["idn"]) if down else 0, P(v["m3"]), P(v["i3"]), P(v["s3"]), D(v["md"]), D(v["ivd"]), D(v["sd"]), P(mask),
                                            P(sums), 0, P(T["dt3"]), ld(T["dt3"]), P(T["did"]), ld(T["did"]), n, h, w, c, st))
        torch.cuda.synchronize()
        return sums
    dense = dict(src, **{k: torch.zeros((n, h, w, c), device=DEV) for k in ("out", "dt3", "did")})
    sums_dense = run(dense)
    shp = (n, h, w, c)
    spec = dict(t3=(shp, 4, c + 8), idn=(shp, 8, c + 12), dout=(shp, 4, c + 16), out=(shp, 12, c + 24), dt3=(shp, 8, c + 28), did=(shp, 4, c + 20))
    views, bufs, keep = _slices(spec, fill=src)
    assert len({ld(t) for t in views.values()}) == 6
    sums = run(views)
    _neighbours_kept(bufs, keep, spec)
    assert _same(sums, sums_dense)
    for k in ("out", "dt3", "did"):
        assert _same(views[k], dense[k]), k
    assert float(dense["out"].abs().max()) > 0 and float(dense["dt3"].abs().max()) > 0 and float(dense["did"].abs().max()) > 0


def test_head_kernels_take_channel_slices(pkg):
    """runet_enet_head_fwd / _bwd with x read from a slice and dx written into a slice of another width, against the dense run"""
    L, ops = _mod("_lib"), _mod("ops")
    lib, check, ld = L.lib, L.check, ops.ld
    n, h, w, c = 2, 5, 7, 16
    g = torch.Generator().manual_seed(43)
    x = torch.randn((n, h, w, c), generator=g).to(DEV)
    wd, bd = (torch.randn((2, 2, c, 1), generator=g) / c ** 0.5).to(DEV), torch.randn(1, generator=g).to(DEV)
    dprob = torch.randn((n, 1, 2 * h, 2 * w), generator=g).to(DEV)
    st = ops.stream()
    nws = lib.runet_enet_head_bwd_workspace_floats(n, h, w, c)

    def run(X, DX):
        prob, ws, dw_db = torch.empty((n, 1, 2 * h, 2 * w), device=DEV), torch.empty(nws, device=DEV), torch.empty(4 * c + 1, device=DEV)
        check(lib.runet_enet_head_fwd(X.data_ptr(), ld(X), wd.data_ptr(), bd.data_ptr(), prob.data_ptr(), n, h, w, c, st))
        check(lib.runet_enet_head_bwd(dprob.data_ptr(), prob.data_ptr(), X.data_ptr(), ld(X), wd.data_ptr(), DX.data_ptr(), ld(DX), ws.data_ptr(), nws,
                                      dw_db.data_ptr(), n, h, w, c, st))
        torch.cuda.synchronize()
        return prob, dw_db
    dx_dense = torch.zeros((n, h, w, c), device=DEV)
    prob_dense, dwdb_dense = run(x, dx_dense)
    shp = (n, h, w, c)
    spec = dict(x=(shp, 4, c + 8), dx=(shp, 12, c + 20))
    views, bufs, keep = _slices(spec, fill=dict(x=x))
    prob, dwdb = run(views["x"], views["dx"])
    _neighbours_kept(bufs, keep, spec)
    assert _same(prob, prob_dense) and _same(dwdb, dwdb_dense) and _same(views["dx"], dx_dense) and float(dx_dense.abs().max()) > 0


def test_initial_kernels_take_channel_slices(pkg):
    """runet_enet_initial_fwd writing t into a 16-channel slice and runet_enet_initial_wgrad reading dt from a slice of another width, against
    the dense run; 3 x 10 x 14 and 1 x 66 x 34 (three 256-pixel parts)"""
    L, ops = _mod("_lib"), _mod("ops")
    lib, check, ld = L.lib, L.check, ops.ld
    st = ops.stream()
    for n, H, W in ((3, 10, 14), (1, 66, 34)):
        g = torch.Generator().manual_seed(47 + H)
        x = torch.randn((n, 3, H, W), generator=g).to(DEV)
        w13 = (torch.randn((3, 3, 3, 13), generator=g) / 27 ** 0.5).to(DEV)
        dt = torch.randn((n, H // 2, W // 2, 16), generator=g).to(DEV)
        parts, nws = lib.runet_enet_initial_parts(n, H, W), lib.runet_enet_initial_wgrad_workspace_floats(n, H, W)
        sn, sc, sh, sw = x.stride()

        def run(T, DT):
            part, ws, dw = torch.empty(parts * 16 * 3, device=DEV), torch.empty(nws, device=DEV), torch.empty((3, 3, 3, 13), device=DEV)
            check(lib.runet_enet_initial_fwd(x.data_ptr(), sn, sc, sh, sw, w13.data_ptr(), T.data_ptr(), ld(T), part.data_ptr(), n, H, W, st))
            check(lib.runet_enet_initial_wgrad(x.data_ptr(), sn, sc, sh, sw, DT.data_ptr(), ld(DT), ws.data_ptr(), nws, dw.data_ptr(), n, H, W, st))
            torch.cuda.synchronize()
            return part, dw
        t_dense = torch.zeros((n, H // 2, W // 2, 16), device=DEV)
        part_dense, dw_dense = run(t_dense, dt)
        shp = (n, H // 2, W // 2, 16)
        spec = dict(t=(shp, 4, 28), dt=(shp, 8, 36))
        views, bufs, keep = _slices(spec, fill=dict(dt=dt))
        keep_dt = bufs["dt"].clone()
        part, dw = run(views["t"], views["dt"])
        _neighbours_kept(bufs, keep, spec)
        assert _same(bufs["dt"], keep_dt)          # a source: untouched altogether
        assert _same(part, part_dense) and _same(dw, dw_dense) and _same(views["t"], t_dense) and float(dw_dense.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------ model
def _net(pkg, st, masks=None):
    net = pkg.ENet()
    res = net.load_state_dict(st, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    net.set_dropout_masks(masks)
    return net.to(DEV).train()


def _pick(gold, key, t):
    t = t.detach().cpu().double().reshape(-1)
    if key in gold:
        return t.float().numpy(), gold[key].reshape(-1)
    stride, numel, k = (int(v) for v in gold[key + "/meta"])
    assert t.numel() == numel
    return t[::stride][:k].float().numpy(), gold[key + "/sample"]


def _golden_step(pkg, tag):
    """one train step (BCELoss, FusedAdam 1e-4, weight decay 1e-4) under the fixture's dropout masks and an eval forward on a fixture's inputs
    -> CPU tensors"""
    meta = json.load(open(os.path.join(GOLDEN, f"enet_{tag}.json")))
    net = _net(pkg, eref.init_state(seed=meta["seed"], perturb_bn=True), eref.dropout_masks(meta["n"], meta["seed"]))
    x, y = pkg.synthetic_batch(meta["n"], meta["size"], seed=meta["seed"])
    opt = pkg.FusedAdam(net.parameters(), lr=1e-4, weight_decay=1e-4)
    opt.zero_grad()
    prob = net(x.to(DEV))
    loss = pkg.bce_loss(prob, y.to(DEV))
    loss.backward()
    res = dict(prob=prob.detach().cpu(), loss=float(loss.detach()), names=[k for k, _ in net.named_parameters()],
               grads=[p.grad.detach().cpu().clone() for p in net.parameters()], bufs={k: b.detach().cpu().clone() for k, b in net.named_buffers()})
    opt.step()
    res["adam"] = [p.detach().cpu().clone() for p in net.parameters()]
    net.eval()
    with torch.no_grad():
        res["eval_prob"] = net(x.to(DEV)).cpu()
    return res


def _check_golden_step(tag, res, what):
    """test_gpu_fastscnn._check_golden_step's bands: probabilities, loss, gradient norms, sampled gradients, BatchNorm buffers, the Adam step
    and the eval forward; the analytically zero gradients (enet_ref.ZERO_GRAD: the transposed convolutions' biases in front of a train-mode
    BatchNorm) within 1e-4 of the largest gradient norm, absolute."""
    meta = json.load(open(os.path.join(GOLDEN, f"enet_{tag}.json")))
    gold = load_npz(f"enet_{tag}.npz")
    a, b = _pick(gold, "prob", res["prob"])
    assert np.abs(a - b).max() <= 1e-3, np.abs(a - b).max()
    assert abs(res["loss"] - float(gold["loss"])) <= 1e-4
    names = meta["param_names"]
    assert res["names"] == names
    gn = np.array([g.double().norm().item() for g in res["grads"]])
    ref = gold["grad_norm"]
    real = np.array([k not in eref.ZERO_GRAD for k in names])
    rel = np.abs(gn - ref) / (ref + 1e-3 * ref.max())
    print(f"\nENet {tag} ({what}): loss {res['loss']:.6f} (reference {float(gold['loss']):.6f}), worst gradient-norm error {rel[real].max():.1e}")
    assert rel[real].max() < 2e-2, (names[int(np.argmax(np.where(real, rel, 0)))], rel[real].max())
    gmax = max(float(np.abs(v).max()) for kk, v in gold.items() if kk.startswith("grad/") and not kk.endswith("/meta"))
    for k, g in zip(names, res["grads"]):
        a, b = _pick(gold, "grad/" + k, g)
        if k in eref.ZERO_GRAD:
            assert np.abs(a).max() <= 1e-4 * ref.max() and np.abs(b).max() <= 1e-4 * ref.max(), (k, np.abs(a).max())
            continue
        scale = max(float(np.abs(b).max()), 1e-3 * gmax)
        err = np.abs(a - b)
        assert err.max() <= 0.2 * scale and int((err > 3e-2 * scale).sum()) <= max(1, err.size // 100), (k, err.max(), scale)
        assert float(np.linalg.norm(a - b)) <= 1e-2 * scale * np.sqrt(err.size), (k, float(np.linalg.norm(a - b)), scale)
    for k, buf in res["bufs"].items():
        if f"buf/{k}" in gold:
            np.testing.assert_allclose(buf.numpy(), gold[f"buf/{k}"], rtol=2e-3, atol=2e-3, err_msg=k)
    for k, p in zip(names, res["adam"]):
        a, b = _pick(gold, "adam/" + k, p)
        assert np.abs(a - b).max() <= 2.1e-4, (k, np.abs(a - b).max())         # one Adam step moves each weight by at most lr
    a, b = _pick(gold, "eval_prob", res["eval_prob"])
    assert np.abs(a - b).max() <= 2e-3, np.abs(a - b).max()


TAGS = ("n2_s64", "n3_s96")
SWITCHES = ("RUNET_NO_FUSED_ENET_INITIAL", "RUNET_NO_FUSED_ENET_TAIL", "RUNET_NO_CONVT3_CLASSES")


@pytest.mark.parametrize("tag", TAGS)
def test_enet_train_step_matches_reference(pkg, tag):
    """loss, probabilities, gradients, BatchNorm buffers, Adam deltas and the eval forward of both fixtures (H/8 map 8 x 8: the dilations 8
    and 16 keep only their centre tap; and 12 x 12) at test_gpu_fastscnn.py's golden-step tolerances (_check_golden_step), in the default
    configuration (the fused initial block and tail)"""
    B = _mod("blocks")
    assert B.FUSED_ENET_INITIAL and B.FUSED_ENET_TAIL and _mod("ops").CONVT3_CLASSES, "run the suite without the RUNET_NO_FUSED_ENET_* / RUNET_NO_CONVT3_CLASSES switches"
    _check_golden_step(tag, _golden_step(pkg, tag), "default")


_AB_CODE = ("import importlib, sys, torch; sys.path[:0] = [%r, %r]; pkg = importlib.import_module(%r); import test_gpu_enet as T\n"
            "B = importlib.import_module(%r)\n"
            "assert (B.FUSED_ENET_INITIAL, B.FUSED_ENET_TAIL) == (sys.argv[2] != 'RUNET_NO_FUSED_ENET_INITIAL', sys.argv[2] != 'RUNET_NO_FUSED_ENET_TAIL')\n"
            "assert importlib.import_module(%r).CONVT3_CLASSES == (sys.argv[2] != 'RUNET_NO_CONVT3_CLASSES')\n"
            "torch.save({tag: T._golden_step(pkg, tag) for tag in T.TAGS}, sys.argv[1])\n" % (ROOT, os.path.join(ROOT, "tests"), PKG, PKG + ".blocks", PKG + ".ops"))


@pytest.mark.parametrize("switch", SWITCHES)
def test_enet_switches_give_the_same_step(pkg, switch):
    """each switch - the initial block and the tail from the shared kernels, the k3-s2 transposed forwards as a data gradient -, selected in a fresh child process (read at import), gives the
    golden train step of both fixtures within the same tolerances as the default (_check_golden_step): compared with the reference, not with
    the default step bit for bit (the summation orders differ, which can move a ReLU mask at a near-tie)"""
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"enet_ab_{switch}_{os.getpid()}.pt")
    r = subprocess.run([sys.executable, "-c", _AB_CODE, path, switch], env={**os.environ, switch: "1"}, timeout=600, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    other = torch.load(path)
    os.remove(path)
    for tag in TAGS:
        _check_golden_step(tag, other[tag], switch + "=1")


@pytest.mark.parametrize("n,size,seed", [(2, 64, 5), (3, 96, 6)])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "partners"])
def test_enet_gradients_under_the_hip_decisions(pkg, n, size, seed, fused, monkeypatch):
    """tests/decisions_seq.py's two-part check against the restatement in float64: ReLU masks on which the HIP step and the restatement differ
    are near-ties (decisions.NEAR_TIE), and under the HIP step's own decisions the worst and the median gradient error per tensor scale are
    bounded by what fp32 itself allows: the restatement run in float32 under the same forced decisions gives (worst32, median32) against
    float64, and the HIP step must stay within max(5e-4, 3 x worst32) and max(3e-5, 3 x median32) (test_gpu_fastscnn.py's bounds) - with
    both fused kernels on, and with both partners."""
    import decisions_seq as DS
    B, en = _mod("blocks"), _mod("enet")
    monkeypatch.setattr(B, "FUSED_ENET_INITIAL", fused)
    monkeypatch.setattr(B, "FUSED_ENET_TAIL", fused)
    st = eref.init_state(seed=seed, perturb_bn=True)
    masks = eref.dropout_masks(n, seed)
    net = _net(pkg, st, masks)
    x, y = pkg.synthetic_batch(n, size, seed=seed)
    got = {}
    real = en.enet_backward

    def spy(net_, C, dprob):
        got["dec"] = DE.hip_decisions(B, C, eref)
        return real(net_, C, dprob)
    monkeypatch.setattr(en, "enet_backward", spy)
    prob = net(x.to(DEV))
    pkg.bce_loss(prob, y.to(DEV)).backward()
    torch.cuda.synchronize()
    log, _, ref_prob, _ = eref.step(st, x, y, masks=masks)
    assert float((prob.detach().cpu().double() - ref_prob).abs().max()) <= 1e-3
    assert len(log) == len(got["dec"]) == len(eref.DECISION_SITES) == 44
    flips = DS.differing(got["dec"], log)
    DS.assert_near_ties(flips)
    _, gref, _, _ = eref.step(st, x, y, forced=got["dec"], masks=masks)
    _, g32, _, _ = eref.step(st, x, y, forced=got["dec"], dtype=torch.float32, masks=masks)
    skip = set(eref.ZERO_GRAD)
    rows = DS.grad_errors({k: p.grad.detach().cpu() for k, p in net.named_parameters()}, gref, skip)
    rows32 = DS.grad_errors({k: v.double() for k, v in g32.items()}, gref, skip)
    med, med32 = float(np.median([r[0] for r in rows])), float(np.median([r[0] for r in rows32]))
    print(f"\nENet {n} x {size}^2 ({'fused initial block and tail' if fused else 'partners'}): {len(flips)} near-tie decisions forced; "
          f"HIP worst {rows[0][0]:.1e} ({rows[0][1]}) median {med:.1e}; float32 restatement worst {rows32[0][0]:.1e} ({rows32[0][1]}) median {med32:.1e}")
    assert rows[0][0] <= max(5e-4, 3 * rows32[0][0]), (rows[:4], rows32[:4])
    assert med <= max(3e-5, 3 * med32), (med, med32)


def test_enet_sizes_and_bounds(pkg):
    """2 x 3 x 144 x 136 (H/8 map 18 x 17: live off-centre taps at dilation 16) and 2 x 3 x 16 x 24 (2 x 3) against the restatement, a
    non-contiguous input, eval mode with one 8 x 8 image, random dropout draws; what the model refuses.  Training-mode maps below 2 x 3 are
    no test of a kernel: at 2 x 3 x 8 x 16 encoder2's thirteen BatchNorms see four values per channel, and the float32 restatement itself is
    5.5e-3 away from the float64 one there (1.3e-5 at 16 x 24)."""
    st = eref.init_state(seed=9, perturb_bn=True)
    net = _net(pkg, st)
    for k, blk in net.blocks().items():          # no dropout: the draws are random
        blk.conv3[2].p, blk._p = 0.0, blk.conv3[2].p
    x, _ = pkg.synthetic_batch(2, 144, seed=9)
    for xs in (x[:, :, :, :136].contiguous(), x[:, :, 8:24, 16:40].contiguous()):
        with torch.no_grad():
            got = net(xs.to(DEV)).cpu()
            want = eref.forward({k: v.clone() for k, v in st.items()}, xs, True)
        assert got.shape == (2, 1) + tuple(xs.shape[2:])
        assert float((got - want).abs().max()) <= 1e-3, (tuple(xs.shape), float((got - want).abs().max()))
    with torch.no_grad():
        view = x.to(DEV)[:, :, 8:40, 16:48]
        assert not view.is_contiguous()
        got = net(view).cpu()
        want = eref.forward({k: v.clone() for k, v in st.items()}, x[:, :, 8:40, 16:48], True)
    assert float((got - want).abs().max()) <= 1e-3
    for k, blk in net.blocks().items():
        blk.conv3[2].p = blk._p
    xs, ys = pkg.synthetic_batch(2, 32, seed=10)
    loss = pkg.bce_loss(net(xs.to(DEV)), ys.to(DEV))          # random Dropout2d draws
    loss.backward()
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        net(xs[:1, :, :8, :8].to(DEV))
    net.eval()
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        got = net(xs[:1, :, :8, :8].to(DEV)).cpu()
        want = eref.forward(sd, xs[:1, :, :8, :8], False)
    assert float((got - want).abs().max()) <= 1e-3
    net.train()
    with pytest.raises(ValueError):
        net(torch.zeros((2, 3, 36, 32), device=DEV))
    with pytest.raises(ValueError):
        net(torch.zeros((2, 3, 32, 20), device=DEV))
    with pytest.raises(ValueError):
        net(torch.zeros((2, 4, 32, 32), device=DEV))
    with pytest.raises(TypeError):
        net(torch.zeros((2, 3, 32, 32), device=DEV, dtype=torch.float16))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "partners"])
def test_enet_step_is_deterministic_and_captures(pkg, fused, monkeypatch):
    """2 x 64^2 under injected dropout masks: two steps from an identical state give identical bits; TrainStep(graph=True) replay == eager,
    bit for bit, with p.grad at fixed addresses - with the initial block and the tail on either path."""
    trainer, B = _mod("trainer"), _mod("blocks")
    monkeypatch.setattr(B, "FUSED_ENET_INITIAL", fused)
    monkeypatch.setattr(B, "FUSED_ENET_TAIL", fused)
    st = eref.init_state(seed=3, perturb_bn=True)
    masks = eref.dropout_masks(2, 3)
    x, y = pkg.synthetic_batch(2, 64, seed=31)
    x, y = x.to(DEV), y.to(DEV)
    runs = []
    for _ in range(2):
        net = _net(pkg, st, masks)
        loss = pkg.bce_loss(net(x), y)
        loss.backward()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss))
        runs.append((loss.detach().clone(), [p.grad.detach().clone() for p in net.parameters()], [b.detach().clone() for b in net.buffers()]))
        del net
    assert _same(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1] + runs[0][2], runs[1][1] + runs[1][2]):
        assert torch.equal(a, b)
    res = {}
    for graph in (False, True):
        net = _net(pkg, st, {k: m.to(DEV) for k, m in masks.items()})
        step = trainer.TrainStep(net, lr=1e-3, weight_decay=1e-4, graph=graph)
        step.optimizer.capturable = True
        ptrs, losses = [], []
        for i in range(5):
            xi, yi = pkg.synthetic_batch(2, 64, seed=80 + i)
            losses.append(step(xi.to(DEV), yi.to(DEV)).detach().clone())
            ptrs.append([p.grad.data_ptr() for p in net.parameters()])
        torch.cuda.synchronize()
        if graph:
            assert step._graph is not None
        else:
            assert all(a == ptrs[0] for a in ptrs[1:]), "p.grad moved between eager steps"
        res[graph] = (losses, [p.detach().clone() for p in net.parameters()], [b.detach().clone() for b in net.buffers()])
        del step, net
    for a, b in zip(res[False][0], res[True][0]):
        assert torch.equal(a, b), (float(a), float(b))
    for a, b in zip(res[False][1] + res[False][2], res[True][1] + res[True][2]):
        assert torch.equal(a, b)
