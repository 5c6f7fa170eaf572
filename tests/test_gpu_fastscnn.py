"""GPU: the Fast-SCNN baseline (the reference's comne.py:305-476, BCELoss + Adam) on the HIP kernels.

  kernels   the depthwise 3x3 (stride 1 and 2: forward, weight and data gradient), the fused depthwise -> pointwise forward with its BatchNorm
            partials and the fused pointwise weight gradient together with their unfused partner, the pyramid pooling / resize kernels, the
            feature fusion with its backward, and the upsampling sigmoid head - each against float64 math written in the reference's order
            (F.conv2d with groups, F.adaptive_avg_pool2d, F.interpolate, F.batch_norm and their autograd)
  model     one train step against the reference goldens (tests/golden/fastscnn_*), the same under each RUNET_NO_FUSED_* switch, decision-aware
            gradient parity against the CPU restatement in float64 (tests/fastscnn_ref.py), sizes and bounds, determinism and graph capture,
            ModelEvaluator
The error measure is tests/test_gpu_hrnet.py's: max |got - want| / max |want|, band 1e-5 (fp32 kernels with fp32 statistics).  Two runs of
every kernel must give the same bits; kernels that write channel slices of wider buffers must leave the other channels bit-unchanged.
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

import decisions_fastscnn as DF
import fastscnn_ref as fref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PKG = "eusipco-2026-robust-unet_amd"
BAND = 1e-5
EPS = 1e-5


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


def _in_slice(t_nhwc, lo, wide):
    """-> (a channel-slice view holding t inside a wider random buffer, the buffer)"""
    n, h, w, c = t_nhwc.shape
    buf = torch.randn((n, h, w, wide), device=DEV)
    buf[..., lo:lo + c] = t_nhwc
    return buf[..., lo:lo + c], buf


def _bn_state(B, c, g, training=True):
    """a BatchNorm2d's handles on the device with random affine parameters (and, for eval mode, random running statistics)"""
    gamma, beta = 1 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    rm = torch.zeros(c) if training else 0.3 * torch.randn(c, generator=g)
    rv = torch.ones(c) if training else 0.5 + torch.rand(c, generator=g)
    cpu = (gamma, beta, rm, rv)
    return B.BNState(gamma.to(DEV), beta.to(DEV), rm.clone().to(DEV), rv.clone().to(DEV), torch.zeros((), dtype=torch.int64, device=DEV)), cpu


# ------------------------------------------------------------------------------------------------------------ depthwise 3x3
DW_SHAPES = [(1, 1, 1, 4, "plain"), (2, 1, 5, 4, "plain"), (2, 5, 1, 8, "plain"), (3, 5, 7, 12, "plain"), (1, 33, 65, 48, "plain"),
             (2, 16, 16, 32, "slices")]


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("n,h,w,c,kind", DW_SHAPES)
def test_depthwise_matches_float64(pkg, n, h, w, c, kind, stride):
    """runet_dw3_fwd / _wgrad / _dgrad against float64 F.conv2d(groups = c, padding 1) and its autograd; output size ceil(h / stride)"""
    B = _mod("blocks")
    g = torch.Generator().manual_seed(13 * n + 7 * h + 3 * w + c + 1000 * stride)
    x = torch.randn((n, c, h, w), generator=g)
    wt = torch.randn((c, 1, 3, 3), generator=g) / 3
    x64, w64 = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    y_ref = F.conv2d(x64, w64, None, stride, 1, 1, c)
    ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride
    assert y_ref.shape == (n, c, ho, wo)
    dy = torch.randn((n, c, ho, wo), generator=g)
    y_ref.backward(dy.double())
    wd = wt.permute(2, 3, 1, 0).contiguous().to(DEV)
    runs = []
    for _ in range(2):
        xd, dyd = _nhwc(x).to(DEV), _nhwc(dy).to(DEV)
        if kind == "slices":
            xd, _ = _in_slice(xd, 8, 48)
            dyd, _ = _in_slice(dyd, 4, 40)
            ybuf, dxbuf = torch.randn((n, ho, wo, 64), device=DEV), torch.randn((n, h, w, 64), device=DEV)
            keep_y, keep_dx = ybuf.clone(), dxbuf.clone()
            yd = B.dw3_forward(xd, wd, stride, out=ybuf[..., 32:])
            dxd = B.dw3_dgrad(dyd, wd, h, w, stride, out=dxbuf[..., 16:48])
        else:
            yd = B.dw3_forward(xd, wd, stride)
            dxd = B.dw3_dgrad(dyd, wd, h, w, stride)
        dw = B.dw3_wgrad(xd, dyd, stride)
        torch.cuda.synchronize()
        if kind == "slices":
            assert torch.equal(ybuf[..., :32], keep_y[..., :32])
            assert torch.equal(dxbuf[..., :16], keep_dx[..., :16]) and torch.equal(dxbuf[..., 48:], keep_dx[..., 48:])
        runs.append((yd.contiguous(), dw, dxd.contiguous()))
    for a, b in zip(*runs):
        assert _same(a, b)
    yd, dw, dxd = runs[0]
    assert tuple(dw.shape) == (3, 3, 1, c)
    errs = dict(y=_err(_nchw(yd), y_ref.detach()), dw=_err(dw.permute(3, 2, 0, 1), w64.grad), dx=_err(_nchw(dxd), x64.grad))
    print(f"\ndepthwise {n}x{h}x{w}x{c} stride {stride} ({kind}): " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= BAND, errs


# ------------------------------------------------------------------------------------------------------------ depthwise -> pointwise
MODEL_PAIRS = sorted({(cin, cout, s) for _, cin, cout, s in fref.SEP_HEAD + fref.SEP_TRUNK + fref.SEP_TAIL})
DWSEP_CASES = ([(2, 5, 7) + p for p in MODEL_PAIRS] + [(2, 1, 3, 64, 64, 1), (2, 3, 1, 64, 64, 1), (2, 1, 3, 64, 64, 2), (1, 33, 65, 96, 128, 1)])


@pytest.mark.parametrize("n,h,w,cin,cout,stride", DWSEP_CASES)
def test_dwsep_fused_and_partner_match_float64(pkg, n, h, w, cin, cout, stride):
    """runet_dwsep_fwd's t, the BatchNorm mean / invstd finalised from its partials, and runet_dwsep_wgrad_pw's dWp against float64
    F.conv2d(groups) -> F.conv2d(1x1); the unfused partner (runet_dw3_fwd + the shared 1x1 convolution and weight gradient) against the same
    reference; the two t within the band of each other (different summation orders, not bit-equal)."""
    B, ops = _mod("blocks"), _mod("ops")
    g = torch.Generator().manual_seed(cin * 131 + cout * 7 + stride + h * w)
    x = torch.randn((n, cin, h, w), generator=g)
    wdw = torch.randn((cin, 1, 3, 3), generator=g) / 3
    wpw = torch.randn((cout, cin, 1, 1), generator=g) / np.sqrt(cin)
    d64 = F.conv2d(x.double(), wdw.double(), None, stride, 1, 1, cin)
    t64 = F.conv2d(d64, wpw.double())
    ho, wo = t64.shape[2:]
    dt = torch.randn((n, cout, ho, wo), generator=g)
    dwp64 = torch.einsum("nihw,nohw->io", d64, dt.double())
    mean64 = t64.mean((0, 2, 3))
    invstd64 = 1.0 / torch.sqrt(t64.var((0, 2, 3), unbiased=False) + EPS)
    bn, _ = _bn_state(B, cout, g)
    p = B.DWSepParams(wdw.permute(2, 3, 1, 0).contiguous().to(DEV), wpw.permute(2, 3, 1, 0).contiguous().to(DEV), bn, stride)
    xd, dtd = _nhwc(x).to(DEV), _nhwc(dt).to(DEV)
    out = {}
    for fused in (True, False):
        runs = []
        for _ in range(2):
            sm = B.Small(torch.device(DEV))
            t, d, fs = B.dwsep_conv(xd, p, True, fused=fused)
            assert (d is None) == fused and (not fused or "part" in fs)
            _, _, mean, invstd, _ = B.bn_coeff(t, bn, True, sm, fused=fs)
            dwp = B.dwsep_wgrad_pw(xd, p.wd, dtd, stride) if fused else ops.conv_wgrad(d, dtd, 1, 1, on_side=False)
            torch.cuda.synchronize()
            runs.append((t, mean.clone(), invstd.clone(), dwp))
        for a, b in zip(*runs):
            assert _same(a, b)
        t, mean, invstd, dwp = runs[0]
        errs = dict(t=_err(_nchw(t), t64), mean=_err(mean, mean64), invstd=_err(invstd, invstd64), dwp=_err(dwp.view(cin, cout), dwp64))
        print(f"\ndwsep {n}x{h}x{w} {cin}->{cout} s{stride} ({'fused' if fused else 'partner'}): " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        assert max(errs.values()) <= BAND, (fused, errs)
        out[fused] = t
    assert _err(out[True], out[False]) <= BAND


def test_dwsep_layer_writes_a_concat_half(pkg):
    """block3's last layer: 128 -> 128 at 2 x 5 x 7 through blocks.dwsep_forward with out = channels [0, 128) of a 256-wide buffer, fused and
    unfused: the activation against float64 relu(batch_norm(...)), the other half bit-unchanged"""
    B = _mod("blocks")
    n, h, w, c = 2, 5, 7, 128
    g = torch.Generator().manual_seed(77)
    x = torch.randn((n, c, h, w), generator=g)
    wdw, wpw = torch.randn((c, 1, 3, 3), generator=g) / 3, torch.randn((c, c, 1, 1), generator=g) / np.sqrt(c)
    bn, (gamma, beta, _, _) = _bn_state(B, c, g)
    t64 = F.conv2d(F.conv2d(x.double(), wdw.double(), None, 1, 1, 1, c), wpw.double())
    a64 = F.relu(F.batch_norm(t64, None, None, gamma.double(), beta.double(), True, 0.1, EPS))
    p = B.DWSepParams(wdw.permute(2, 3, 1, 0).contiguous().to(DEV), wpw.permute(2, 3, 1, 0).contiguous().to(DEV), bn, 1)
    for fused in (True, False):
        cat = torch.randn((n, h, w, 2 * c), device=DEV)
        keep = cat.clone()
        a, cx = B.dwsep_forward(_nhwc(x).to(DEV), p, True, B.Small(torch.device(DEV)), out=cat[..., :c], fused=fused)
        torch.cuda.synchronize()
        assert a.data_ptr() == cat.data_ptr() and (cx["d"] is None) == fused
        assert _err(_nchw(cat[..., :c]), a64) <= BAND
        assert torch.equal(cat[..., c:], keep[..., c:])


# ------------------------------------------------------------------------------------------------------------ pyramid pooling
PYR_SIZES = [(1, 1), (2, 2), (2, 3), (3, 3), (5, 7), (7, 7), (8, 8), (13, 6)]
BINS = (1, 2, 3, 6)


def _branch_major(ts):
    """four [n, c, b, b] tensors -> the [50 n, c] branch-major layout"""
    return torch.cat([t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) for t in ts], 0)


def _from_branch_major(buf, n):
    out, r = [], 0
    for b in BINS:
        out.append(buf[r:r + n * b * b].view(n, b, b, -1).permute(0, 3, 1, 2))
        r += n * b * b
    return out


@pytest.mark.parametrize("c", [4, 128])
@pytest.mark.parametrize("h,w", PYR_SIZES)
def test_pyramid_pool_matches_adaptive_avg_pool(pkg, h, w, c):
    """runet_pyramid_pool_fwd against float64 F.adaptive_avg_pool2d for 1 / 2 / 3 / 6 bins (overlapping windows where h % b != 0, replicated
    pixels where h < b), x a channel slice; runet_pyramid_pool_bwd against its autograd plus the direct slice term, and without one"""
    lib, check, ops = _mod("_lib").lib, _mod("_lib").check, _mod("ops")
    n = 2
    g = torch.Generator().manual_seed(31 * h + w + c)
    x = torch.randn((n, c, h, w), generator=g)
    x64 = x.double().requires_grad_(True)
    pooled64 = [F.adaptive_avg_pool2d(x64, b) for b in BINS]
    dps = [torch.randn((n, c, b, b), generator=g) for b in BINS]
    direct = torch.randn((n, c, h, w), generator=g)
    torch.autograd.backward(pooled64, [d.double() for d in dps])
    st = ops.stream()
    runs = []
    for _ in range(2):
        xd, _ = _in_slice(_nhwc(x).to(DEV), c, 2 * c + 4)
        pooled = torch.empty((50 * n, c), device=DEV)
        check(lib.runet_pyramid_pool_fwd(xd.data_ptr(), ops.ld(xd), pooled.data_ptr(), c, n, h, w, c, st))
        dpd = _branch_major(dps).to(DEV)
        dird, _ = _in_slice(_nhwc(direct).to(DEV), 0, 2 * c)
        dxbuf = torch.randn((n, h, w, c + 8), device=DEV)
        keep = dxbuf.clone()
        dx = dxbuf[..., 4:4 + c]
        check(lib.runet_pyramid_pool_bwd(dpd.data_ptr(), c, dird.data_ptr(), ops.ld(dird), dx.data_ptr(), ops.ld(dx), n, h, w, c, st))
        dx0 = torch.empty((n, h, w, c), device=DEV)
        check(lib.runet_pyramid_pool_bwd(dpd.data_ptr(), c, None, 0, dx0.data_ptr(), c, n, h, w, c, st))
        torch.cuda.synchronize()
        assert torch.equal(dxbuf[..., :4], keep[..., :4]) and torch.equal(dxbuf[..., 4 + c:], keep[..., 4 + c:])
        runs.append((pooled, dx.contiguous(), dx0))
    for a, b in zip(*runs):
        assert _same(a, b)
    pooled, dx, dx0 = runs[0]
    errs = {f"pool{b}": _err(got, want.detach()) for b, got, want in zip(BINS, _from_branch_major(pooled, n), pooled64)}
    errs["dx"] = _err(_nchw(dx), x64.grad + direct.double())
    errs["dx_nodirect"] = _err(_nchw(dx0), x64.grad)
    print(f"\npyramid pool {h}x{w}x{c}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= BAND, errs


@pytest.mark.parametrize("cq", [4, 32])
@pytest.mark.parametrize("h,w", PYR_SIZES)
def test_pyramid_upsample_matches_interpolate(pkg, h, w, cq):
    """runet_pyramid_upsample_fwd / _bwd against float64 F.interpolate(size=(h, w), bilinear, align_corners=False) of the four [n, b, b, cq]
    pyramids and its autograd; the destination is channels [cq, 5 cq) of a wider buffer whose other channels stay bit-unchanged"""
    lib, check, ops = _mod("_lib").lib, _mod("_lib").check, _mod("ops")
    n = 2
    g = torch.Generator().manual_seed(17 * h + w + cq)
    acts = [torch.randn((n, cq, b, b), generator=g) for b in BINS]
    a64 = [a.double().requires_grad_(True) for a in acts]
    up64 = torch.cat([F.interpolate(a, size=(h, w), mode="bilinear", align_corners=False) for a in a64], 1)
    dy = torch.randn((n, 4 * cq, h, w), generator=g)
    up64.backward(dy.double())
    st = ops.stream()
    runs = []
    for _ in range(2):
        ad = _branch_major(acts).to(DEV)
        buf = torch.randn((n, h, w, 6 * cq), device=DEV)
        keep = buf.clone()
        y = buf[..., cq:5 * cq]
        check(lib.runet_pyramid_upsample_fwd(ad.data_ptr(), cq, y.data_ptr(), ops.ld(y), n, h, w, cq, st))
        dyd, _ = _in_slice(_nhwc(dy).to(DEV), 4 * cq, 8 * cq)
        da = torch.empty((50 * n, cq), device=DEV)
        check(lib.runet_pyramid_upsample_bwd(dyd.data_ptr(), ops.ld(dyd), da.data_ptr(), cq, n, h, w, cq, st))
        torch.cuda.synchronize()
        assert torch.equal(buf[..., :cq], keep[..., :cq]) and torch.equal(buf[..., 5 * cq:], keep[..., 5 * cq:])
        runs.append((y.contiguous(), da))
    for a, b in zip(*runs):
        assert _same(a, b)
    y, da = runs[0]
    errs = dict(y=_err(_nchw(y), up64.detach()))
    errs.update({f"da{b}": _err(got, want.grad) for b, got, want in zip(BINS, _from_branch_major(da, n), a64)})
    print(f"\npyramid upsample {h}x{w}x{cq}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= BAND, errs


# ------------------------------------------------------------------------------------------------------------ feature fusion
def _ffm_case(n, h, w, c, s, training, seed):
    """float64 reference of relu(bn(t_low) + interpolate(bn(t_high))) and its gradients; as test_gpu_mswnet._ms_case, redrawn on the reference
    only until no pre-ReLU value is within 1e-5 of zero (a mask there could differ between fp32 and float64), at most 64 draws"""
    for draw in range(64):
        g = torch.Generator().manual_seed(seed + 1000 * draw)
        tl, th = torch.randn((n, c, s * h, s * w), generator=g), torch.randn((n, c, h, w), generator=g)
        par = {k: (1 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g), 0.3 * torch.randn(c, generator=g),
                   0.5 + torch.rand(c, generator=g)) for k in ("low", "high")}
        dy = torch.randn((n, c, s * h, s * w), generator=g)
        tl64, th64 = tl.double().requires_grad_(True), th.double().requires_grad_(True)
        leaf = {k: tuple(v.double().requires_grad_(i < 2) for i, v in enumerate(par[k])) for k in par}

        def bn(t, k):
            ga, be, rm, rv = leaf[k]
            return F.batch_norm(t, rm.clone(), rv.clone(), ga, be, training, 0.1, EPS)
        hi = bn(th64, "high")
        hi.retain_grad()
        pre = bn(tl64, "low") + F.interpolate(hi, size=(s * h, s * w), mode="bilinear", align_corners=False)
        if float(pre.detach().abs().min()) > 1e-5:
            y = F.relu(pre)
            y.backward(dy.double())
            return dict(tl=tl, th=th, par=par, dy=dy, y=y.detach(), dtl=tl64.grad, dth=th64.grad, dhi=hi.grad, leaf=leaf, draws=draw + 1)
    raise AssertionError("no draw without a pre-ReLU value within 1e-5 of zero")


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("c", [4, 128])
@pytest.mark.parametrize("h,w,s", [(1, 1, 2), (2, 3, 2), (5, 7, 2), (2, 3, 4)])
def test_ffm_matches_float64(pkg, h, w, s, c, training):
    """runet_ffm_fwd (and its unfused partner) and blocks.ffm_backward (runet_relu_mask_nhwc, the shared BatchNorm backward, the gather with
    the BatchNorm sums) against float64 autograd, with batch and with running statistics; s = 2 is the model's factor.
    The 1 x 1 high map in training mode is the 1-bin situation: a BatchNorm over the batch's two values per channel, whose input gradient
    cancels analytically to (g1 - g2) / 2 * scale * eps / (var + eps) - five orders below the terms it is made of.  max |want| is then no
    scale for a rounding error, so that one comparison (dt_high there) is measured against the size of the cancelling terms,
    max |scale| * max |gradient of the BatchNorm's output|; every other figure keeps max |want|."""
    B = _mod("blocks")
    n = 2
    ref = _ffm_case(n, h, w, c, s, training, 97 * h + 11 * w + c + s)
    assert ref["draws"] <= 8, ref["draws"]
    dev = torch.device(DEV)
    tl, th, dy = (_nhwc(ref[k]).to(DEV) for k in ("tl", "th", "dy"))
    res = {}
    for fused in (True, False):
        runs = []
        for _ in range(2):
            sm = B.Small(dev)
            co = {}
            for k, t in (("low", tl), ("high", th)):
                ga, be, rm, rv = ref["par"][k]
                bn = B.BNState(ga.to(DEV), be.to(DEV), rm.clone().to(DEV), rv.clone().to(DEV), torch.zeros((), dtype=torch.int64, device=DEV))
                co[k] = B.bn_coeff(t, bn, training, sm)[:4]
            y = B.ffm_forward(tl, co["low"][:2], th, co["high"][:2], s, fused=fused)
            sl, shh = B.vec(2 * c, dev), B.vec(2 * c, dev)
            dtl, dth = B.ffm_backward(dy, y, tl, (co["low"][2], co["low"][3], co["low"][0]), th, (co["high"][2], co["high"][3], co["high"][0]), s,
                                      sl, shh, training=training)
            torch.cuda.synchronize()
            runs.append((y, dtl, dth, sl, shh))
        for a, b in zip(*runs):
            assert _same(a, b)
        y, dtl, dth, sl, shh = runs[0]
        errs = dict(y=_err(_nchw(y), ref["y"]), dt_low=_err(_nchw(dtl), ref["dtl"]), dt_high=_err(_nchw(dth), ref["dth"]))
        if training and n * h * w == 2:
            ga, _, _, _ = ref["par"]["high"]
            invstd = 1.0 / torch.sqrt(ref["th"].double().var((0, 2, 3), unbiased=False) + EPS)
            terms = float((ga.double() * invstd).abs().max()) * float(ref["dhi"].abs().max())
            errs["dt_high"] = float((_nchw(dth).double().cpu() - ref["dth"]).abs().max()) / terms
        for k, sums in (("low", sl), ("high", shh)):
            errs[f"dgamma_{k}"] = _err(sums[:c], ref["leaf"][k][0].grad)
            errs[f"dbeta_{k}"] = _err(sums[c:], ref["leaf"][k][1].grad)
        print(f"\nffm {h}x{w} x{s} c={c} {'train' if training else 'eval'} ({'fused' if fused else 'partner'}, {ref['draws']} draw(s)): "
              + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        assert max(errs.values()) <= BAND, (fused, errs)
        res[fused] = y
    assert _err(res[True], res[False]) <= BAND


# ------------------------------------------------------------------------------------------------------------ head
@pytest.mark.parametrize("n,h,w,s", [(2, 1, 1, 8), (3, 5, 7, 8), (1, 33, 17, 8), (3, 5, 7, 2), (1, 33, 17, 2)])
def test_up_sigmoid_matches_float64(pkg, n, h, w, s):
    """runet_up_sigmoid_fwd / _bwd against float64 sigmoid(F.interpolate(z, scale s)) and its autograd; s = 2 also against runet_up2_sigmoid_*"""
    B, ops = _mod("blocks"), _mod("ops")
    lib, check = _mod("_lib").lib, _mod("_lib").check
    g = torch.Generator().manual_seed(5 * n + 3 * h + w + s)
    z = 2 * torch.randn((n, 1, h, w), generator=g)
    dprob = torch.randn((n, 1, s * h, s * w), generator=g)
    z64 = z.double().requires_grad_(True)
    p64 = torch.sigmoid(F.interpolate(z64, size=(s * h, s * w), mode="bilinear", align_corners=False))
    p64.backward(dprob.double())
    zd, dpd = z.view(n, h, w).to(DEV), dprob.to(DEV)
    runs = []
    for _ in range(2):
        prob = B.up_sigmoid_forward(zd, s)
        dz = B.up_sigmoid_backward(dpd, prob, s)
        torch.cuda.synchronize()
        runs.append((prob, dz))
    for a, b in zip(*runs):
        assert _same(a, b)
    prob, dz = runs[0]
    assert prob.shape == (n, 1, s * h, s * w) and dz.shape == (n, h, w)
    errs = dict(prob=_err(prob, p64.detach()), dz=_err(dz.view(n, 1, h, w), z64.grad))
    if s == 2:
        st = ops.stream()
        p2, dz2 = torch.empty_like(prob), torch.empty_like(dz)
        check(lib.runet_up2_sigmoid_fwd(zd.data_ptr(), p2.data_ptr(), n, h, w, st))
        check(lib.runet_up2_sigmoid_bwd(dpd.data_ptr(), p2.data_ptr(), dz2.data_ptr(), n, h, w, st))
        torch.cuda.synchronize()
        errs.update(prob_vs_up2=_err(prob, p2), dz_vs_up2=_err(dz, dz2))
    print(f"\nup-sigmoid {n}x{h}x{w} x{s}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= BAND, errs


# ------------------------------------------------------------------------------------------------------------ model
def _net(pkg, st):
    net = pkg.FastSCNN()
    res = net.load_state_dict(st, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return net.to(DEV).train()


def _pick(gold, key, t):
    t = t.detach().cpu().double().reshape(-1)
    if key in gold:
        return t.float().numpy(), gold[key].reshape(-1)
    stride, numel, k = (int(v) for v in gold[key + "/meta"])
    assert t.numel() == numel
    return t[::stride][:k].float().numpy(), gold[key + "/sample"]


def _golden_step(pkg, tag):
    """one train step (BCELoss, FusedAdam 1e-4, weight decay 1e-4) and an eval forward on a fixture's inputs -> CPU tensors"""
    meta = json.load(open(os.path.join(GOLDEN, f"fastscnn_{tag}.json")))
    net = _net(pkg, fref.init_state(seed=meta["seed"], perturb_bn=True))
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
    """test_gpu_mswnet._check_golden_step's bands: probabilities, loss, gradient norms, sampled gradients, BatchNorm buffers, the Adam step
    and the eval forward; the analytically zero gradients (fastscnn_ref.ZERO_GRAD: the conv biases in front of a train-mode BatchNorm) within
    1e-4 of the largest gradient norm, absolute."""
    meta = json.load(open(os.path.join(GOLDEN, f"fastscnn_{tag}.json")))
    gold = load_npz(f"fastscnn_{tag}.npz")
    a, b = _pick(gold, "prob", res["prob"])
    assert np.abs(a - b).max() <= 1e-3, np.abs(a - b).max()
    assert abs(res["loss"] - float(gold["loss"])) <= 1e-4
    names = meta["param_names"]
    assert res["names"] == names
    gn = np.array([g.double().norm().item() for g in res["grads"]])
    ref = gold["grad_norm"]
    real = np.array([k not in fref.ZERO_GRAD for k in names])
    rel = np.abs(gn - ref) / (ref + 1e-3 * ref.max())
    print(f"\nFastSCNN {tag} ({what}): loss {res['loss']:.6f} (reference {float(gold['loss']):.6f}), worst gradient-norm error {rel[real].max():.1e}")
    assert rel[real].max() < 2e-2, (names[int(np.argmax(np.where(real, rel, 0)))], rel[real].max())
    gmax = max(float(np.abs(v).max()) for kk, v in gold.items() if kk.startswith("grad/") and not kk.endswith("/meta"))
    for k, g in zip(names, res["grads"]):
        a, b = _pick(gold, "grad/" + k, g)
        if k in fref.ZERO_GRAD:
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


@pytest.mark.parametrize("tag", TAGS)
def test_fastscnn_train_step_matches_reference(pkg, tag):
    """loss, probabilities, gradients, BatchNorm buffers, Adam deltas and the eval forward of both fixtures (H/16 map 4 x 4 and 6 x 6) at
    test_gpu_mswnet.py's golden-step tolerances (_check_golden_step), in the default configuration (the fused feature fusion; the separable
    layers on runet_dw3_fwd + the shared 1x1 convolution, the fused separable kernels being the opt-in)"""
    B = _mod("blocks")
    assert not B.FUSED_DWSEP and B.FUSED_FFM, "run the suite without RUNET_FUSED_DWSEP / RUNET_NO_FUSED_FFM"
    _check_golden_step(tag, _golden_step(pkg, tag), "default")


_AB_CODE = ("import importlib, sys, torch; sys.path[:0] = [%r, %r]; pkg = importlib.import_module(%r); import test_gpu_fastscnn as T\n"
            "B = importlib.import_module(%r)\n"
            "assert (B.FUSED_DWSEP, B.FUSED_FFM) == (sys.argv[2] == 'RUNET_FUSED_DWSEP', sys.argv[2] != 'RUNET_NO_FUSED_FFM')\n"
            "torch.save({tag: T._golden_step(pkg, tag) for tag in T.TAGS}, sys.argv[1])\n" % (ROOT, os.path.join(ROOT, "tests"), PKG, PKG + ".blocks"))


@pytest.mark.parametrize("switch", ["RUNET_FUSED_DWSEP", "RUNET_NO_FUSED_FFM"])
def test_fastscnn_switches_give_the_same_step(pkg, switch):
    """each switch - the opt-in fused separable kernels (RUNET_FUSED_DWSEP=1) and the unfused feature fusion (RUNET_NO_FUSED_FFM=1) -, selected
    in a fresh child process (read at import), gives the golden train step of both fixtures within the same tolerances as the default
    (_check_golden_step): compared with the reference, not with the default step bit for bit (the summation orders differ, which can move a
    ReLU mask at a near-tie)"""
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"fastscnn_ab_{switch}_{os.getpid()}.pt")
    r = subprocess.run([sys.executable, "-c", _AB_CODE, path, switch], env={**os.environ, switch: "1"}, timeout=600, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    other = torch.load(path)
    os.remove(path)
    for tag in TAGS:
        _check_golden_step(tag, other[tag], switch + "=1")


@pytest.mark.parametrize("n,size,seed", [(2, 64, 5), (3, 96, 6)])
@pytest.mark.parametrize("fused_dwsep", [False, True], ids=["default", "fused_dwsep"])
def test_fastscnn_gradients_under_the_hip_decisions(pkg, n, size, seed, fused_dwsep, monkeypatch):
    """tests/decisions_seq.py's two-part check against the restatement in float64: ReLU masks on which the HIP step and the restatement differ
    are near-ties (decisions.NEAR_TIE), and under the HIP step's own decisions the worst and the median gradient error per tensor scale are
    bounded by what fp32 itself allows: the restatement run in float32 under the same forced decisions gives (worst32, median32) against
    float64, and the HIP step must stay within max(5e-4, 3 x worst32) and max(3e-5, 3 x median32) - three times, because two fp32 evaluations
    with different summation orders differ from float64 independently (the two-value BatchNorm of the 1-bin pyramid branch conditions this
    model worse than the other baselines)."""
    import decisions_seq as DS
    B, fs = _mod("blocks"), _mod("fastscnn")
    monkeypatch.setattr(B, "FUSED_DWSEP", fused_dwsep)
    st = fref.init_state(seed=seed, perturb_bn=True)
    net = _net(pkg, st)
    x, y = pkg.synthetic_batch(n, size, seed=seed)
    got = {}
    real = fs.fastscnn_backward

    def spy(net_, C, dprob):
        got["dec"] = DF.hip_decisions(B, C, fref)
        return real(net_, C, dprob)
    monkeypatch.setattr(fs, "fastscnn_backward", spy)
    prob = net(x.to(DEV))
    pkg.bce_loss(prob, y.to(DEV)).backward()
    torch.cuda.synchronize()
    log, _, ref_prob, _ = fref.step(st, x, y)
    assert float((prob.detach().cpu().double() - ref_prob).abs().max()) <= 1e-3
    assert len(log) == len(got["dec"]) == len(fref.DECISION_SITES) == 19
    flips = DS.differing(got["dec"], log)
    DS.assert_near_ties(flips)
    _, gref, _, _ = fref.step(st, x, y, forced=got["dec"])
    _, g32, _, _ = fref.step(st, x, y, forced=got["dec"], dtype=torch.float32)
    skip = set(fref.ZERO_GRAD)
    rows = DS.grad_errors({k: p.grad.detach().cpu() for k, p in net.named_parameters()}, gref, skip)
    rows32 = DS.grad_errors({k: v.double() for k, v in g32.items()}, gref, skip)
    med, med32 = float(np.median([r[0] for r in rows])), float(np.median([r[0] for r in rows32]))
    print(f"\nFastSCNN {n} x {size}^2 ({'fused' if fused_dwsep else 'unfused'} separable layers): {len(flips)} near-tie decisions forced; HIP worst {rows[0][0]:.1e} ({rows[0][1]}) median {med:.1e}; "
          f"float32 restatement worst {rows32[0][0]:.1e} ({rows32[0][1]}) median {med32:.1e}")
    assert rows[0][0] <= max(5e-4, 3 * rows32[0][0]), (rows[:4], rows32[:4])
    assert med <= max(3e-5, 3 * med32), (med, med32)


def test_fastscnn_sizes_and_bounds(pkg):
    """2 x 3 x 64 x 96 (H/16 map 4 x 6) and 2 x 3 x 32 x 32 (2 x 2: every 3- and 6-bin window a replicated pixel) against the restatement, a
    non-contiguous input, eval mode with one image; what the model refuses"""
    st = fref.init_state(seed=9, perturb_bn=True)
    net = _net(pkg, st)
    x, _ = pkg.synthetic_batch(2, 96, seed=9)
    for xs in (x[:, :, :64, :].contiguous(), x[:, :, 8:40, 16:48].contiguous()):
        with torch.no_grad():
            got = net(xs.to(DEV)).cpu()
            want = fref.forward({k: v.clone() for k, v in st.items()}, xs, True)
        assert got.shape == (2, 1) + tuple(xs.shape[2:])
        assert float((got - want).abs().max()) <= 1e-3, (tuple(xs.shape), float((got - want).abs().max()))
    with torch.no_grad():
        view = x.to(DEV)[:, :, 8:40, 16:48]
        assert not view.is_contiguous()
        got = net(view).cpu()
        want = fref.forward({k: v.clone() for k, v in st.items()}, x[:, :, 8:40, 16:48], True)
    assert float((got - want).abs().max()) <= 1e-3
    xs, ys = pkg.synthetic_batch(2, 32, seed=10)
    loss = pkg.bce_loss(net(xs.to(DEV)), ys.to(DEV))
    loss.backward()
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        net(xs[:1].to(DEV))
    net.eval()
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        got = net(xs[:1].to(DEV)).cpu()
        want = fref.forward(sd, xs[:1], False)
    assert float((got - want).abs().max()) <= 1e-3
    net.train()
    with pytest.raises(ValueError):
        net(torch.zeros((2, 3, 48, 48), device=DEV))
    with pytest.raises(ValueError):
        net(torch.zeros((2, 3, 32, 16), device=DEV))
    with pytest.raises(ValueError):
        net(torch.zeros((2, 4, 32, 32), device=DEV))
    with pytest.raises(TypeError):
        net(torch.zeros((2, 3, 32, 32), device=DEV, dtype=torch.float16))
    with pytest.raises(ValueError):
        pkg.FastSCNN(n_classes=2)
    with pytest.raises(ValueError):
        net.set_precision("bf16")
    with pytest.raises(NotImplementedError):
        net.sync_bn_hook = object()


@pytest.mark.parametrize("fused_dwsep", [False, True], ids=["default", "fused_dwsep"])
def test_fastscnn_step_is_deterministic_and_captures(pkg, fused_dwsep, monkeypatch):
    """2 x 64^2: two steps from an identical state give identical bits; TrainStep(graph=True) replay == eager, bit for bit, with p.grad at
    fixed addresses - with the separable layers on either path."""
    trainer = _mod("trainer")
    monkeypatch.setattr(_mod("blocks"), "FUSED_DWSEP", fused_dwsep)
    st = fref.init_state(seed=3, perturb_bn=True)
    x, y = pkg.synthetic_batch(2, 64, seed=31)
    x, y = x.to(DEV), y.to(DEV)
    runs = []
    for _ in range(2):
        net = _net(pkg, st)
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
        net = _net(pkg, st)
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


def test_fastscnn_trains_under_model_evaluator(pkg):
    """ModelEvaluator.train_model / evaluate_model drive FastSCNN unchanged for 2 batches x 2 epochs at 64 x 64; the eval-mode forward of the
    trained weights equals the restatement on the same state."""
    net = _net(pkg, fref.init_state(seed=1))
    ev = pkg.ModelEvaluator(torch.device(DEV))
    x, y = pkg.synthetic_batch(4, 64, seed=2)
    data = [(x[:2], y[:2]), (x[2:], y[2:])]
    out = ev.train_model(net, data, data, epochs=2, lr=1e-3)
    assert len(out["history"]["train_loss"]) == 2 and all(np.isfinite(out["history"]["val_loss"]))
    res = ev.evaluate_model(net, data)
    assert res["total_samples"] == 4 and 0.0 <= res["mean_iou"] <= 1.0
    st = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        got = net(x.to(DEV)).cpu()
        want = fref.forward(st, x, training=False)
    assert float((got - want).abs().max()) <= 1e-3
