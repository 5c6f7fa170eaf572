"""GPU: the MSWNet baseline (the reference's Extended_Baseline_Comparison.py:479-548, BCELoss + Adam :780-837) on the HIP kernels.

  kernels   the 3x3 stride-1 max-pool and its gather backward against torch's CPU pool (values and winners bit for bit, the gradient against
            float64 autograd); the fused multi-scale stem (statistics, forward, the two backward kernels, with the shared finalize) against
            float64 math written in the reference's order (four F.conv2d, F.max_pool2d, torch.cat, F.batch_norm, ReLU), its unfused A/B partner
            against the same reference; the shared convolutions at the widths this model brings (5x5 through the general kernel, 16- and
            32-channel output slices, the 1024-channel bridge at 1 x 1 and 2 x 2 pixels, the 1024 -> 512 transposed convolution)
  model     one train step against the reference goldens (tests/golden/mswnet_*), decision-aware gradient parity against the CPU restatement
            in float64 (tests/mswnet_ref.py), sizes and bounds, the A/B switch, determinism and graph capture, ModelEvaluator
The error measure is tests/test_gpu_hrnet.py's: max |got - want| / max |want|, band 1e-5 (fp32 kernels with fp32 statistics).
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

import decisions_mswnet as DM
import mswnet_ref as mref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PKG = "eusipco-2026-robust-unet_amd"
BAND = 1e-5


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


# ------------------------------------------------------------------------------------------------------------ 3x3 stride-1 max-pool
POOL_SHAPES = [(1, 1, 1, 4, "plain"), (2, 1, 5, 4, "plain"), (2, 5, 1, 8, "plain"), (3, 5, 7, 12, "plain"), (1, 33, 65, 4, "plain"),
               (2, 16, 16, 32, "slices")]


def _pool_inputs(n, h, w, c, ties):
    g = torch.Generator().manual_seed(11 * n + 7 * h + 3 * w + c + 1000 * int(ties))
    x = torch.randint(0, 3, (n, c, h, w), generator=g).float() if ties else torch.randn((n, c, h, w), generator=g)
    return x, torch.randn((n, c, h, w), generator=g), torch.randn((n, c, h, w), generator=g)


@pytest.mark.parametrize("ties", [False, True], ids=["continuous", "ties"])
@pytest.mark.parametrize("n,h,w,c,kind", POOL_SHAPES)
def test_maxpool3s1_matches_torch(pkg, n, h, w, c, kind, ties):
    """Forward values bit-equal to torch's CPU F.max_pool2d(x, 3, 1, 1), winner bytes equal to its return_indices as window positions (a
    continuous input and a tie-heavy one of integers 0..2: the first maximum in row-major order wins); the gather backward within 1e-5 of
    float64 autograd on the same input, accumulate=1 adding onto a non-zero dx; the idx=NULL forward; two runs give the same bits.  "slices":
    x, y, dy and dx are channel slices of wider buffers, whose other channels stay untouched."""
    B = _mod("blocks")
    x, dy, dx0 = _pool_inputs(n, h, w, c, ties)
    y_ref, flat = F.max_pool2d(x, 3, 1, 1, return_indices=True)
    code_ref = DM.pool_code_3s1(flat, w)
    x64 = x.double().requires_grad_(True)
    F.max_pool2d(x64, 3, 1, 1).backward(dy.double())

    def dev(t, lo, wide):
        t = _nhwc(t).to(DEV)
        if kind != "slices":
            return t, None
        buf = torch.randn((n, h, w, wide), device=DEV)
        buf[..., lo:lo + c] = t
        return buf[..., lo:lo + c], buf
    runs = []
    for _ in range(2):
        xd, _ = dev(x, 8, 48)
        dyd, _ = dev(dy, 4, 40)
        dxa, dxa_buf = dev(dx0, 16, 64)
        if kind == "slices":
            ybuf = torch.randn((n, h, w, 64), device=DEV)
            keep_y, keep_dx = ybuf.clone(), dxa_buf.clone()
            yd, idx = B.maxpool3s1_forward(xd, out=ybuf[..., 32:])
        else:
            yd, idx = B.maxpool3s1_forward(xd)
        y2, none = B.maxpool3s1_forward(xd, want_idx=False)
        dxd = B.maxpool3s1_backward(dyd, idx)
        B.maxpool3s1_backward(dyd, idx, dx=dxa)
        torch.cuda.synchronize()
        assert none is None and _same(y2, yd)
        if kind == "slices":
            assert torch.equal(ybuf[..., :32], keep_y[..., :32]) and torch.equal(dxa_buf[..., :16], keep_dx[..., :16])
            assert torch.equal(dxa_buf[..., 48:], keep_dx[..., 48:])
        runs.append((yd.contiguous(), idx, dxd, dxa.contiguous()))
    yd, idx, dxd, dxa = runs[0]
    assert _same(yd.permute(0, 3, 1, 2).cpu(), y_ref)
    assert torch.equal(idx.permute(0, 3, 1, 2).cpu().long(), code_ref)
    errs = dict(dx=_err(dxd.permute(0, 3, 1, 2), x64.grad), dx_acc=_err(dxa.permute(0, 3, 1, 2), dx0.double() + x64.grad))
    print(f"\nmaxpool3s1 {n}x{h}x{w}x{c} {kind} {'ties' if ties else 'continuous'}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= BAND, errs
    assert all(_same(a, b) for a, b in zip(runs[0], runs[1]))


def test_maxpool3s1_nan_reaches_exactly_its_covering_windows(pkg):
    """one NaN element at 3 x 5 x 7 x 12: the outputs of the windows that cover it are NaN and point at it, every other output is untouched
    (torch's CPU rule: a NaN wins over everything)"""
    B = _mod("blocks")
    n, h, w, c = 3, 5, 7, 12
    x, _, _ = _pool_inputs(n, h, w, c, False)
    x[1, 5, 2, 3] = float("nan")
    y_ref, flat = F.max_pool2d(x, 3, 1, 1, return_indices=True)
    yd, idx = B.maxpool3s1_forward(_nhwc(x).to(DEV))
    y = yd.permute(0, 3, 1, 2).cpu()
    want = torch.zeros((n, c, h, w), dtype=torch.bool)
    want[1, 5, 1:4, 2:5] = True
    assert torch.equal(torch.isnan(y), want) and torch.equal(torch.isnan(y_ref), want)
    assert _same(torch.nan_to_num(y, nan=7.0), torch.nan_to_num(y_ref, nan=7.0))
    assert torch.equal(idx.permute(0, 3, 1, 2).cpu().long(), DM.pool_code_3s1(flat, w))


# ------------------------------------------------------------------------------------------------------------ multi-scale stem kernels
KS = (1, 3, 5, 1)


def _ms_case(n, h, w, training=True):
    """Inputs of a stem case and its float64 evaluation in the reference's order: an image uniform in [0, 1], the four convolutions from
    torch's default initialisation (U(-1/sqrt(fan_in), +)), jittered BatchNorm affines (and running statistics for the eval case).  A ReLU
    input that is zero to within fp32 rounding would make the mask depend on the last bit of the statistics on either side, so - as
    test_gpu_waternet.py's _wi_case - the draw is repeated (next seed) until the float64 BatchNorm output has no value within 1e-5 of zero.
    This looks at the float64 reference only."""
    for attempt in range(64):
        g = torch.Generator().manual_seed(1000 * attempt + 97 * h + 13 * w + n + 3 * int(training))
        x = torch.rand((n, 3, h, w), generator=g)
        u = lambda shape, fan: (torch.rand(shape, generator=g) * 2 - 1) / np.sqrt(fan)      # noqa: E731
        ws = [u((16, 3, k, k), 3 * k * k) for k in KS]
        bs = [u((16,), 3 * k * k) for k in KS]
        gamma, beta = 1 + 0.1 * torch.randn(64, generator=g), 0.1 * torch.randn(64, generator=g)
        rm, rv = 0.2 * torch.randn(64, generator=g), 0.05 + 0.2 * torch.rand(64, generator=g)
        de = torch.randn((n, h, w, 64), generator=g)
        P = [v.double().requires_grad_(True) for v in ws + bs + [gamma, beta]]
        x64 = x.double()
        t = torch.cat([F.conv2d(F.max_pool2d(x64, 3, 1, 1) if b == 3 else x64, P[b], P[4 + b], padding=KS[b] // 2) for b in range(4)], 1)
        t.retain_grad()
        y = F.batch_norm(t, None if training else rm.double(), None if training else rv.double(), P[8], P[9], training, 0.0, 1e-5)
        if float(y.detach().abs().min()) >= 1e-5:
            break
    else:
        raise AssertionError("no draw without a near-zero ReLU input")
    e = F.relu(y)
    e.backward(de.double().permute(0, 3, 1, 2))
    ref = dict(e=e.detach(), dgamma=P[8].grad, dbeta=P[9].grad, dt=t.grad, t=t.detach(), attempt=attempt)
    return dict(x=x, ws=ws, bs=bs, gamma=gamma, beta=beta, rm=rm, rv=rv, de=de), ref


def _ms_params(B, c):
    bn = [B.BNState(c["gamma"][16 * b:16 * b + 16].clone().to(DEV), c["beta"][16 * b:16 * b + 16].clone().to(DEV),
                    c["rm"][16 * b:16 * b + 16].clone().to(DEV), c["rv"][16 * b:16 * b + 16].clone().to(DEV),
                    torch.zeros((), dtype=torch.int64, device=DEV)) for b in range(4)]
    return B.MSBlockParams([v.permute(2, 3, 1, 0).contiguous().to(DEV) for v in c["ws"]], [v.to(DEV) for v in c["bs"]], bn)


def _ms_run(B, c, xd, training, fused, e_out=None, de=None):
    G = {}
    e, ctx = B.ms_stem_forward(xd, _ms_params(B, c), training, B.Small(xd.device), out=e_out, fused=fused)
    dt = B.ms_stem_backward(ctx, c["de"].to(DEV) if de is None else de, G, pre="enc1.", want_dt=True)
    torch.cuda.synchronize()
    assert ctx["fused"] == fused
    dgamma = torch.cat([G[f"enc1.branch{b + 1}.{2 if b == 3 else 1}.weight"] for b in range(4)])
    dbeta = torch.cat([G[f"enc1.branch{b + 1}.{2 if b == 3 else 1}.bias"] for b in range(4)])
    return e, dgamma, dbeta, dt, ctx, G


def _ms_errors(e, dgamma, dbeta, dt, ref):
    return dict(e=_err(e.permute(0, 3, 1, 2), ref["e"]), dgamma=_err(dgamma, ref["dgamma"]), dbeta=_err(dbeta, ref["dbeta"]),
                dt=_err(dt.permute(0, 3, 1, 2), ref["dt"]))


MS_SHAPES = [(2, 1, 3, "plain"), (2, 3, 1, "plain"), (3, 5, 7, "plain"), (1, 19, 35, "plain"), (2, 16, 16, "plain"), (1, 33, 65, "plain"),
             (2, 16, 16, "views")]


@pytest.mark.parametrize("n,h,w,kind", MS_SHAPES)
def test_ms_stem_kernels_match_float64(pkg, n, h, w, kind):
    """e, dgamma, dbeta and dt within 1e-5 of each tensor's largest magnitude; two calls give identical bits.  One-pixel-wide images, odd
    sizes, sizes that are no multiple of the 8 x 32 tile (more than one block: 15 at 33 x 65), "views": a non-contiguous NCHW input view, e
    and de as halves of 128-channel buffers."""
    B = _mod("blocks")
    c, ref = _ms_case(n, h, w)
    xd = c["x"].to(DEV)
    e_out = de = None
    if kind == "views":
        wide = torch.randn((n, 4, h + 3, w + 5), device=DEV)
        wide[:, 1:, 2:2 + h, 1:1 + w] = xd
        xd = wide[:, 1:, 2:2 + h, 1:1 + w]
        assert not xd.is_contiguous()
        ebuf, dbuf = torch.randn((n, h, w, 128), device=DEV), torch.randn((n, h, w, 128), device=DEV)
        keep = ebuf.clone()
        dbuf[..., 64:] = c["de"].to(DEV)
        e_out, de = ebuf[..., 64:], dbuf[..., 64:]
    runs = [_ms_run(B, c, xd, True, True, e_out, de)[:4] for _ in range(2)]
    errs = _ms_errors(*runs[0], ref)
    print(f"\nms stem {n}x{h}x{w} {kind} (draw {ref['attempt']}): " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= BAND, errs
    assert all(_same(a, b) for a, b in zip(runs[0], runs[1]))
    if kind == "views":
        assert torch.equal(ebuf[..., :64], keep[..., :64])


def test_ms_stem_kernels_eval_mode(pkg):
    """running statistics (runet_bn_finalize's eval route, no statistics launch): the same quantities at 3 x 5 x 7; the running buffers and
    the batch counters are left alone"""
    B = _mod("blocks")
    c, ref = _ms_case(3, 5, 7, training=False)
    e, dgamma, dbeta, dt, ctx, _ = _ms_run(B, c, c["x"].to(DEV), False, True)
    errs = _ms_errors(e, dgamma, dbeta, dt, ref)
    print("\nms stem eval 3x5x7: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= BAND, errs
    for b, bn in enumerate(ctx["p"].bn):
        assert torch.equal(bn.running_mean.cpu(), c["rm"][16 * b:16 * b + 16]) and torch.equal(bn.running_var.cpu(), c["rv"][16 * b:16 * b + 16])
        assert int(bn.nbt) == 0


def test_ms_stem_training_updates_the_running_buffers(pkg):
    """the shared finalize behind the statistics kernel, once per branch: running mean / unbiased running variance (momentum 0.1) and the batch
    counter of each of the four BatchNorms"""
    B = _mod("blocks")
    c, ref = _ms_case(1, 33, 65)
    p = _ms_params(B, c)
    B.ms_stem_forward(c["x"].to(DEV), p, True, B.Small(torch.device(DEV)), fused=True)
    t = ref["t"]
    for b, bn in enumerate(p.bn):
        sl = slice(16 * b, 16 * b + 16)
        assert _err(bn.running_mean, 0.9 * c["rm"][sl].double() + 0.1 * t[:, sl].mean((0, 2, 3))) <= BAND
        assert _err(bn.running_var, 0.9 * c["rv"][sl].double() + 0.1 * t[:, sl].var((0, 2, 3), unbiased=True)) <= BAND
        assert int(bn.nbt) == 1


def test_ms_stem_weight_gradients_and_unfused_partner_match_float64(pkg):
    """the A/B partner of enc1 (runet_to_nhwc_pad, the shared convolutions into 16-channel slices, runet_maxpool3s1_fwd, bn_apply / bn_backward
    over the concat) against the same reference, same band, at 3 x 5 x 7 - and, for both front ends, the four convolutions' weight gradients
    taken from dt's channel slices within the band.  dw4 (branch4's 1x1 on the 3x3 max-pool of the image) is measured against the float64
    sum of its absolute terms, as db1 is in the WaterNet test, for a reason of conditioning: the maximum of up to nine values uniform in
    [0, 1] is nearly constant (mean 0.87, standard deviation 0.10 at this shape), and the train-mode BatchNorm backward makes dt sum to
    zero over the pixels of each channel, so dw4 = sum pool(x) * dt keeps only the small varying part of pool(x): in float64 max |dw4| is
    22.8 here while the sums of the absolute terms are 335 to 1979, so a rounding error of the terms shows up to 87 x larger against
    max |dw4| (measured: 9.5e-6 unfused, 1.3e-5 fused; dw1..3, on the image itself, meet the plain band at 1e-6)."""
    B = _mod("blocks")
    c, ref = _ms_case(3, 5, 7)
    P = [v.double().requires_grad_(True) for v in c["ws"]]
    x64 = c["x"].double()
    t = torch.cat([F.conv2d(F.max_pool2d(x64, 3, 1, 1) if b == 3 else x64, P[b], c["bs"][b].double(), padding=KS[b] // 2) for b in range(4)], 1)
    t.backward(ref["dt"])
    dw4_abs = torch.einsum("nihw,nohw->oi", F.max_pool2d(x64, 3, 1, 1).abs(), ref["dt"][:, 48:].abs())
    for fused in (False, True):
        e, dgamma, dbeta, dt, _, G = _ms_run(B, c, c["x"].to(DEV), True, fused)
        errs = _ms_errors(e, dgamma, dbeta, dt, ref)
        for b in range(3):
            errs[f"dw{b + 1}"] = _err(G[f"enc1.branch{b + 1}.0.weight"].permute(3, 2, 0, 1), P[b].grad)
        dw4 = G["enc1.branch4.1.weight"].permute(3, 2, 0, 1).double().cpu()
        errs["dw4"] = float(((dw4 - P[3].grad).abs()[:, :, 0, 0] / dw4_abs).max())
        print(f"\nms stem {'fused' if fused else 'unfused'} 3x5x7: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        assert max(errs.values()) <= BAND, errs


# ------------------------------------------------------------------------------------------------------------ shared convolutions, new widths
def _conv_case(cin, cout, k, n, h, w, cin_w=None, seed=0):
    cin_w = cin if cin_w is None else cin_w
    g = torch.Generator().manual_seed(seed + 7 * cin + cout + k)
    x = torch.randn((n, cin_w, h, w), generator=g)
    wt = torch.randn((cout, cin_w, k, k), generator=g) / np.sqrt(cin_w * k * k)
    b = torch.randn(cout, generator=g) * 0.1
    x64, w64 = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    y_ref = F.conv2d(x64, w64, b.double(), padding=k // 2)
    dy = torch.randn(y_ref.shape, generator=g)
    y_ref.backward(dy.double())
    dx0 = torch.randn((n, h, w, cin), generator=g)
    xd = torch.zeros((n, h, w, cin))                       # channels past cin_w: the image's zero padding
    xd[..., :cin_w] = _nhwc(x)
    return dict(x=xd.to(DEV), w=wt.permute(2, 3, 1, 0).contiguous().to(DEV), b=b.to(DEV), dy=dy, dx0=dx0, y_ref=y_ref.detach(), dx_ref=x64.grad,
                dw_ref=w64.grad, cin_w=cin_w)


def _slice_of(t_nchw, lo, wide):
    """an NCHW CPU tensor as channels [lo, lo + c) of a `wide`-channel NHWC device buffer -> (view, buffer, copy of the buffer)"""
    n, c, h, w = t_nchw.shape
    buf = torch.randn((n, h, w, wide), device=DEV)
    buf[..., lo:lo + c] = _nhwc(t_nchw).to(DEV)
    return buf[..., lo:lo + c], buf, buf.clone()


def _others_unchanged(buf, keep, lo, c):
    return torch.equal(buf[..., :lo], keep[..., :lo]) and torch.equal(buf[..., lo + c:], keep[..., lo + c:])


@pytest.mark.parametrize("cin,cout,cin_w", [(64, 32, None), (128, 64, None), (256, 128, None), (4, 16, 3)])
def test_conv5x5_at_the_block_widths(pkg, cin, cout, cin_w):
    """Conv2d 5x5 s1 p2 through the general kernel at 2 x 6 x 10 pixels, written into channels [2 cout, 3 cout) of a 4 cout wide buffer (the
    other channels bit-unchanged); its data gradient read from the same slice and accumulated onto a non-zero buffer, its weight gradient -
    against float64 F.conv2d within 1e-5.  (4 with 3 weight rows, 16): the first level's unfused partner; its data gradient (which the model
    never takes: the input is the image) runs with the weight zero-padded to 4 rows."""
    ops = _mod("ops")
    n, h, w = 2, 6, 10
    c = _conv_case(cin, cout, 5, n, h, w, cin_w)
    ybuf = torch.randn((n, h, w, 4 * cout), device=DEV)
    keep = ybuf.clone()
    ops.conv_general_fwd(c["x"], c["w"], c["b"], 1, 2, out=ybuf[..., 2 * cout:3 * cout])
    dyv, _, _ = _slice_of(c["dy"], 2 * cout, 4 * cout)
    dw = ops.conv_general_wgrad(c["x"], dyv, 5, 5, 1, 2, cin_w=c["cin_w"])
    wd = c["w"]
    if c["cin_w"] != cin:
        wd = torch.zeros((5, 5, cin, cout), device=DEV)
        wd[:, :, :c["cin_w"]] = c["w"]
    dx = c["dx0"].to(DEV)
    ops.conv_general_dgrad(dyv, wd, h, w, 1, 2, out=dx, accumulate=True)
    torch.cuda.synchronize()
    k = c["cin_w"]
    errs = dict(y=_err(ybuf[..., 2 * cout:3 * cout].permute(0, 3, 1, 2), c["y_ref"]), dw=_err(dw.permute(3, 2, 0, 1), c["dw_ref"]),
                dx=_err(dx[..., :k].permute(0, 3, 1, 2), c["dx0"][..., :k].permute(0, 3, 1, 2).double() + c["dx_ref"]))
    print(f"\nconv 5x5 {cin}({k})->{cout} at 6x10: " + " ".join(f"{kk} {v:.1e}" for kk, v in errs.items()))
    assert max(errs.values()) <= BAND, errs
    assert _others_unchanged(ybuf, keep, 2 * cout, cout)
    if k != cin:
        assert torch.equal(dx[..., k:].cpu(), c["dx0"][..., k:])


@pytest.mark.parametrize("k", [1, 3])
def test_conv_into_32_channel_slices(pkg, k):
    """64 -> 32, 1x1 and 3x3, at 2 x 8 x 8 through the calls blocks.ms_block_forward / _backward make: forward (with the statistics dict) into
    channels [32, 64) of a 128-channel buffer, the data gradient from a 32-channel slice (accumulated onto a non-zero buffer) and the weight
    gradient - against float64 within 1e-5; the BatchNorm statistics of the slice (epilogue partials or the separate pass) give its mean."""
    ops, B = _mod("ops"), _mod("blocks")
    n, h, w, cin, cout = 2, 8, 8, 64, 32
    c = _conv_case(cin, cout, k, n, h, w, seed=5)
    ybuf = torch.randn((n, h, w, 128), device=DEV)
    keep = ybuf.clone()
    sl = ybuf[..., 32:64]
    fs = {}
    ops.conv_fwd(c["x"], c["w"], c["b"], out=sl, stats=fs)
    bn = B.BNState(torch.ones(cout, device=DEV), torch.zeros(cout, device=DEV), torch.zeros(cout, device=DEV), torch.ones(cout, device=DEV),
                   torch.zeros((), dtype=torch.int64, device=DEV))
    vec = [torch.empty(128, device=DEV) for _ in range(4)]
    B._bn_coeff_into(sl, bn, True, fs, *(v[32:64] for v in vec))
    dyv, _, _ = _slice_of(c["dy"], 32, 128)
    dw = ops.conv_wgrad(c["x"], dyv, k, k, cin_w=cin)
    dx = c["dx0"].to(DEV)
    ops.conv_dgrad(dyv, c["w"], out=dx, accumulate=True)
    torch.cuda.synchronize()
    errs = dict(y=_err(sl.permute(0, 3, 1, 2), c["y_ref"]), dw=_err(dw.permute(3, 2, 0, 1), c["dw_ref"]),
                dx=_err(dx.permute(0, 3, 1, 2), c["dx0"].permute(0, 3, 1, 2).double() + c["dx_ref"]),
                mean=_err(vec[2][32:64], c["y_ref"].mean((0, 2, 3))), invstd=_err(vec[3][32:64], (c["y_ref"].var((0, 2, 3), unbiased=False) + 1e-5).rsqrt()))
    print(f"\nconv {k}x{k} 64->32 slice at 8^2: " + " ".join(f"{kk} {v:.1e}" for kk, v in errs.items()))
    assert max(errs.values()) <= BAND, errs
    assert _others_unchanged(ybuf, keep, 32, 32) and int(bn.nbt) == 1


@pytest.mark.parametrize("cin,cout,size", [(512, 1024, 1), (1024, 1024, 1), (512, 1024, 2), (1024, 1024, 2)])
def test_bridge_convolutions_at_tiny_images(pkg, cin, cout, size):
    """the bridge's 3x3 convolutions on 2 x 1 x 1 and 2 x 2 x 2 pixels (a 16 x 16 and a 32 x 32 input): forward with the statistics dict, data
    and weight gradients through the calls mswnet.py makes, against float64 within 1e-5"""
    ops = _mod("ops")
    c = _conv_case(cin, cout, 3, 2, size, size, seed=9)
    y = ops.conv_fwd(c["x"], c["w"], c["b"], stats={})
    dyd = _nhwc(c["dy"]).to(DEV)
    dx = ops.conv_dgrad(dyd, c["w"])
    dw = ops.conv_wgrad(c["x"], dyd, 3, 3)
    torch.cuda.synchronize()
    errs = dict(y=_err(y.permute(0, 3, 1, 2), c["y_ref"]), dw=_err(dw.permute(3, 2, 0, 1), c["dw_ref"]), dx=_err(dx.permute(0, 3, 1, 2), c["dx_ref"]))
    print(f"\nconv 3x3 {cin}->{cout} at {size}^2: " + " ".join(f"{kk} {v:.1e}" for kk, v in errs.items()))
    assert max(errs.values()) <= BAND, errs


def test_transposed_convolution_1024_to_512_writes_a_concat_half(pkg):
    """ConvTranspose2d(k2, s2) 1024 -> 512, 2 x 2 x 2 -> 4 x 4, written into channels [0, 512) of a 1024-wide buffer (the other half
    bit-unchanged), with its data and weight gradients read from the same half of a gradient buffer - against float64 within 1e-5"""
    ops = _mod("ops")
    cin, cout, n, size = 1024, 512, 2, 2
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.randn((n, cin, size, size), generator=g)
    wt = torch.randn((cin, cout, 2, 2), generator=g) / np.sqrt(cin)
    b = torch.randn(cout, generator=g) * 0.1
    x64, w64 = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    y_ref = F.conv_transpose2d(x64, w64, b.double(), stride=2)
    dcat = torch.randn((n, 2 * size, 2 * size, 2 * cout), generator=g)
    y_ref.backward(dcat[..., :cout].double().permute(0, 3, 1, 2))
    xd = _nhwc(x).to(DEV)
    wd = wt.permute(2, 3, 0, 1).contiguous().to(DEV)
    cat = torch.randn((n, 2 * size, 2 * size, 2 * cout), generator=g).to(DEV)
    keep = cat.clone()
    dcd = dcat.to(DEV)
    ops.convt_fwd(xd, wd, b.to(DEV), out=cat[..., :cout])
    dw = ops.convt_wgrad(xd, dcd[..., :cout])
    dx = ops.convt_dgrad(dcd[..., :cout], wd)
    torch.cuda.synchronize()
    errs = dict(y=_err(cat[..., :cout].permute(0, 3, 1, 2), y_ref.detach()), dw=_err(dw.permute(2, 3, 0, 1), w64.grad), dx=_err(dx.permute(0, 3, 1, 2), x64.grad))
    print("\nconvt 1024->512 at 2^2: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= BAND, errs
    assert torch.equal(cat[..., cout:], keep[..., cout:])


# ------------------------------------------------------------------------------------------------------------ model
def _net(pkg, st):
    net = pkg.MSWNet()
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
    meta = json.load(open(os.path.join(GOLDEN, f"mswnet_{tag}.json")))
    net = _net(pkg, mref.init_state(seed=meta["seed"], perturb_bn=True))
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
    """test_gpu_waternet._check_golden_step's bands: probabilities, loss, gradient norms, sampled gradients, BatchNorm buffers, the Adam step
    and the eval forward; the analytically zero gradients (mswnet_ref.ZERO_GRAD: the conv biases in front of a train-mode BatchNorm) within
    1e-4 of the largest gradient norm, absolute."""
    meta = json.load(open(os.path.join(GOLDEN, f"mswnet_{tag}.json")))
    gold = load_npz(f"mswnet_{tag}.npz")
    a, b = _pick(gold, "prob", res["prob"])
    assert np.abs(a - b).max() <= 1e-3, np.abs(a - b).max()
    assert abs(res["loss"] - float(gold["loss"])) <= 1e-4
    names = meta["param_names"]
    assert res["names"] == names
    gn = np.array([g.double().norm().item() for g in res["grads"]])
    ref = gold["grad_norm"]
    real = np.array([k not in mref.ZERO_GRAD for k in names])
    rel = np.abs(gn - ref) / (ref + 1e-3 * ref.max())
    print(f"\nMSWNet {tag} ({what}): loss {res['loss']:.6f} (reference {float(gold['loss']):.6f}), worst gradient-norm error {rel[real].max():.1e}")
    assert rel[real].max() < 2e-2, (names[int(np.argmax(np.where(real, rel, 0)))], rel[real].max())
    gmax = max(float(np.abs(v).max()) for kk, v in gold.items() if kk.startswith("grad/") and not kk.endswith("/meta"))
    for k, g in zip(names, res["grads"]):
        a, b = _pick(gold, "grad/" + k, g)
        if k in mref.ZERO_GRAD:
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


@pytest.mark.parametrize("tag", ["n2_s32", "n2_s64"])
def test_mswnet_train_step_matches_reference(pkg, tag):
    """loss, probabilities, gradients, BatchNorm buffers, Adam deltas and the eval forward of both fixtures (bridge 2 x 2 and 4 x 4) at
    test_gpu_waternet.py's golden-step tolerances (_check_golden_step)"""
    B = _mod("blocks")
    assert B.FUSED_MS_STEM, "run the suite without RUNET_NO_FUSED_MS_STEM"
    _check_golden_step(tag, _golden_step(pkg, tag), "fused")


@pytest.mark.parametrize("n,size,seed", [(2, 32, 5), (2, 64, 6)])
def test_mswnet_gradients_under_the_hip_decisions(pkg, n, size, seed, monkeypatch):
    """tests/decisions_seq.py's two-part check against the restatement in float64: ReLU masks, 2x2 and 3x3 pool winners on which the HIP step
    and the restatement differ are near-ties (decisions.NEAR_TIE), and under the HIP step's own decisions every gradient (but the analytically
    zero ones) is within 5e-4 of its tensor's scale, median within 3e-5 (test_gpu_waternet.py's bounds)."""
    import decisions_seq as DS
    B, mw = _mod("blocks"), _mod("mswnet")
    st = mref.init_state(seed=seed, perturb_bn=True)
    net = _net(pkg, st)
    x, y = pkg.synthetic_batch(n, size, seed=seed)
    got = {}
    real = mw.mswnet_backward

    def spy(net_, C, dprob):
        got["dec"] = DM.hip_decisions(B, C, mref)
        return real(net_, C, dprob)
    monkeypatch.setattr(mw, "mswnet_backward", spy)
    prob = net(x.to(DEV))
    pkg.bce_loss(prob, y.to(DEV)).backward()
    torch.cuda.synchronize()
    log, _, ref_prob, _ = mref.step(st, x, y)
    assert float((prob.detach().cpu().double() - ref_prob).abs().max()) <= 1e-3
    assert len(log) == len(got["dec"]) == len(mref.DECISION_SITES) == 29
    flips = DS.differing(got["dec"], log)
    DS.assert_near_ties(flips)
    _, gref, _, _ = mref.step(st, x, y, forced=got["dec"])
    rows = DS.grad_errors({k: p.grad.detach().cpu() for k, p in net.named_parameters()}, gref, set(mref.ZERO_GRAD))
    med = float(np.median([r[0] for r in rows]))
    print(f"\nMSWNet {n} x {size}^2: {len(flips)} near-tie decisions forced; worst gradient errors / scale "
          f"{[(f'{e:.1e}', k) for e, k in rows[:4]]}, median {med:.1e}")
    assert rows[0][0] <= 5e-4, rows[:4]
    assert med <= 3e-5, med


def test_mswnet_non_square_forward_and_bounds(pkg):
    """2 x 3 x 32 x 48 (bridge 2 x 3) and 2 x 3 x 16 x 16 (bridge 1 x 1) against the restatement, the stand-alone MultiScaleBlock (forward
    only), a non-contiguous input; what the modules refuse"""
    st = mref.init_state(seed=9, perturb_bn=True)
    net = _net(pkg, st)
    x, _ = pkg.synthetic_batch(2, 48, seed=9)
    for xs in (x[:, :, :32, :].contiguous(), x[:, :, 8:24, 16:32].contiguous()):
        with torch.no_grad():
            got = net(xs.to(DEV)).cpu()
            want = mref.forward({k: v.clone() for k, v in st.items()}, xs, True)
        assert got.shape == (2, 1) + tuple(xs.shape[2:])
        assert float((got - want).abs().max()) <= 1e-3, (tuple(xs.shape), float((got - want).abs().max()))
    with torch.no_grad():
        view = x.to(DEV)[:, :, 8:24, 16:32]
        assert not view.is_contiguous()
        e1 = net.enc1(view).cpu()
        P = {k: v.clone() for k, v in st.items()}
        want1 = mref.multi_scale_block(P, "enc1", x[:, :, 8:24, 16:32], True, on_image=True)
        e2 = net.enc2(e1.to(DEV)).cpu()
        want2 = mref.multi_scale_block(P, "enc2", want1, True)
    assert e1.shape == (2, 64, 16, 16) and _err(e1, want1) <= 1e-4 and e2.shape == (2, 128, 16, 16) and _err(e2, want2) <= 1e-4
    with pytest.raises(NotImplementedError):
        net.enc1(x.to(DEV)[:, :, :16, :16])          # gradients enabled: the block on its own has no backward
    xs, ys = pkg.synthetic_batch(2, 16, seed=10)
    loss = pkg.bce_loss(net(xs.to(DEV)), ys.to(DEV))
    loss.backward()
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    with pytest.raises(ValueError):
        net(torch.zeros((1, 3, 40, 40), device=DEV))
    with pytest.raises(ValueError):
        net(torch.zeros((1, 3, 24, 32), device=DEV))
    with pytest.raises(ValueError):
        net(torch.zeros((1, 4, 16, 16), device=DEV))
    with pytest.raises(TypeError):
        net(torch.zeros((1, 3, 16, 16), device=DEV, dtype=torch.float16))
    with pytest.raises(ValueError):
        pkg.MSWNet(n_classes=2)
    with pytest.raises(ValueError):
        net.set_precision("bf16")
    with pytest.raises(NotImplementedError):
        net.sync_bn_hook = object()


_AB_CODE = ("import importlib, sys, torch; sys.path[:0] = [%r, %r]; pkg = importlib.import_module(%r); import test_gpu_mswnet as T\n"
            "assert not importlib.import_module(%r).FUSED_MS_STEM\n"
            "torch.save({tag: T._golden_step(pkg, tag) for tag in ('n2_s32', 'n2_s64')}, sys.argv[1])\n" % (ROOT, os.path.join(ROOT, "tests"), PKG, PKG + ".blocks"))


def test_mswnet_unfused_partner_gives_the_same_step(pkg):
    """RUNET_NO_FUSED_MS_STEM=1, selected in a fresh child process (the switch is read at import), gives the golden train step of both
    fixtures within the same tolerances as the fused default (_check_golden_step).  The two front ends differ in the last bits of enc1's
    activation, which can move a pool winner or a ReLU mask at a near-tie downstream: the steps are compared with the reference at the
    golden-step tolerances, not with each other bit for bit."""
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"mswnet_ab_{os.getpid()}.pt")
    r = subprocess.run([sys.executable, "-c", _AB_CODE, path], env=dict(os.environ, RUNET_NO_FUSED_MS_STEM="1"), timeout=600, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    other = torch.load(path)
    os.remove(path)
    for tag in ("n2_s32", "n2_s64"):
        _check_golden_step(tag, other[tag], "RUNET_NO_FUSED_MS_STEM=1")


def test_mswnet_step_is_deterministic_and_captures(pkg):
    """2 x 32^2: two steps from an identical state give identical bits; TrainStep(graph=True) replay == eager, bit for bit, with p.grad at
    fixed addresses."""
    trainer = _mod("trainer")
    st = mref.init_state(seed=3, perturb_bn=True)
    x, y = pkg.synthetic_batch(2, 32, seed=31)
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
            xi, yi = pkg.synthetic_batch(2, 32, seed=80 + i)
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


def test_mswnet_trains_under_model_evaluator(pkg):
    """ModelEvaluator.train_model / evaluate_model drive MSWNet unchanged for 2 batches x 2 epochs at 32 x 32; the eval-mode forward of the
    trained weights equals the restatement on the same state."""
    net = _net(pkg, mref.init_state(seed=1))
    ev = pkg.ModelEvaluator(torch.device(DEV))
    x, y = pkg.synthetic_batch(4, 32, seed=2)
    data = [(x[:2], y[:2]), (x[2:], y[2:])]
    out = ev.train_model(net, data, data, epochs=2, lr=1e-3)
    assert len(out["history"]["train_loss"]) == 2 and all(np.isfinite(out["history"]["val_loss"]))
    res = ev.evaluate_model(net, data)
    assert res["total_samples"] == 4 and 0.0 <= res["mean_iou"] <= 1.0
    st = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        got = net(x.to(DEV)).cpu()
        want = mref.forward(st, x, training=False)
    assert float((got - want).abs().max()) <= 1e-3
