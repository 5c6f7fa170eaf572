"""GPU: the HRNet-Water baseline (the reference's Extended_Baseline_Comparison.py:554-616, BCELoss + Adam :780-837) on the HIP kernels.

  kernels   the fused head (BatchNorm + ReLU + 1x1 at half resolution, x2 + sigmoid) and the fused fusion branches (BatchNorm affine behind the
            interpolation) against float64 math written in the reference's order (BatchNorm, ReLU, upsample, then the 1x1), and the shared
            convolutions at the widths this model brings (48, 96, 144, 192)
  model     one train step against the reference goldens (tests/golden/hrnet_*), decision-aware gradient parity against the CPU restatement
            (tests/hrnet_ref.py), sizes and bounds, both A/B switches, and the 16 x 256^2 benchmark size (determinism, graph capture)
The error measure is tests/test_gpu_segformer.py's: max |got - want| / max |want|, band 1e-5.
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

import hrnet_ref as href

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


def _nhwc_view(t, pad):
    """t [n, h, w, c] -> the same values as a channel slice of a wider [n, h, w, c + pad] buffer (pixel stride c + pad)"""
    n, h, w, c = t.shape
    wide = torch.randn((n, h, w, c + pad), device=DEV)
    wide[..., :c] = t
    return wide[..., :c]


def _bn_state(B, gamma, beta):
    c = gamma.numel()
    return B.BNState(gamma.to(DEV), beta.to(DEV), torch.zeros(c, device=DEV), torch.ones(c, device=DEV), torch.zeros((), dtype=torch.int64, device=DEV))


# ------------------------------------------------------------------------------------------------------------ head kernels
def _head_case(n, h, w, c):
    """Inputs of a head case and its float64 evaluation in the reference's order.  A ReLU input that is zero to within fp32 rounding would
    make the mask, and with it dt, depend on the last bit of the BatchNorm statistics on either side; the draw is repeated (next seed) until
    the float64 evaluation has no BatchNorm output within 1e-5 of zero (outputs are O(1); fp32 statistics reproduce them to ~1e-6).  This
    looks at the float64 reference only."""
    for attempt in range(64):
        g = torch.Generator().manual_seed(1000 * attempt + 97 * h + 13 * w + c)
        t = torch.randn((n, h, w, c), generator=g) * 2 + 0.5
        gamma, beta = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
        w1, b1 = torch.randn(c, generator=g) / np.sqrt(c), torch.randn(1, generator=g) * 0.1
        dprob = torch.randn((n, 1, 2 * h, 2 * w), generator=g)
        t64 = t.double().permute(0, 3, 1, 2).requires_grad_(True)
        g64, be64, w64, b64 = (v.double().requires_grad_(True) for v in (gamma, beta, w1, b1))
        y = F.batch_norm(t64, None, None, g64, be64, True, 0.0, 1e-5)
        if float(y.detach().abs().min()) >= 1e-5:
            break
    else:
        raise AssertionError("no draw without a near-zero ReLU input")
    up = F.interpolate(F.relu(y), scale_factor=2, mode="bilinear", align_corners=False)
    prob = torch.sigmoid(F.conv2d(up, w64.view(1, c, 1, 1), b64))
    prob.backward(dprob.double())
    dl = (dprob.double() * prob.detach() * (1 - prob.detach()))
    ref = dict(prob=prob.detach(), dt=t64.grad, dgamma=g64.grad, dbeta=be64.grad, dw=w64.grad, db=b64.grad, db_scale=float(dl.abs().sum()))
    return t, gamma, beta, w1, b1, dprob, ref


@pytest.mark.parametrize("n,h,w,c,pad", [(2, 1, 3, 64, 0), (2, 3, 1, 64, 0), (3, 5, 7, 64, 16), (1, 33, 65, 64, 0), (2, 16, 16, 64, 80), (2, 3, 5, 8, 4)])
def test_hr_head_kernels_match_float64(pkg, n, h, w, c, pad):
    """prob, dt, dgamma, dbeta, dw within 1e-5 of each tensor's largest magnitude; db (a cancelling scalar sum) within 1e-5 of the float64
    sum of its absolute terms; t a channel slice of a wider buffer where pad > 0; two calls give identical bits.  One-pixel-wide maps
    (every pixel an edge clamp), odd non-square sizes, a size that is no multiple of any tile, a second channel count."""
    B = _mod("blocks")
    t, gamma, beta, w1, b1, dprob, ref = _head_case(n, h, w, c)
    td = _nhwc_view(t.to(DEV), pad) if pad else t.to(DEV)
    s, sh, mean, invstd, _ = B.bn_coeff(td, _bn_state(B, gamma, beta), True, B.Small(td.device))
    wd, bd, dpd = w1.to(DEV), b1.to(DEV), dprob.to(DEV)
    runs = []
    for _ in range(2):
        prob, saved = B.hr_head_forward(td, s, sh, wd, bd, fused=True)
        dt, out = B.hr_head_backward(dpd, prob, td, s, sh, wd, mean, invstd, saved=saved)
        runs.append((prob, dt, out))
    torch.cuda.synchronize()
    prob, dt, out = runs[0]
    assert saved is None and prob.shape == (n, 1, 2 * h, 2 * w)
    errs = dict(prob=_err(prob, ref["prob"]), dt=_err(dt.permute(0, 3, 1, 2), ref["dt"]), dgamma=_err(out[:c], ref["dgamma"]),
                dbeta=_err(out[c:2 * c], ref["dbeta"]), dw=_err(out[2 * c:3 * c], ref["dw"]),
                db=abs(float(out[3 * c]) - float(ref["db"])) / ref["db_scale"])
    print(f"\nhr head {n}x{h}x{w}x{c}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= BAND, errs
    assert all(_same(a, b) for a, b in zip(runs[0], runs[1]))


def test_hr_head_unfused_partner_matches_float64(pkg):
    """the A/B partner (bn_apply -> runet_bilinear_nhwc_fwd at 64 channels -> runet_outc_*) against the same reference, same band"""
    B = _mod("blocks")
    n, h, w, c = 3, 5, 7, 64
    t, gamma, beta, w1, b1, dprob, ref = _head_case(n, h, w, c)
    td = t.to(DEV)
    s, sh, mean, invstd, _ = B.bn_coeff(td, _bn_state(B, gamma, beta), True, B.Small(td.device))
    prob, saved = B.hr_head_forward(td, s, sh, w1.to(DEV), b1.to(DEV), fused=False)
    dt, out = B.hr_head_backward(dprob.to(DEV), prob, td, s, sh, w1.to(DEV), mean, invstd, saved=saved)
    torch.cuda.synchronize()
    errs = dict(prob=_err(prob, ref["prob"]), dt=_err(dt.permute(0, 3, 1, 2), ref["dt"]), dgamma=_err(out[:c], ref["dgamma"]),
                dbeta=_err(out[c:2 * c], ref["dbeta"]), dw=_err(out[2 * c:3 * c], ref["dw"]),
                db=abs(float(out[3 * c]) - float(ref["db"])) / ref["db_scale"])
    print(f"\nhr head unfused {n}x{h}x{w}x{c}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= BAND, errs


# ------------------------------------------------------------------------------------------------------------ fusion-branch kernels
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("s,n,h,w,c,lo", [(2, 2, 1, 3, 48, 48), (4, 2, 3, 1, 48, 96), (2, 3, 5, 7, 48, 96), (4, 3, 3, 5, 12, 48), (4, 2, 16, 16, 48, 96)])
def test_bn_bilinear_kernels_match_float64(pkg, s, n, h, w, c, lo, fused):
    """y = upsample_s(BatchNorm(x)) written into channels [lo, lo + c) of a 144-wide buffer (the other channels bit-unchanged), and dx, dgamma,
    dbeta from the matching slice of a 144-wide gradient, within 1e-5 of each tensor's largest magnitude; two calls give identical bits.
    fused=False: the A/B partner on the shared kernels, same band."""
    B = _mod("blocks")
    g = torch.Generator().manual_seed(s * 1000 + h * 37 + w * 5 + c)
    x = torch.randn((n, h, w, c), generator=g) * 2 + 0.5
    gamma, beta = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    wide = torch.randn((n, s * h, s * w, 144), generator=g).to(DEV)
    dwide = torch.randn((n, s * h, s * w, 144), generator=g)
    keep = wide.clone()
    xd, dwd = x.to(DEV), dwide.to(DEV)
    sc, sh, mean, invstd, _ = B.bn_coeff(xd, _bn_state(B, gamma, beta), True, B.Small(xd.device))
    runs = []
    for _ in range(2):
        B.bn_bilinear_forward(xd, sc, sh, wide[..., lo:lo + c], s, fused=fused)
        sums = torch.empty(2 * c, device=DEV)
        dx = B.bn_bilinear_backward(dwd[..., lo:lo + c], xd, mean, invstd, sc, sums, s, fused=fused)
        runs.append((wide[..., lo:lo + c].clone(), dx, sums))
    torch.cuda.synchronize()
    x64 = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y_ref = F.interpolate(F.batch_norm(x64, None, None, g64, b64, True, 0.0, 1e-5), scale_factor=s, mode="bilinear", align_corners=False)
    y_ref.backward(dwide[..., lo:lo + c].double().permute(0, 3, 1, 2))
    y, dx, sums = runs[0]
    errs = dict(y=_err(y.permute(0, 3, 1, 2), y_ref.detach()), dx=_err(dx.permute(0, 3, 1, 2), x64.grad), dgamma=_err(sums[:c], g64.grad),
                dbeta=_err(sums[c:], b64.grad))
    print(f"\nbn + x{s} ({'fused' if fused else 'unfused'}) {n}x{h}x{w}x{c}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= BAND, errs
    assert torch.equal(wide[..., :lo], keep[..., :lo]) and torch.equal(wide[..., lo + c:], keep[..., lo + c:])
    assert all(_same(a, b) for a, b in zip(runs[0], runs[1]))


# ------------------------------------------------------------------------------------------------------------ shared convolutions, new widths
@pytest.mark.parametrize("cin,cout,k,stride", [(64, 48, 3, 1), (48, 48, 3, 1), (144, 64, 3, 1), (3, 64, 3, 2), (64, 96, 3, 2), (96, 192, 3, 2),
                                               (96, 48, 1, 1), (192, 48, 1, 1), (96, 96, 3, 1), (192, 192, 3, 1)])
def test_shared_convolutions_at_the_new_widths(pkg, cin, cout, k, stride):
    """forward, data gradient (not for the RGB stem) and weight gradient at 2 x 16 x 16 through the entry points hrnet.py uses (ops.conv_* for
    stride 1, ops.conv_general_* for the stride-2 layers) against float64 F.conv2d, within 1e-5 of scale (the band of
    test_widened_general_conv_matches_float64).  The stride-1 data gradient is also taken with accumulate (the stem's second consumer)."""
    ops, B = _mod("ops"), _mod("blocks")
    n, size, pad = 2, 16, k // 2
    g = torch.Generator().manual_seed(cin * 7 + cout + k + stride)
    x = torch.randn((n, cin, size, size), generator=g)
    wt = torch.randn((cout, cin, k, k), generator=g) / np.sqrt(cin * k * k)
    b = torch.randn(cout, generator=g) * 0.1
    x64, w64 = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    y_ref = F.conv2d(x64, w64, b.double(), stride=stride, padding=pad)
    dy = torch.randn(y_ref.shape, generator=g)
    y_ref.backward(dy.double())
    xd = B.to_nhwc_pad(x.to(DEV), 4) if cin == 3 else x.to(DEV).permute(0, 2, 3, 1).contiguous()
    wd = wt.permute(2, 3, 1, 0).contiguous().to(DEV)
    dyd = dy.to(DEV).permute(0, 2, 3, 1).contiguous()
    errs = {}
    if stride == 1:
        stats = {}
        y = ops.conv_fwd(xd, wd, b.to(DEV), stats=stats)
        dw = ops.conv_wgrad(xd, dyd, k, k)
        dx = ops.conv_dgrad(dyd, wd)
        base = torch.randn(dx.shape, generator=g).to(DEV)
        acc = ops.conv_dgrad(dyd, wd, out=base.clone(), accumulate=True)
        errs["dx+"] = _err((acc - base).permute(0, 3, 1, 2), x64.grad)
        if "part" in stats:      # the epilogue's BatchNorm statistics partials against the tensor's own statistics
            st = B.BNState(torch.ones(cout, device=DEV), torch.zeros(cout, device=DEV), torch.zeros(cout, device=DEV), torch.ones(cout, device=DEV),
                           torch.zeros((), dtype=torch.int64, device=DEV))
            _, _, mean, invstd, _ = B.bn_coeff(y, st, True, B.Small(y.device), fused=stats)
            yr = y_ref.detach()
            errs["mean"] = float((mean.double().cpu() - yr.mean((0, 2, 3))).abs().max()) / float(yr.abs().max())
            errs["invstd"] = _err(invstd, (yr.var((0, 2, 3), unbiased=False) + 1e-5).rsqrt())
    else:
        y = ops.conv_general_fwd(xd, wd, b.to(DEV), stride, pad)
        dw = ops.conv_general_wgrad(xd, dyd, k, k, stride, pad, cin_w=cin)
        dx = ops.conv_general_dgrad(dyd, wd, size, size, stride, pad) if cin != 3 else None
    errs.update(y=_err(y.permute(0, 3, 1, 2), y_ref.detach()), dw=_err(dw.permute(3, 2, 0, 1), w64.grad))
    if dx is not None:
        errs["dx"] = _err(dx.permute(0, 3, 1, 2), x64.grad)
    torch.cuda.synchronize()
    print(f"\nconv {cin}->{cout} k{k} s{stride} at {size}^2: " + " ".join(f"{kk} {v:.1e}" for kk, v in errs.items()))
    assert max(errs.values()) <= BAND, errs


def test_branch_activation_and_gradient_use_concat_slices(pkg):
    """the layout hrnet.py relies on: hr_branch's last BatchNorm + ReLU written into channels [0, 48) of the 144-wide concat (bn_apply with
    out = a slice, the other channels bit-unchanged), and bn_backward reading the [0, 48) slice of a 144-wide gradient (the same bits as from
    a dense copy)."""
    ops, B = _mod("ops"), _mod("blocks")
    g = torch.Generator().manual_seed(11)
    n, size = 2, 16
    t = torch.randn((n, size, size, 48), generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(48, generator=g), 0.1 * torch.randn(48, generator=g)
    cat = torch.randn((n, size, size, 144), generator=g).to(DEV)
    keep = cat.clone()
    td = t.to(DEV)
    s, sh, mean, invstd, _ = B.bn_coeff(td, _bn_state(B, gamma, beta), True, B.Small(td.device))
    B.bn_apply(td, s, sh, None, relu=True, out=cat[..., :48])
    a_ref = F.relu(F.batch_norm(t.double().permute(0, 3, 1, 2), None, None, gamma.double(), beta.double(), True, 0.0, 1e-5))
    assert _err(cat[..., :48].permute(0, 3, 1, 2), a_ref) <= BAND
    assert torch.equal(cat[..., 48:], keep[..., 48:])
    dcat = torch.randn((n, size, size, 144), generator=g).to(DEV)
    sums = torch.empty(96, device=DEV)
    dt = B.bn_backward(dcat[..., :48], td, mean, invstd, s, sums, relu_shift=sh)
    dt2 = B.bn_backward(dcat[..., :48].contiguous(), td, mean, invstd, s, torch.empty(96, device=DEV), relu_shift=sh)
    assert _same(dt, dt2)


# ------------------------------------------------------------------------------------------------------------ model
def _net(pkg, st):
    net = pkg.HRNetWater()
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


@pytest.mark.parametrize("tag", ["n2_s64", "n2_s128"])
def test_hrnet_train_step_matches_reference(pkg, tag):
    """test_segformer_train_step_matches_reference's bands; the analytically zero gradients (hrnet_ref.ZERO_GRAD: the conv biases in front of
    a train-mode BatchNorm) within 1e-4 of the largest gradient norm, absolute."""
    meta = json.load(open(os.path.join(GOLDEN, f"hrnet_{tag}.json")))
    gold = load_npz(f"hrnet_{tag}.npz")
    st = href.init_state(seed=meta["seed"], perturb_bn=True)
    net = _net(pkg, st)
    x, y = pkg.synthetic_batch(meta["n"], meta["size"], seed=meta["seed"])
    opt = pkg.FusedAdam(net.parameters(), lr=1e-4, weight_decay=1e-4)
    opt.zero_grad()
    prob = net(x.to(DEV))
    loss = pkg.bce_loss(prob, y.to(DEV))
    loss.backward()
    a, b = _pick(gold, "prob", prob)
    assert np.abs(a - b).max() <= 1e-3, np.abs(a - b).max()
    assert abs(loss.item() - float(gold["loss"])) <= 1e-4
    names = meta["param_names"]
    assert [k for k, _ in net.named_parameters()] == names
    gn = np.array([p.grad.double().norm().item() for p in net.parameters()])
    ref = gold["grad_norm"]
    real = np.array([k not in href.ZERO_GRAD for k in names])
    rel = np.abs(gn - ref) / (ref + 1e-3 * ref.max())
    print(f"\nHRNetWater {tag}: loss {loss.item():.6f} (reference {float(gold['loss']):.6f}), worst gradient-norm error {rel[real].max():.1e}")
    assert rel[real].max() < 2e-2, (names[int(np.argmax(np.where(real, rel, 0)))], rel[real].max())
    gmax = max(float(np.abs(v).max()) for kk, v in gold.items() if kk.startswith("grad/") and not kk.endswith("/meta"))
    for k, p in net.named_parameters():
        a, b = _pick(gold, "grad/" + k, p.grad)
        if k in href.ZERO_GRAD:
            assert np.abs(a).max() <= 1e-4 * ref.max() and np.abs(b).max() <= 1e-4 * ref.max(), (k, np.abs(a).max())
            continue
        scale = max(float(np.abs(b).max()), 1e-3 * gmax)
        err = np.abs(a - b)
        assert err.max() <= 0.2 * scale and int((err > 3e-2 * scale).sum()) <= max(1, err.size // 100), (k, err.max(), scale)
        assert float(np.linalg.norm(a - b)) <= 1e-2 * scale * np.sqrt(err.size), (k, float(np.linalg.norm(a - b)), scale)
    for k, buf in net.named_buffers():
        if f"buf/{k}" in gold:
            np.testing.assert_allclose(buf.cpu().numpy(), gold[f"buf/{k}"], rtol=2e-3, atol=2e-3, err_msg=k)
    opt.step()
    for k, p in net.named_parameters():
        a, b = _pick(gold, "adam/" + k, p)
        assert np.abs(a - b).max() <= 2.1e-4, (k, np.abs(a - b).max())         # one Adam step moves each weight by at most lr
    net.eval()
    with torch.no_grad():
        pe = net(x.to(DEV))
    a, b = _pick(gold, "eval_prob", pe)
    assert np.abs(a - b).max() <= 2e-3, np.abs(a - b).max()


DECISION_KEYS = tuple(f"{name}.{i}" for name, _ in href.BRANCHES for i in (0, 3)) + ("head",)      # hrnet_ref.RELU_SITES' order


def _record_decisions(monkeypatch):
    """Wraps hrnet.hrnet_backward: the step's nine ReLU masks in the restatement's call order, from the saved BatchNorm inputs and
    coefficients with bn_apply's own arithmetic (the fused head kernels take the same decision from the same expression)"""
    B = _mod("blocks")
    hr = _mod("hrnet")
    got = {}
    real = hr.hrnet_backward

    def spy(net_, C, dprob):
        got["dec"] = [(B.bn_apply(C[k]["t"], C[k]["s"], C[k]["h"], None, relu=True) > 0).permute(0, 3, 1, 2).cpu() for k in DECISION_KEYS]
        return real(net_, C, dprob)

    monkeypatch.setattr(hr, "hrnet_backward", spy)
    return got


def _oracle(st, x, y, forced=None):
    import decisions_seq as DS
    names = href.param_names()
    P = {k: v.clone() for k, v in st.items()}
    for k in names:
        P[k].requires_grad_(True)
    out = {}

    def step(rec):
        out["p"] = href.forward(P, x, True)
        return (lambda q: out.setdefault("loss", href.bce_mean(q, y))), out["p"], None
    log, pr = DS.run_oracle(href, step, forced)
    return log, {k: P[k].grad for k in names}, pr


@pytest.mark.parametrize("n,size,seed", [(2, 64, 5), (2, 128, 6)])
def test_hrnet_gradients_under_the_hip_decisions(pkg, n, size, seed, monkeypatch):
    """tests/decisions_seq.py's two-part check: ReLU masks on which the HIP step and the restatement differ are near-ties, and under the HIP
    step's own masks every gradient (but the analytically zero ones) is within 5e-4 of its tensor's scale, median within 3e-5."""
    import decisions_seq as DS
    st = href.init_state(seed=seed, perturb_bn=True)
    net = _net(pkg, st)
    x, y = pkg.synthetic_batch(n, size, seed=seed)
    got = _record_decisions(monkeypatch)
    prob = net(x.to(DEV))
    pkg.bce_loss(prob, y.to(DEV)).backward()
    torch.cuda.synchronize()
    log, _, ref_prob = _oracle(st, x, y)
    assert float((prob.detach().cpu() - ref_prob).abs().max()) <= 1e-3
    assert len(log) == len(got["dec"]) == 9
    flips = DS.differing(got["dec"], log)
    DS.assert_near_ties(flips)
    _, gref, _ = _oracle(st, x, y, got["dec"])
    rows = DS.grad_errors({k: p.grad.detach().cpu() for k, p in net.named_parameters()}, gref, set(href.ZERO_GRAD))
    med = float(np.median([r[0] for r in rows]))
    print(f"\nHRNetWater {n} x {size}^2: {len(flips)} near-tie decisions forced; worst gradient errors / scale "
          f"{[(f'{e:.1e}', k) for e, k in rows[:4]]}, median {med:.1e}")
    assert rows[0][0] <= 5e-4, rows[:4]
    assert med <= 3e-5, med


def test_hrnet_non_square_forward_and_bounds(pkg):
    """2 x 3 x 40 x 72 (lr branch 5 x 9) and 2 x 3 x 16 x 16 (lr branch 2 x 2: the smallest size with more than two BatchNorm samples there)
    against the restatement; what the module refuses"""
    st = href.init_state(seed=9, perturb_bn=True)
    net = _net(pkg, st)
    x, _ = pkg.synthetic_batch(2, 72, seed=9)
    for xs in (x[:, :, :40, :].contiguous(), x[:, :, 8:24, 16:32].contiguous()):
        with torch.no_grad():
            got = net(xs.to(DEV)).cpu()
            want = href.forward({k: v.clone() for k, v in st.items()}, xs, True)
        assert got.shape == (2, 1) + tuple(xs.shape[2:])
        assert float((got - want).abs().max()) <= 1e-3, (tuple(xs.shape), float((got - want).abs().max()))
    xs, ys = pkg.synthetic_batch(2, 16, seed=10)
    loss = pkg.bce_loss(net(xs.to(DEV)), ys.to(DEV))
    loss.backward()
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    with pytest.raises(ValueError):
        net(torch.zeros((1, 3, 20, 28), device=DEV))
    with pytest.raises(ValueError):
        pkg.HRNetWater(n_classes=2)
    with pytest.raises(ValueError):
        net.set_precision("bf16")
    with pytest.raises(NotImplementedError):
        net.sync_bn_hook = object()


_AB_CODE = ("import importlib, sys, torch; sys.path[:0] = [%r, %r]; pkg = importlib.import_module(%r); import hrnet_ref as href\n"
            "net = pkg.HRNetWater(); net.load_state_dict(href.init_state(seed=4)); net = net.to('cuda:0').train()\n"
            "x, y = pkg.synthetic_batch(2, 64, seed=4); loss = pkg.bce_loss(net(x.to('cuda:0')), y.to('cuda:0')); loss.backward()\n"
            "torch.save([loss.detach().cpu()] + [p.grad.cpu() for p in net.parameters()], sys.argv[1])\n" % (ROOT, os.path.join(ROOT, "tests"), PKG))


@pytest.fixture(scope="module")
def fused_step(pkg):
    """loss and gradients of the 2 x 64^2 step on the fused default, in this process (the switches are read at import: both must be off here)"""
    B = _mod("blocks")
    assert B.FUSED_HR_HEAD and B.FUSED_BN_UPSAMPLE, "run the suite without RUNET_NO_FUSED_HR_HEAD / RUNET_NO_FUSED_BN_UPSAMPLE"
    net = _net(pkg, href.init_state(seed=4))
    x, y = pkg.synthetic_batch(2, 64, seed=4)
    loss = pkg.bce_loss(net(x.to(DEV)), y.to(DEV))
    loss.backward()
    return [loss.detach().cpu()] + [p.grad.cpu() for p in net.parameters()]


@pytest.mark.parametrize("env", ["RUNET_NO_FUSED_HR_HEAD", "RUNET_NO_FUSED_BN_UPSAMPLE"])
def test_hrnet_unfused_partners_give_the_same_step(pkg, fused_step, env):
    """Each A/B partner, selected in a fresh child process (the switches are read at import), gives the loss and every gradient of the fused
    default within the kernel band, 1e-5 of the tensor's largest magnitude; the analytically zero gradients (rounding noise on both sides)
    within 1e-5 of the largest gradient."""
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"hrnet_ab_{env}_{os.getpid()}.pt")
    r = subprocess.run([sys.executable, "-c", _AB_CODE, path], env=dict(os.environ, **{env: "1"}), timeout=600, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    other = torch.load(path)
    os.remove(path)
    names = ["loss"] + href.param_names()
    gmax = max(float(t.abs().max()) for t in fused_step[1:])
    rows = []
    for k, a, b in zip(names, other, fused_step):
        scale = gmax if k in href.ZERO_GRAD else float(b.abs().max())
        rows.append((float((a - b).abs().max()) / scale, k))
    rows.sort(reverse=True)
    print(f"\n{env}=1 against the fused default at 2 x 64^2: worst {[(f'{e:.1e}', k) for e, k in rows[:4]]}")
    assert rows[0][0] <= BAND, rows[:4]


def test_hrnet_benchmark_size_is_deterministic_and_captures(pkg):
    """16 x 256^2: finite loss; two steps from an identical state give identical bits; TrainStep(graph=True) replay == eager, bit for bit, with
    p.grad at fixed addresses."""
    trainer = _mod("trainer")
    st = href.init_state(seed=3, perturb_bn=True)
    x, y = pkg.synthetic_batch(16, 256, seed=31)
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
    del runs
    res = {}
    for graph in (False, True):
        net = _net(pkg, st)
        step = trainer.TrainStep(net, lr=1e-3, weight_decay=1e-4, graph=graph)
        step.optimizer.capturable = True
        ptrs, losses = [], []
        for i in range(5):
            xi, yi = pkg.synthetic_batch(16, 256, seed=80 + i)
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


def test_hrnet_trains_under_model_evaluator(pkg):
    """ModelEvaluator.train_model / evaluate_model drive HRNetWater unchanged for 2 epochs; the eval-mode forward of the trained weights
    equals the restatement on the same state."""
    net = _net(pkg, href.init_state(seed=1))
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
        want = href.forward(st, x, training=False)
    assert float((got - want).abs().max()) <= 1e-3
