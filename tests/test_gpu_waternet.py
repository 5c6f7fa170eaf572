"""GPU: the WaterNet baseline (the reference's Extended_Baseline_Comparison.py:378-473, BCELoss + Adam :780-837) on the HIP kernels.

  kernels   the fused water-index front end (statistics, forward, the two backward kernels, with the shared finalize) against float64 math
            written in the reference's order (Conv2d 1x1, F.batch_norm, ReLU, Conv2d 1x1, sigmoid, cat), its unfused A/B partner against the
            same reference, and the shared convolutions at the widths this model brings (8-channel input with 7 weight rows; the three k2
            transposed convolutions writing a concat half)
  model     one train step against the reference goldens (tests/golden/waternet_*), decision-aware gradient parity against the CPU restatement
            in float64 (tests/waternet_ref.py), sizes and bounds, the A/B switch, determinism and graph capture, ModelEvaluator
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

import waternet_ref as wref

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


# ------------------------------------------------------------------------------------------------------------ front-end kernels
def _wi_case(n, h, w, training=True, gray=False):
    """Inputs of a front-end case and its float64 evaluation in the reference's order: an image uniform in [0, 1], the two 1x1 convolutions from
    torch's default initialisation (U(-1/sqrt(fan_in), +)), a jittered BatchNorm affine (and running statistics for the eval case).  A ReLU
    input that is zero to within fp32 rounding would make the mask depend on the last bit of the statistics on either side, so - as
    test_gpu_hrnet.py's _head_case - the draw is repeated (next seed) until the float64 BatchNorm output has no value within 1e-5 of zero.
    This looks at the float64 reference only.  At these sizes (at most 1 x 33 x 65 x 16 = 34 320 outputs of density <= 0.4 near zero) the
    expected number of such values per draw is below 0.3 (counted on the CPU over the seven shapes: 0 to 1 redraws each)."""
    for attempt in range(64):
        g = torch.Generator().manual_seed(1000 * attempt + 97 * h + 13 * w + n + 7 * int(gray) + 3 * int(training))
        x = torch.rand((n, 1 if gray else 3, h, w), generator=g)
        if gray:
            x = x.expand(n, 3, h, w).contiguous()
        u = lambda shape, fan: (torch.rand(shape, generator=g) * 2 - 1) / np.sqrt(fan)      # noqa: E731
        w1, b1, w2, b2 = u((16, 3, 1, 1), 3), u((16,), 3), u((4, 16, 1, 1), 16), u((4,), 16)
        gamma, beta = 1 + 0.1 * torch.randn(16, generator=g), 0.1 * torch.randn(16, generator=g)
        rm, rv = 0.2 * torch.randn(16, generator=g), 0.05 + 0.2 * torch.rand(16, generator=g)
        gs = torch.randn((n, h, w, 4), generator=g)
        P = [v.double().requires_grad_(True) for v in (w1, b1, gamma, beta, w2, b2)]
        x64 = x.double()
        z = F.conv2d(x64, P[0], P[1])
        z.retain_grad()
        y = F.batch_norm(z, None, None, P[2], P[3], True, 0.0, 1e-5) if training else F.batch_norm(z, rm.double(), rv.double(), P[2], P[3], False, 0.0, 1e-5)
        if float(y.detach().abs().min()) >= 1e-5:
            break
    else:
        raise AssertionError("no draw without a near-zero ReLU input")
    s = torch.sigmoid(F.conv2d(F.relu(y), P[4], P[5]))
    s.backward(gs.double().permute(0, 3, 1, 2))
    ref = dict(buf=torch.cat([x64, s.detach(), torch.zeros((n, 1, h, w), dtype=torch.float64)], 1), dw1=P[0].grad.view(16, 3).t(), db1=P[1].grad,
               dgamma=P[2].grad, dbeta=P[3].grad, dw2=P[4].grad.view(4, 16).t(), db2=P[5].grad, db1_scale=z.grad.abs().sum((0, 2, 3)), attempt=attempt)
    return dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, gamma=gamma, beta=beta, rm=rm, rv=rv, g=gs), ref


def _params(B, c):
    bn = B.BNState(c["gamma"].to(DEV), c["beta"].to(DEV), c["rm"].to(DEV), c["rv"].to(DEV), torch.zeros((), dtype=torch.int64, device=DEV))
    return B.WaterIndexParams(c["w1"].permute(2, 3, 1, 0).contiguous().to(DEV), c["b1"].to(DEV), bn, c["w2"].permute(2, 3, 1, 0).contiguous().to(DEV),
                              c["b2"].to(DEV))


def _wi_errors(buf, red, app, ref):
    errs = dict(buf=_err(buf.permute(0, 3, 1, 2), ref["buf"]), dgamma=_err(red[:16], ref["dgamma"]), dbeta=_err(red[16:32], ref["dbeta"]),
                dw2=_err(red[32:96].view(16, 4), ref["dw2"]), db2=_err(red[96:], ref["db2"]), dw1=_err(app[:48].view(3, 16), ref["dw1"]))
    # db1 cancels to zero in training mode: measured against the float64 sum of its absolute terms
    errs["db1"] = float(((app[48:].double().cpu() - ref["db1"]).abs() / ref["db1_scale"]).max())
    return errs


WI_SHAPES = [(2, 1, 3, "plain"), (2, 3, 1, "plain"), (3, 5, 7, "plain"), (1, 33, 65, "plain"), (2, 16, 16, "plain"), (2, 8, 8, "views"), (2, 16, 16, "gray")]


@pytest.mark.parametrize("n,h,w,kind", WI_SHAPES)
def test_water_index_kernels_match_float64(pkg, n, h, w, kind):
    """The 8-channel buffer, dgamma, dbeta, dW1, dW2, db2 within 1e-5 of each tensor's largest magnitude, db1 within 1e-5 of the float64 sum of
    its absolute terms; two calls give identical bits.  One-pixel-wide images, an odd size, a size that is no multiple of any block or vector
    width (more than one block: 2145 pixels), "views": a non-contiguous NCHW input view and g a channel slice of a wider gradient buffer,
    "gray": R = G = B (the 3x3 input covariance has rank 1; there z is a linear function of one variable, so dW1 = sum x dz is made of the two
    sums BatchNorm's backward cancels and only its eps / (var + eps) part survives: the 1e-5 band on that residual has little margin)."""
    B = _mod("blocks")
    c, ref = _wi_case(n, h, w, gray=kind == "gray")
    xd, gd = c["x"].to(DEV), c["g"].to(DEV)
    if kind == "views":
        wide = torch.randn((n, 4, h + 3, w + 5), device=DEV)
        wide[:, 1:, 2:2 + h, 1:1 + w] = xd
        xd = wide[:, 1:, 2:2 + h, 1:1 + w]
        gw = torch.randn((n, h, w, 8), device=DEV)
        gw[..., 3:7] = gd
        gd = gw[..., 3:7]
        assert not xd.is_contiguous()
    runs = []
    for _ in range(2):
        buf, ctx = B.water_index_forward(xd, _params(B, c), True, B.Small(xd.device), fused=True)
        red, app = B.water_index_backward(ctx, gd)
        runs.append((buf, red, app))
    torch.cuda.synchronize()
    assert ctx["fused"] and buf.shape == (n, h, w, 8)
    errs = _wi_errors(*runs[0], ref)
    print(f"\nwater index {n}x{h}x{w} {kind} (draw {ref['attempt']}): " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= BAND, errs
    assert all(_same(a, b) for a, b in zip(runs[0], runs[1]))


def test_water_index_kernels_eval_mode(pkg):
    """running statistics (runet_bn_finalize's eval route, no statistics launch): the same quantities at 3 x 5 x 7; the running buffers and
    the batch counter are left alone"""
    B = _mod("blocks")
    n, h, w = 3, 5, 7
    c, ref = _wi_case(n, h, w, training=False)
    p = _params(B, c)
    buf, ctx = B.water_index_forward(c["x"].to(DEV), p, False, B.Small(torch.device(DEV)), fused=True)
    red, app = B.water_index_backward(ctx, c["g"].to(DEV))
    torch.cuda.synchronize()
    errs = _wi_errors(buf, red, app, ref)
    print(f"\nwater index eval {n}x{h}x{w}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= BAND, errs
    assert torch.equal(p.bn.running_mean.cpu(), c["rm"]) and torch.equal(p.bn.running_var.cpu(), c["rv"]) and int(p.bn.nbt) == 0


def test_water_index_training_updates_the_running_buffers(pkg):
    """the shared finalize behind the statistics kernel: running mean / unbiased running variance (momentum 0.1) and the batch counter"""
    B = _mod("blocks")
    c, _ = _wi_case(1, 33, 65)
    p = _params(B, c)
    B.water_index_forward(c["x"].to(DEV), p, True, B.Small(torch.device(DEV)), fused=True)
    z = F.conv2d(c["x"].double(), c["w1"].double(), c["b1"].double())
    assert _err(p.bn.running_mean, 0.9 * c["rm"].double() + 0.1 * z.mean((0, 2, 3))) <= BAND
    assert _err(p.bn.running_var, 0.9 * c["rv"].double() + 0.1 * z.var((0, 2, 3), unbiased=True)) <= BAND
    assert int(p.bn.nbt) == 1


def test_water_index_unfused_partner_matches_float64(pkg):
    """the A/B partner (runet_to_nhwc_pad, 1x1 convolutions, bn_coeff / bn_apply / bn_backward, the sigmoid and slice-copy kernels, conv_wgrad,
    chan_sum) against the same reference, same band, at 3 x 5 x 7"""
    B = _mod("blocks")
    n, h, w = 3, 5, 7
    c, ref = _wi_case(n, h, w)
    buf, ctx = B.water_index_forward(c["x"].to(DEV), _params(B, c), True, B.Small(torch.device(DEV)), fused=False)
    red, app = B.water_index_backward(ctx, c["g"].to(DEV))
    torch.cuda.synchronize()
    assert not ctx["fused"]
    errs = _wi_errors(buf, red, app, ref)
    print(f"\nwater index unfused {n}x{h}x{w}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= BAND, errs


# ------------------------------------------------------------------------------------------------------------ shared convolutions, new widths
def test_enc1_convolution_on_the_8_channel_buffer(pkg):
    """3x3, 8 channels in the buffer / 7 rows in the weight -> 64 at 2 x 16 x 16 through the calls waternet.py makes: forward (the padding
    channel holds junk here: it must not be read), the weight gradient with cin_w = 7, and the data gradient of channels 3..6 from the weight's
    rows 3..6 - against float64 F.conv2d within 1e-5 of scale"""
    ops = _mod("ops")
    g = torch.Generator().manual_seed(78)
    n, size = 2, 16
    x = torch.randn((n, 7, size, size), generator=g)
    wt = torch.randn((64, 7, 3, 3), generator=g) / np.sqrt(63)
    b = torch.randn(64, generator=g) * 0.1
    x64, w64 = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    y_ref = F.conv2d(x64, w64, b.double(), padding=1)
    dy = torch.randn(y_ref.shape, generator=g)
    y_ref.backward(dy.double())
    xd = torch.randn((n, size, size, 8), generator=g).to(DEV)
    xd[..., :7] = x.permute(0, 2, 3, 1).to(DEV)
    wd = wt.permute(2, 3, 1, 0).contiguous().to(DEV)
    dyd = dy.to(DEV).permute(0, 2, 3, 1).contiguous()
    y = ops.conv_fwd(xd, wd, b.to(DEV), stats={})
    dw = ops.conv_wgrad(xd, dyd, 3, 3, cin_w=7)
    dx = ops.conv_dgrad(dyd, wd[:, :, 3:7, :].contiguous())
    torch.cuda.synchronize()
    assert dw.shape == (3, 3, 7, 64) and dx.shape == (n, size, size, 4)
    errs = dict(y=_err(y.permute(0, 3, 1, 2), y_ref.detach()), dw=_err(dw.permute(3, 2, 0, 1), w64.grad), dx=_err(dx.permute(0, 3, 1, 2), x64.grad[:, 3:7]))
    print("\nconv 8(7)->64 k3 at 16^2: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= BAND, errs


@pytest.mark.parametrize("cin,cout", [(512, 256), (256, 128), (128, 64)])
def test_transposed_convolutions_write_a_concat_half(pkg, cin, cout):
    """ConvTranspose2d(k2, s2) at the three decoder widths, 2 x 4 x 4 -> 8 x 8, written into channels [0, cout) of a 2 cout wide buffer (the
    other half bit-unchanged), with its data and weight gradients read from the same half of a gradient buffer - against float64 within 1e-5"""
    ops = _mod("ops")
    g = torch.Generator().manual_seed(cin + cout)
    n, size = 2, 4
    x = torch.randn((n, cin, size, size), generator=g)
    wt = torch.randn((cin, cout, 2, 2), generator=g) / np.sqrt(cin)
    b = torch.randn(cout, generator=g) * 0.1
    x64, w64 = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    y_ref = F.conv_transpose2d(x64, w64, b.double(), stride=2)
    dcat = torch.randn((n, 2 * size, 2 * size, 2 * cout), generator=g)
    y_ref.backward(dcat[..., :cout].double().permute(0, 3, 1, 2))
    xd = x.to(DEV).permute(0, 2, 3, 1).contiguous()
    wd = wt.permute(2, 3, 0, 1).contiguous().to(DEV)
    cat = torch.randn((n, 2 * size, 2 * size, 2 * cout), generator=g).to(DEV)
    keep = cat.clone()
    dcd = dcat.to(DEV)
    ops.convt_fwd(xd, wd, b.to(DEV), out=cat[..., :cout])
    dw = ops.convt_wgrad(xd, dcd[..., :cout])
    dx = ops.convt_dgrad(dcd[..., :cout], wd)
    torch.cuda.synchronize()
    errs = dict(y=_err(cat[..., :cout].permute(0, 3, 1, 2), y_ref.detach()), dw=_err(dw.permute(2, 3, 0, 1), w64.grad), dx=_err(dx.permute(0, 3, 1, 2), x64.grad))
    print(f"\nconvt {cin}->{cout} at 4^2: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= BAND, errs
    assert torch.equal(cat[..., cout:], keep[..., cout:])


# ------------------------------------------------------------------------------------------------------------ model
def _net(pkg, st):
    net = pkg.WaterNet()
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


def _golden_step(pkg, tag, wref_mod=wref):
    """one train step (BCELoss, FusedAdam 1e-4, weight decay 1e-4) and an eval forward on a fixture's inputs -> CPU tensors"""
    meta = json.load(open(os.path.join(GOLDEN, f"waternet_{tag}.json")))
    net = _net(pkg, wref_mod.init_state(seed=meta["seed"], perturb_bn=True))
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
    """test_hrnet_train_step_matches_reference's bands: probabilities, loss, gradient norms, sampled gradients, BatchNorm buffers, the Adam
    step and the eval forward; the analytically zero gradients (waternet_ref.ZERO_GRAD: the conv biases in front of a train-mode BatchNorm)
    within 1e-4 of the largest gradient norm, absolute."""
    meta = json.load(open(os.path.join(GOLDEN, f"waternet_{tag}.json")))
    gold = load_npz(f"waternet_{tag}.npz")
    a, b = _pick(gold, "prob", res["prob"])
    assert np.abs(a - b).max() <= 1e-3, np.abs(a - b).max()
    assert abs(res["loss"] - float(gold["loss"])) <= 1e-4
    names = meta["param_names"]
    assert res["names"] == names
    gn = np.array([g.double().norm().item() for g in res["grads"]])
    ref = gold["grad_norm"]
    real = np.array([k not in wref.ZERO_GRAD for k in names])
    rel = np.abs(gn - ref) / (ref + 1e-3 * ref.max())
    print(f"\nWaterNet {tag} ({what}): loss {res['loss']:.6f} (reference {float(gold['loss']):.6f}), worst gradient-norm error {rel[real].max():.1e}")
    assert rel[real].max() < 2e-2, (names[int(np.argmax(np.where(real, rel, 0)))], rel[real].max())
    gmax = max(float(np.abs(v).max()) for kk, v in gold.items() if kk.startswith("grad/") and not kk.endswith("/meta"))
    for k, g in zip(names, res["grads"]):
        a, b = _pick(gold, "grad/" + k, g)
        if k in wref.ZERO_GRAD:
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
def test_waternet_train_step_matches_reference(pkg, tag):
    """loss, probabilities, gradients, BatchNorm buffers, Adam deltas and the eval forward of both fixtures (bottleneck 4 x 4 and 8 x 8) at
    test_gpu_hrnet.py's golden-step tolerances (_check_golden_step)"""
    B = _mod("blocks")
    assert B.FUSED_WATER_INDEX, "run the suite without RUNET_NO_FUSED_WATER_INDEX"
    _check_golden_step(tag, _golden_step(pkg, tag), "fused")


def _record_decisions(monkeypatch, x):
    """Wraps waternet.waternet_backward: the step's 15 ReLU masks and three pool winners in the restatement's call order
    (waternet_ref.DECISION_SITES).  The encoder / decoder masks come from the saved BatchNorm inputs and coefficients with bn_apply's own
    arithmetic.  The index branch's 16-channel BatchNorm input exists only in registers: its mask is taken from the same coefficients applied
    to the 1x1 convolution evaluated by the shared kernel (a value there can differ from the fused kernel's in the last bit)."""
    import decisions_seq as DS
    B, ops = _mod("blocks"), _mod("ops")
    wn = _mod("waternet")
    got = {}
    real = wn.waternet_backward

    def spy(net_, C, dprob):
        def mask(k):
            return (B.bn_apply(C[k]["t"], C[k]["s"], C[k]["h"], None, relu=True) > 0).permute(0, 3, 1, 2).cpu()
        wi = C["wi"]
        z = ops.conv_fwd(B.to_nhwc_pad(x, 4), wi["p"].w1, wi["p"].b1)
        dec = [(B.bn_apply(z, wi["scale"], wi["shift"], None, relu=True) > 0).permute(0, 3, 1, 2).cpu()]
        for lvl in (1, 2, 3):
            dec += [mask(f"enc{lvl}.0"), mask(f"enc{lvl}.3")]
            dec.append(DS.pool_flat_2x2(C["pools"][lvl].permute(0, 3, 1, 2).cpu().long(), x.shape[3] >> (lvl - 1)))
        for k in ("bottleneck", "dec3", "dec2", "dec1"):
            dec += [mask(f"{k}.0"), mask(f"{k}.3")]
        got["dec"] = dec
        return real(net_, C, dprob)

    monkeypatch.setattr(wn, "waternet_backward", spy)
    return got


def _oracle(st, x, y, forced=None):
    """the restatement in float64"""
    import decisions_seq as DS
    names = wref.param_names()
    P = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in st.items()}
    for k in names:
        P[k].requires_grad_(True)
    out = {}

    def step(rec):
        out["p"] = wref.forward(P, x.double(), True)
        return (lambda q: out.setdefault("loss", wref.bce_mean(q, y.double()))), out["p"], None
    log, pr = DS.run_oracle(wref, step, forced)
    return log, {k: P[k].grad for k in names}, pr


@pytest.mark.parametrize("n,size,seed", [(2, 32, 5), (2, 64, 6)])
def test_waternet_gradients_under_the_hip_decisions(pkg, n, size, seed, monkeypatch):
    """tests/decisions_seq.py's two-part check against the restatement in float64: ReLU masks and pool winners on which the HIP step and the
    restatement differ are near-ties, and under the HIP step's own decisions every gradient (but the analytically zero ones) is within 5e-4
    of its tensor's scale, median within 3e-5 (test_gpu_hrnet.py's bounds)."""
    import decisions_seq as DS
    st = wref.init_state(seed=seed, perturb_bn=True)
    net = _net(pkg, st)
    x, y = pkg.synthetic_batch(n, size, seed=seed)
    xd = x.to(DEV)
    got = _record_decisions(monkeypatch, xd)
    prob = net(xd)
    pkg.bce_loss(prob, y.to(DEV)).backward()
    torch.cuda.synchronize()
    log, _, ref_prob = _oracle(st, x, y)
    assert float((prob.detach().cpu().double() - ref_prob).abs().max()) <= 1e-3
    assert len(log) == len(got["dec"]) == len(wref.DECISION_SITES) == 18
    flips = DS.differing(got["dec"], log)
    DS.assert_near_ties(flips)
    _, gref, _ = _oracle(st, x, y, got["dec"])
    rows = DS.grad_errors({k: p.grad.detach().cpu() for k, p in net.named_parameters()}, gref, set(wref.ZERO_GRAD))
    med = float(np.median([r[0] for r in rows]))
    print(f"\nWaterNet {n} x {size}^2: {len(flips)} near-tie decisions forced; worst gradient errors / scale "
          f"{[(f'{e:.1e}', k) for e, k in rows[:4]]}, median {med:.1e}")
    assert rows[0][0] <= 5e-4, rows[:4]
    assert med <= 3e-5, med


def test_waternet_non_square_forward_and_bounds(pkg):
    """2 x 3 x 40 x 72 (bottleneck 5 x 9) and 2 x 3 x 16 x 16 (bottleneck 2 x 2) against the restatement, the stand-alone WaterIndexModule, a
    non-contiguous input; what the module refuses"""
    st = wref.init_state(seed=9, perturb_bn=True)
    net = _net(pkg, st)
    x, _ = pkg.synthetic_batch(2, 72, seed=9)
    for xs in (x[:, :, :40, :].contiguous(), x[:, :, 8:24, 16:32].contiguous()):
        with torch.no_grad():
            got = net(xs.to(DEV)).cpu()
            want = wref.forward({k: v.clone() for k, v in st.items()}, xs, True)
        assert got.shape == (2, 1) + tuple(xs.shape[2:])
        assert float((got - want).abs().max()) <= 1e-3, (tuple(xs.shape), float((got - want).abs().max()))
    with torch.no_grad():
        view = x.to(DEV)[:, :, 8:24, 16:32]
        assert not view.is_contiguous()
        idx = net.water_index(view).cpu()
        want = wref.water_index({k: v.clone() for k, v in st.items()}, x[:, :, 8:24, 16:32], True)
    assert idx.shape == (2, 4, 16, 16) and float((idx - want).abs().max()) <= 1e-5
    xs, ys = pkg.synthetic_batch(2, 16, seed=10)
    loss = pkg.bce_loss(net(xs.to(DEV)), ys.to(DEV))
    loss.backward()
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    with pytest.raises(ValueError):
        net(torch.zeros((1, 3, 20, 28), device=DEV))
    with pytest.raises(ValueError):
        net(torch.zeros((1, 4, 16, 16), device=DEV))
    with pytest.raises(TypeError):
        net(torch.zeros((1, 3, 16, 16), device=DEV, dtype=torch.float16))
    with pytest.raises(ValueError):
        pkg.WaterNet(n_classes=2)
    with pytest.raises(ValueError):
        net.set_precision("bf16")
    with pytest.raises(NotImplementedError):
        net.sync_bn_hook = object()


_AB_CODE = ("import importlib, sys, torch; sys.path[:0] = [%r, %r]; pkg = importlib.import_module(%r); import test_gpu_waternet as T\n"
            "assert not importlib.import_module(%r).FUSED_WATER_INDEX\n"
            "torch.save({tag: T._golden_step(pkg, tag) for tag in ('n2_s32', 'n2_s64')}, sys.argv[1])\n" % (ROOT, os.path.join(ROOT, "tests"), PKG, PKG + ".blocks"))


def test_waternet_unfused_partner_gives_the_same_step(pkg):
    """RUNET_NO_FUSED_WATER_INDEX=1, selected in a fresh child process (the switch is read at import), gives the golden train step of both
    fixtures within the same tolerances as the fused default (_check_golden_step).  The two front ends differ in the last bits of the index
    channels, which can move a max-pool winner or a ReLU mask at a near-tie downstream: the steps are compared with the reference at the
    golden-step tolerances, not with each other bit for bit."""
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"waternet_ab_{os.getpid()}.pt")
    r = subprocess.run([sys.executable, "-c", _AB_CODE, path], env=dict(os.environ, RUNET_NO_FUSED_WATER_INDEX="1"), timeout=600, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    other = torch.load(path)
    os.remove(path)
    for tag in ("n2_s32", "n2_s64"):
        _check_golden_step(tag, other[tag], "RUNET_NO_FUSED_WATER_INDEX=1")


def test_waternet_step_is_deterministic_and_captures(pkg):
    """2 x 64^2: two steps from an identical state give identical bits; TrainStep(graph=True) replay == eager, bit for bit, with p.grad at
    fixed addresses."""
    trainer = _mod("trainer")
    st = wref.init_state(seed=3, perturb_bn=True)
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


def test_waternet_trains_under_model_evaluator(pkg):
    """ModelEvaluator.train_model / evaluate_model drive WaterNet unchanged for 2 epochs; the eval-mode forward of the trained weights equals
    the restatement on the same state."""
    net = _net(pkg, wref.init_state(seed=1))
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
        want = wref.forward(st, x, training=False)
    assert float((got - want).abs().max()) <= 1e-3
