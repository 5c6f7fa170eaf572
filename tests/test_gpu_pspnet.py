"""GPU: the PSPNet baseline (the reference's comne.py:214-299, BCELoss + Adam) on the HIP kernels.

  kernels   the tap-plane kernels (blocks.psp_taps_forward / _backward: the pyramid half of final_conv.0 computed on the 50 cells per image)
            against float64 autograd of F.conv2d(cat[F.interpolate(P_j)], padding=1), and the head kernels (runet_psp_head_*) against float64
            F.batch_norm / relu / mask / 1x1 convolution and their autograd
  model     one train step against the reference goldens (tests/golden/pspnet_*), the same under each RUNET_FUSED_PSP_* switch,
            decision-aware gradient parity against the CPU restatement in float64 (tests/pspnet_ref.py) on both paths, sizes and bounds,
            determinism and graph capture
The error measure is tests/test_gpu_enet.py's: max |got - want| / max |want|, band 1e-5 (fp32 kernels with fp32 statistics); where the shared
matrix-core kernels carry the value (the Z_j = P_j . Wtap_j products and their gradients), tests/test_gpu_conv.py's bands in the same measure
(2e-4, weight gradients 3e-4 x max(1, sqrt(pixels / 256))).  Two runs of every kernel must give the same bits; kernels that write channel
slices of wider buffers must leave the other channels bit-unchanged.
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

import decisions_pspnet as DP
import pspnet_ref as pref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PKG = "eusipco-2026-robust-unet_amd"
BAND = 1e-5
CONV_BAND = 2e-4
EPS = 1e-5
BINS, OFF = (1, 2, 3, 6), (0, 1, 5, 14)


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
    """NCHW -> a dense NHWC tensor with canonical strides"""
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


def _cells(rows, j, n):
    """branch j's [n, b, b, c] image inside a branch-major [50 n, c] buffer (blocks._pyr_view)"""
    b = BINS[j]
    return rows[n * OFF[j]:n * (OFF[j] + b * b)].view(n, b, b, rows.shape[1])


# ------------------------------------------------------------------------------------------------------------ tap planes
@pytest.mark.parametrize("cq,cout", [(4, 8), (128, 512)])
@pytest.mark.parametrize("n,h,w", [(2, 1, 1), (2, 2, 3), (3, 7, 5), (2, 16, 16)])
def test_tap_planes_match_float64(pkg, n, h, w, cq, cout):
    """blocks.psp_taps_forward / _backward against float64 autograd of F.conv2d(cat[F.interpolate(P_j, (h, w))], W, padding=1), the pyramid
    half of final_conv.0: t (accumulated onto a channel slice of a wider random buffer whose neighbours keep their bits), the cells' gradient
    dP and the weight gradient dWtap.  1 x 1: only the centre tap is in range; 2 x 3: smaller than the kernel and the 6-bin grid; 7 x 5: odd,
    divisible by no bin count; 16 x 16: the workload's map (four 128-channel chunks per row at cout = 512)."""
    B = _mod("blocks")
    g = torch.Generator().manual_seed(17 * n + 5 * h + w + cq)
    acts = torch.randn((50 * n, cq), generator=g)
    wt = torch.randn((cout, 4 * cq, 3, 3), generator=g) / (4 * cq * 9) ** 0.5
    t0 = torch.randn((n, h, w, cout), generator=g)
    dt = torch.randn((n, cout, h, w), generator=g)
    a64, w64 = acts.double().requires_grad_(True), wt.double().requires_grad_(True)
    ups = [F.interpolate(_cells(a64, j, n).permute(0, 3, 1, 2), size=(h, w), mode="bilinear", align_corners=False) for j in range(4)]
    y64 = F.conv2d(torch.cat(ups, 1), w64, None, 1, 1)
    y64.backward(dt.double())
    wp = wt.permute(1, 2, 3, 0).contiguous().view(1, 1, 4 * cq, 9 * cout).to(DEV)      # [cin][kh][kw][cout]: blocks.psp_split_weights' second half
    actsd, dtd = acts.to(DEV), _nhwc(dt).to(DEV)
    runs = []
    for _ in range(2):
        ts, tbuf = _in_slice(t0.to(DEV), 4, cout + 12)
        keep = tbuf.clone()
        B.psp_taps_forward(ts, actsd, wp)
        dts, _ = _in_slice(dtd, 8, cout + 8)
        dacts, dwp = B.psp_taps_backward(dts, actsd, wp)
        torch.cuda.synchronize()
        assert _same(tbuf[..., :4], keep[..., :4]) and _same(tbuf[..., 4 + cout:], keep[..., 4 + cout:])
        runs.append((ts.clone(), dacts, dwp))
    for a, b in zip(*runs):
        assert _same(a, b)
    t, dacts, dwp = runs[0]
    dw = dwp.view(4 * cq, 3, 3, cout).permute(3, 0, 1, 2)
    errs = dict(t=_err(_nchw(t.cpu() - t0), y64.detach()), dP=_err(dacts, a64.grad), dWtap=_err(dw, w64.grad))
    print(f"\ntap planes {n}x{h}x{w} cq={cq} cout={cout}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs["t"], errs["dP"]) <= CONV_BAND and errs["dWtap"] <= _wgrad_band(n * 36), errs


# ------------------------------------------------------------------------------------------------------------ head
def _head_case(n, h, w, c, training, masked, seed):
    """float64 reference of z = b + sum_c w * mask * relu(bn(t)) and its gradients, redrawn on the reference only until no pre-ReLU value is
    within 1e-5 of zero (a mask there could differ between fp32 and float64), as test_gpu_enet._tail_case does"""
    for draw in range(64):
        g = torch.Generator().manual_seed(seed + 1000 * draw)
        t, dz = torch.randn((n, c, h, w), generator=g), torch.randn((n, 1, h, w), generator=g)
        ga, be = 1 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
        rm, rv = 0.3 * torch.randn(c, generator=g), 0.5 + torch.rand(c, generator=g)
        wo, bo = torch.randn((1, c, 1, 1), generator=g) / c ** 0.5, torch.randn(1, generator=g)
        mask = None
        if masked:          # p = 0.25, one channel dropped in every image (another one per image)
            mask = torch.full((n, c), 1 / 0.75)
            for i in range(n):
                mask[i, (i * 3 + 1) % c] = 0.0
        t64, ga64, be64, w64, b64 = (v.double().requires_grad_(True) for v in (t, ga, be, wo, bo))
        y = F.batch_norm(t64, rm.double().clone(), rv.double().clone(), ga64, be64, training, 0.1, EPS)
        y.retain_grad()
        if float(y.detach().abs().min()) <= 1e-5:
            continue
        a = F.relu(y)
        if masked:
            a = a * mask.double()[:, :, None, None]
        z = F.conv2d(a, w64, b64)
        z.backward(dz.double())
        return dict(t=t, dz=dz, ga=ga, be=be, rm=rm, rv=rv, wo=wo, bo=bo, mask=mask, z=z.detach(), dt=t64.grad, dy=y.grad, dgamma=ga64.grad,
                    dbeta=be64.grad, dw=w64.grad, db=b64.grad, draws=draw + 1)
    raise AssertionError("no draw without a pre-ReLU value within 1e-5 of zero")


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("n,h,w,c", [(2, 1, 1, 512), (3, 5, 7, 16), (2, 4, 4, 4)])
def test_head_kernels_match_float64(pkg, n, h, w, c, training, masked):
    """runet_psp_head_fwd / _bwd_reduce / _bwd_apply against float64 autograd: z, dt, dw, db and the BatchNorm sums, with batch and with
    running statistics, without and with a Dropout2d mask that drops one channel in every image; t is read from a channel slice and dt written
    into a slice of another width, the neighbours keep their bits.  2 x 1 x 1 in training mode is the two-values-per-channel BatchNorm: its
    input gradient cancels analytically, so dt there is measured against the size of the cancelling terms, max |scale| * max |gradient of
    the BatchNorm's output| (test_gpu_enet.test_tail_fused_and_partner_match_float64); every other figure keeps max |want|."""
    B, L, ops = _mod("blocks"), _mod("_lib"), _mod("ops")
    lib, check = L.lib, L.check
    dev = torch.device(DEV)
    ref = _head_case(n, h, w, c, training, masked, 29 * n + 7 * h + w + c + training)
    assert ref["draws"] <= 8, ref["draws"]
    ts, _ = _in_slice(_nhwc(ref["t"]).to(DEV), 4, c + 8)
    dz = ref["dz"].reshape(n, h, w).contiguous().to(DEV)
    mask = ref["mask"].to(DEV) if masked else None
    mp = mask.data_ptr() if masked else None
    wo, bo = ref["wo"].reshape(c).contiguous().to(DEV), ref["bo"].to(DEV)
    st = ops.stream()
    nws = lib.runet_psp_head_bwd_workspace_floats(n, h, w, c)
    runs = []
    for _ in range(2):
        bn = B.BNState(ref["ga"].to(DEV), ref["be"].to(DEV), ref["rm"].clone().to(DEV), ref["rv"].clone().to(DEV), torch.zeros((), dtype=torch.int64, device=DEV))
        s, hh, mean, invstd, _ = B.bn_coeff(ts, bn, training, B.Small(dev))
        z = torch.empty((n, h, w), device=DEV)
        check(lib.runet_psp_head_fwd(ts.data_ptr(), ops.ld(ts), s.data_ptr(), hh.data_ptr(), mp, wo.data_ptr(), bo.data_ptr(), z.data_ptr(), n, h, w, c, st))
        ws, out = torch.empty(nws, device=DEV), torch.empty(3 * c + 1, device=DEV)
        check(lib.runet_psp_head_bwd_reduce(dz.data_ptr(), ts.data_ptr(), ops.ld(ts), s.data_ptr(), hh.data_ptr(), mp, wo.data_ptr(), mean.data_ptr(),
                                            invstd.data_ptr(), ws.data_ptr(), nws, out.data_ptr(), n, h, w, c, st))
        use = out if training else B.zeros(2 * c, dev)
        dts, dbuf = _in_slice(torch.zeros((n, h, w, c), device=DEV), 8, c + 20)
        keep = dbuf.clone()
        check(lib.runet_psp_head_bwd_apply(dz.data_ptr(), ts.data_ptr(), ops.ld(ts), mp, wo.data_ptr(), dts.data_ptr(), ops.ld(dts), n, h, w, c,
                                           mean.data_ptr(), invstd.data_ptr(), s.data_ptr(), hh.data_ptr(), use.data_ptr(), 0, st))
        torch.cuda.synchronize()
        assert _same(dbuf[..., :8], keep[..., :8]) and _same(dbuf[..., 8 + c:], keep[..., 8 + c:])
        runs.append((z, out, dts.clone()))
    for a, b in zip(*runs):
        assert _same(a, b)
    z, out, dt = runs[0]
    errs = dict(z=_err(z, ref["z"].reshape(n, h, w)), dt=_err(_nchw(dt), ref["dt"]), dgamma=_err(out[:c], ref["dgamma"]), dbeta=_err(out[c:2 * c], ref["dbeta"]),
                dw=_err(out[2 * c:3 * c], ref["dw"].reshape(c)), db=_err(out[3 * c:], ref["db"]))
    if training and n * h * w == 2:
        invstd64 = 1.0 / torch.sqrt(ref["t"].double().var((0, 2, 3), unbiased=False) + EPS)
        terms = max(float((ref["ga"].double() * invstd64).abs().max()) * float(ref["dy"].abs().max()), 1e-30)
        errs["dt"] = float((_nchw(dt).double().cpu() - ref["dt"]).abs().max()) / terms
    print(f"\npsp head {n}x{h}x{w} c={c} {'train' if training else 'eval'} {'mask' if masked else 'nomask'} ({ref['draws']} draw(s)): "
          + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= BAND, errs


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "partner"])
def test_head_paths_match_float64_through_the_resize(pkg, fused):
    """blocks.psp_head_forward / _backward on either path (runet_psp_head_* or runet_bn_apply + runet_outc_*), through the x16 resize and the
    sigmoid, against float64: prob, dt and the (dgamma | dbeta | dw | db) vector"""
    B = _mod("blocks")
    dev = torch.device(DEV)
    n, h, w, c = 3, 5, 7, 16
    ref = _head_case(n, h, w, c, True, True, 77)
    g = torch.Generator().manual_seed(78)
    dprob = torch.randn((n, 1, 16 * h, 16 * w), generator=g)
    t64, ga64, be64, w64, b64 = (ref[k].double().requires_grad_(True) for k in ("t", "ga", "be", "wo", "bo"))
    a = F.relu(F.batch_norm(t64, None, None, ga64, be64, True, 0.1, EPS)) * ref["mask"].double()[:, :, None, None]
    p64 = torch.sigmoid(F.interpolate(F.conv2d(a, w64, b64), scale_factor=16, mode="bilinear", align_corners=False))
    p64.backward(dprob.double())
    td, mask = _nhwc(ref["t"]).to(DEV), ref["mask"].to(DEV)
    wo = ref["wo"].permute(2, 3, 1, 0).contiguous().to(DEV)
    bn = B.BNState(ref["ga"].to(DEV), ref["be"].to(DEV), torch.zeros(c, device=DEV), torch.ones(c, device=DEV), torch.zeros((), dtype=torch.int64, device=DEV))
    s, hh, mean, invstd, _ = B.bn_coeff(td, bn, True, B.Small(dev))
    prob, saved = B.psp_head_forward(td, s, hh, mask, wo, ref["bo"].to(DEV), fused=fused)
    assert (saved is None) == fused
    dt, out = B.psp_head_backward(dprob.to(DEV), prob, td, s, hh, mask, wo, mean, invstd, saved, True)
    torch.cuda.synchronize()
    want = torch.cat([ga64.grad, be64.grad, w64.grad.reshape(c), b64.grad])
    errs = dict(prob=_err(prob, p64.detach()), dt=_err(_nchw(dt), t64.grad), dgamma=_err(out[:c], want[:c]), dbeta=_err(out[c:2 * c], want[c:2 * c]),
                dw=_err(out[2 * c:3 * c], want[2 * c:3 * c]), db=_err(out[3 * c:], want[3 * c:]))
    print(f"\npsp head through the resize ({'fused' if fused else 'partner'}): " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= BAND, errs


# ------------------------------------------------------------------------------------------------------------ model
def _net(pkg, st, masks=None):
    net = pkg.PSPNet()
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
    """one train step (BCELoss, FusedAdam 1e-4, weight decay 1e-4) under the fixture's dropout mask and an eval forward on a fixture's inputs
    -> CPU tensors"""
    meta = json.load(open(os.path.join(GOLDEN, f"pspnet_{tag}.json")))
    net = _net(pkg, pref.init_state(seed=meta["seed"], perturb_bn=True), pref.dropout_masks(meta["n"], meta["seed"]))
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
    """test_gpu_enet._check_golden_step's bands: probabilities, loss, gradient norms, sampled gradients, BatchNorm buffers, the Adam step
    and the eval forward; the analytically zero gradients (pspnet_ref.ZERO_GRAD: the convolution biases in front of a train-mode BatchNorm)
    within 1e-4 of the largest gradient norm, absolute."""
    meta = json.load(open(os.path.join(GOLDEN, f"pspnet_{tag}.json")))
    gold = load_npz(f"pspnet_{tag}.npz")
    a, b = _pick(gold, "prob", res["prob"])
    assert np.abs(a - b).max() <= 1e-3, np.abs(a - b).max()
    assert abs(res["loss"] - float(gold["loss"])) <= 1e-4
    names = meta["param_names"]
    assert res["names"] == names
    gn = np.array([g.double().norm().item() for g in res["grads"]])
    ref = gold["grad_norm"]
    real = np.array([k not in pref.ZERO_GRAD for k in names])
    rel = np.abs(gn - ref) / (ref + 1e-3 * ref.max())
    print(f"\nPSPNet {tag} ({what}): loss {res['loss']:.6f} (reference {float(gold['loss']):.6f}), worst gradient-norm error {rel[real].max():.1e}")
    assert rel[real].max() < 2e-2, (names[int(np.argmax(np.where(real, rel, 0)))], rel[real].max())
    gmax = max(float(np.abs(v).max()) for kk, v in gold.items() if kk.startswith("grad/") and not kk.endswith("/meta"))
    for k, g in zip(names, res["grads"]):
        a, b = _pick(gold, "grad/" + k, g)
        if k in pref.ZERO_GRAD:
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
SWITCHES = ("RUNET_FUSED_PSP_TAPS", "RUNET_FUSED_PSP_HEAD")


@pytest.mark.parametrize("tag", TAGS)
def test_pspnet_train_step_matches_reference(pkg, tag):
    """loss, probabilities, gradients, BatchNorm buffers, Adam deltas and the eval forward of both fixtures (H/16 map 4 x 4: the 6-bin branch
    is resized down; and 6 x 6) at test_gpu_enet.py's golden-step tolerances (_check_golden_step), in the default configuration (the
    reference's order on the shared kernels: neither fusion gained more than the rounds' spread in the 16 x 256^2 step, so both are opt-in)"""
    B = _mod("blocks")
    assert not B.FUSED_PSP_TAPS and not B.FUSED_PSP_HEAD, "run the suite without the RUNET_FUSED_PSP_* switches"
    _check_golden_step(tag, _golden_step(pkg, tag), "default")


_AB_CODE = ("import importlib, sys, torch; sys.path[:0] = [%r, %r]; pkg = importlib.import_module(%r); import test_gpu_pspnet as T\n"
            "B = importlib.import_module(%r)\n"
            "assert (B.FUSED_PSP_TAPS, B.FUSED_PSP_HEAD) == (sys.argv[2] == 'RUNET_FUSED_PSP_TAPS', sys.argv[2] == 'RUNET_FUSED_PSP_HEAD')\n"
            "torch.save({tag: T._golden_step(pkg, tag) for tag in T.TAGS}, sys.argv[1])\n" % (ROOT, os.path.join(ROOT, "tests"), PKG, PKG + ".blocks"))


@pytest.mark.parametrize("switch", SWITCHES)
def test_pspnet_switches_give_the_same_step(pkg, switch):
    """each switch - final_conv.0 as tap planes (runet_psp_taps_*, no concat buffer), the head on runet_psp_head_* -, selected in a fresh child
    process (read at import), gives the golden train step of both fixtures within the same tolerances as the default (_check_golden_step):
    compared with the reference, never with the other path"""
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"pspnet_ab_{switch}_{os.getpid()}.pt")
    r = subprocess.run([sys.executable, "-c", _AB_CODE, path, switch], env={**os.environ, switch: "1"}, timeout=600, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    other = torch.load(path)
    os.remove(path)
    for tag in TAGS:
        _check_golden_step(tag, other[tag], switch + "=1")


@pytest.mark.parametrize("n,size,seed", [(2, 64, 5), (3, 96, 6)])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "partners"])
def test_pspnet_gradients_under_the_hip_decisions(pkg, n, size, seed, fused, monkeypatch):
    """tests/decisions_seq.py's two-part check against the restatement in float64: ReLU masks on which the HIP step and the restatement differ
    are near-ties (decisions.NEAR_TIE), and under the HIP step's own decisions the worst and the median gradient error per tensor scale are
    bounded by what fp32 itself allows: the restatement run in float32 under the same forced decisions gives (worst32, median32) against
    float64, and the HIP step must stay within max(5e-4, 3 x worst32) and max(3e-5, 3 x median32) (test_gpu_enet.py's bounds) - with the tap
    planes and the fused head, and with both partners."""
    import decisions_seq as DS
    B, ps = _mod("blocks"), _mod("pspnet")
    monkeypatch.setattr(B, "FUSED_PSP_TAPS", fused)
    monkeypatch.setattr(B, "FUSED_PSP_HEAD", fused)
    st = pref.init_state(seed=seed, perturb_bn=True)
    masks = pref.dropout_masks(n, seed)
    net = _net(pkg, st, masks)
    x, y = pkg.synthetic_batch(n, size, seed=seed)
    got = {}
    real = ps.pspnet_backward

    def spy(net_, C, dprob):
        assert C["fin"]["taps"] == fused and (C["fin"]["saved"] is None) == fused
        got["dec"] = DP.hip_decisions(B, C, pref)
        return real(net_, C, dprob)
    monkeypatch.setattr(ps, "pspnet_backward", spy)
    prob = net(x.to(DEV))
    pkg.bce_loss(prob, y.to(DEV)).backward()
    torch.cuda.synchronize()
    log, _, ref_prob, _ = pref.step(st, x, y, masks=masks)
    assert float((prob.detach().cpu().double() - ref_prob).abs().max()) <= 1e-3
    assert len(log) == len(got["dec"]) == len(pref.DECISION_SITES) == 9
    flips = DS.differing(got["dec"], log)
    DS.assert_near_ties(flips)
    _, gref, _, _ = pref.step(st, x, y, forced=got["dec"], masks=masks)
    _, g32, _, _ = pref.step(st, x, y, forced=got["dec"], dtype=torch.float32, masks=masks)
    skip = set(pref.ZERO_GRAD)
    rows = DS.grad_errors({k: p.grad.detach().cpu() for k, p in net.named_parameters()}, gref, skip)
    rows32 = DS.grad_errors({k: v.double() for k, v in g32.items()}, gref, skip)
    med, med32 = float(np.median([r[0] for r in rows])), float(np.median([r[0] for r in rows32]))
    print(f"\nPSPNet {n} x {size}^2 ({'tap planes and fused head' if fused else 'partners'}): {len(flips)} near-tie decisions forced; "
          f"HIP worst {rows[0][0]:.1e} ({rows[0][1]}) median {med:.1e}; float32 restatement worst {rows32[0][0]:.1e} ({rows32[0][1]}) median {med32:.1e}")
    assert rows[0][0] <= max(5e-4, 3 * rows32[0][0]), (rows[:4], rows32[:4])
    assert med <= max(3e-5, 3 * med32), (med, med32)


def test_pspnet_sizes_and_bounds(pkg):
    """2 x 3 x 112 x 80 (H/16 map 7 x 5: odd, divisible by no bin count) and 2 x 3 x 16 x 32 (1 x 2: smaller than every grid but the first)
    against the restatement in training mode, a non-contiguous input, eval mode with one 16 x 16 image, a random dropout draw; what the model
    refuses.  The bound is 1e-3 on the probabilities, or three times what the float32 restatement itself is away from the float64 one
    where that is more (at 1 x 2 every BatchNorm behind conv4 sees four values per channel or fewer)."""
    st = pref.init_state(seed=9, perturb_bn=True)
    net = _net(pkg, st)
    net.final_conv[3].p = 0.0          # no dropout: the draws are random
    x, _ = pkg.synthetic_batch(2, 112, seed=9)
    for xs in (x[:, :, :, :80].contiguous(), x[:, :, 8:24, 16:48].contiguous()):
        with torch.no_grad():
            got = net(xs.to(DEV)).cpu()
            want32 = pref.forward({k: v.clone() for k, v in st.items()}, xs, True)
            want = pref.forward({k: (v.double() if v.is_floating_point() else v.clone()) for k, v in st.items()}, xs.double(), True)
        own = float((want32.double() - want).abs().max())
        err = float((got.double() - want).abs().max())
        print(f"\nPSPNet {tuple(xs.shape)}: |HIP - float64| {err:.1e}, |float32 restatement - float64| {own:.1e}")
        assert got.shape == (2, 1) + tuple(xs.shape[2:])
        assert err <= max(1e-3, 3 * own), (tuple(xs.shape), err, own)
    with torch.no_grad():
        view = x.to(DEV)[:, :, 8:72, 16:80]
        assert not view.is_contiguous()
        got = net(view).cpu()
        want = pref.forward({k: v.clone() for k, v in st.items()}, x[:, :, 8:72, 16:80], True)
    assert float((got - want).abs().max()) <= 1e-3
    net.final_conv[3].p = 0.1
    xs, ys = pkg.synthetic_batch(2, 32, seed=10)
    loss = pkg.bce_loss(net(xs.to(DEV)), ys.to(DEV))          # a random Dropout2d draw
    loss.backward()
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        net(xs[:1].to(DEV))
    net.eval()
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        got = net(xs[:1, :, :16, :16].to(DEV)).cpu()
        want = pref.forward(sd, xs[:1, :, :16, :16], False)
    assert float((got - want).abs().max()) <= 1e-3
    net.train()
    with pytest.raises(ValueError):
        net(torch.zeros((2, 3, 40, 32), device=DEV))
    with pytest.raises(ValueError):
        net(torch.zeros((2, 3, 32, 24), device=DEV))
    with pytest.raises(ValueError):
        net(torch.zeros((2, 4, 32, 32), device=DEV))
    with pytest.raises(TypeError):
        net(torch.zeros((2, 3, 32, 32), device=DEV, dtype=torch.float16))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "partners"])
def test_pspnet_step_is_deterministic_and_captures(pkg, fused, monkeypatch):
    """2 x 64^2 under an injected dropout mask: two steps from an identical state give identical bits; TrainStep(graph=True) replay == eager,
    bit for bit, with p.grad at fixed addresses - with the tap planes and the fused head (the split copies of final_conv.0's weight are
    refreshed inside the captured step), and with both partners."""
    trainer, B = _mod("trainer"), _mod("blocks")
    monkeypatch.setattr(B, "FUSED_PSP_TAPS", fused)
    monkeypatch.setattr(B, "FUSED_PSP_HEAD", fused)
    st = pref.init_state(seed=3, perturb_bn=True)
    masks = pref.dropout_masks(2, 3)
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
