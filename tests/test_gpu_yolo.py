"""GPU: the YOLOSeg baseline (the reference's Main_Final.py:436-510, BCELoss + Adam :551-552) on the HIP kernels.

  kernel parity   the LeakyReLU BatchNorm apply, the fused BatchNorm + LeakyReLU + 2x2 max-pool forward and the pooled-gradient backward are
                  bit-identical to the compositions they replace (and to aten's leaky_relu / max_pool2d_with_indices on the same z);
                  runet_convt4_igemm_stats leaves y bit-identical to runet_convt4_igemm and the statistics of runet_bn_stats
  model           one train step against the reference goldens (tests/golden/yolo_*), decision-aware gradient parity against the CPU
                  restatement (tests/yolo_ref.py), the 16 x 256^2 benchmark size (determinism, graph capture), ModelEvaluator
"""
import importlib
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, load_npz

import yolo_ref as yref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PKG = "eusipco-2026-robust-unet_amd"
SLOPE = 0.1
POOL_SHAPES = [(256, 256, 32), (128, 128, 64), (64, 64, 128), (32, 32, 256)]        # the backbone's stage ends at 16 x 256^2
DEC_SHAPES = [(16, 16, 256, 128), (32, 32, 128, 64), (64, 64, 64, 32), (128, 128, 32, 16)]   # seg_head's transposed convs: (h, w, cin, cout)


def _B():
    return importlib.import_module(PKG + ".blocks")


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _bn_state(c, seed, neg=False):
    B = _B()
    g = torch.Generator().manual_seed(seed)
    w = 1.0 + 0.3 * torch.randn(c, generator=g)
    if neg:
        w[::3] = -w[::3].abs()
    return B.BNState(w.to(DEV), (0.2 * torch.randn(c, generator=g)).to(DEV), (0.1 * torch.randn(c, generator=g)).to(DEV),
                     (1.0 + torch.rand(c, generator=g)).to(DEV), torch.zeros((), dtype=torch.int64, device=DEV))


def _bn_coeffs(t, training, seed, neg=False):
    B = _B()
    s, h, mean, invstd, _ = B.bn_coeff(t, _bn_state(t.shape[3], seed, neg), training, B.Small(t.device))
    return s, h, mean, invstd


def _z(t, s, h):
    """z = t * scale + shift with the library's own expression (bn_apply without activation)"""
    return _B().bn_apply(t, s, h, None, relu=False)


def _aten_pool(a_nhwc):
    """aten max_pool2d_with_indices on an NHWC activation -> (values NHWC, window bytes NHWC)"""
    y, i = F.max_pool2d(a_nhwc.permute(0, 3, 1, 2), 2, 2, return_indices=True)
    w = a_nhwc.shape[2]
    hh, ww = i // w, i % w
    code = ((hh & 1) * 2 + (ww & 1)).to(torch.uint8)
    return y.permute(0, 2, 3, 1), code.permute(0, 2, 3, 1)


@pytest.mark.parametrize("h,w,c", POOL_SHAPES + [(18, 22, 12)])
@pytest.mark.parametrize("training", [True, False])
def test_leaky_apply_and_fused_pool_are_the_composition_bit_for_bit(pkg, h, w, c, training):
    B = _B()
    n = 16 if h <= 32 else 4
    g = torch.Generator().manual_seed(h * 7 + c)
    t = (0.5 * torch.randn((n, h, w, c), generator=g) + 0.1).to(DEV)
    s, sh, _, _ = _bn_coeffs(t, training, seed=c, neg=True)
    z = _z(t, s, sh)
    a = B.bn_apply_leaky(t, s, sh, SLOPE)
    assert _same(a, F.leaky_relu(z, SLOPE))                          # aten's leaky_relu on the same z
    y0, i0 = B.maxpool_forward(a)                                      # the composition it replaces
    y1, i1 = B.bn_leaky_maxpool_forward(t, s, sh, SLOPE)
    torch.cuda.synchronize()
    assert _same(y0, y1), float((y0 - y1).abs().max())
    assert torch.equal(i0, i1), int((i0 != i1).sum())
    ya, ia = _aten_pool(F.leaky_relu(z, SLOPE))
    assert _same(y1, ya) and torch.equal(i1, ia)


def test_fused_leaky_pool_ties_negative_windows_and_nan(pkg):
    """scale 1, shift 0: z = t except for -0.0 (the fused multiply-add gives +0.0).  Windows with equal values, all-negative windows (the
    LeakyReLU keeps them apart, unlike ReLU), zeros and NaN: values and bytes equal aten's max_pool2d_with_indices on leaky_relu(z) (first
    maximum, NaN wins)."""
    B = _B()
    n, h, w, c = 2, 8, 8, 8
    g = torch.Generator().manual_seed(3)
    t = torch.randn((n, h, w, c), generator=g)
    t[:, 0:2, 0:2, :] = 0.75                                           # ties
    t[:, 2:4, 0:2, :] = -torch.rand((n, 2, 2, c), generator=g) - 0.1    # all negative
    t[:, 4:6, 0:2, :] = -0.5                                           # negative ties
    t[:, 6:8, 0:2, :] = -0.0
    t[0, 0, 2, 0] = float("nan")
    t[0, 1, 3, 1] = float("nan")
    t[1, 2, 2, 2], t[1, 3, 3, 2] = float("nan"), float("nan")
    t = t.to(DEV)
    one, zero = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    y, idx = B.bn_leaky_maxpool_forward(t, one, zero, SLOPE)
    ya, ia = _aten_pool(F.leaky_relu(_z(t, one, zero), SLOPE))
    torch.cuda.synchronize()
    assert _same(y, ya)
    assert torch.equal(idx, ia)
    assert bool(torch.isnan(y[0, 0, 1, 0])) and bool(torch.isnan(y[1, 1, 1, 2]))


@pytest.mark.parametrize("h,w,c", POOL_SHAPES + [(18, 22, 12)])
@pytest.mark.parametrize("training", [True, False])
def test_leaky_backward_and_pooled_backward_are_the_composition_bit_for_bit(pkg, h, w, c, training):
    """bn_backward_leaky == aten's leaky_relu_backward on the same z followed by the plain BatchNorm backward; the pooled form == the scatter
    runet_maxpool2_bwd followed by bn_backward_leaky (dx and the dgamma / dbeta sums)."""
    B = _B()
    n = 16 if h <= 32 else 4
    g = torch.Generator().manual_seed(h + c)
    t = (0.5 * torch.randn((n, h, w, c), generator=g) - 0.05).to(DEV)
    s, sh, mean, invstd = _bn_coeffs(t, training, seed=c + 1, neg=True)
    y, idx = B.bn_leaky_maxpool_forward(t, s, sh, SLOPE)
    dp = torch.randn(y.shape, generator=g).to(DEV)
    full = B.maxpool_backward(dp, idx)
    z = _z(t, s, sh)
    gz = torch.ops.aten.leaky_relu_backward(full, z, SLOPE, False)
    sums_a = torch.empty(2 * c, device=DEV)
    dx_a = B.bn_backward(gz, t, mean, invstd, s, sums_a, training=training)
    sums_b = torch.empty(2 * c, device=DEV)
    dx_b = B.bn_backward_leaky(full, t, mean, invstd, s, sums_b, sh, SLOPE, training=training)
    sums_c = torch.empty(2 * c, device=DEV)
    dx_c = B.bn_backward_pooled_leaky(dp, idx, t, mean, invstd, s, sums_c, sh, SLOPE, training=training)
    torch.cuda.synchronize()
    assert _same(dx_a, dx_b) and _same(sums_a, sums_b)
    assert _same(dx_b, dx_c), float((dx_b - dx_c).abs().max())
    assert _same(sums_b, sums_c)


@pytest.mark.parametrize("h,w,cin,cout", DEC_SHAPES)
def test_convt4_epilogue_statistics(pkg, h, w, cin, cout):
    """runet_convt4_igemm_stats: y bit-identical to runet_convt4_igemm; the finalized batch statistics within 1e-5 (relative) of runet_bn_stats
    over the same y."""
    B = _B()
    ops = importlib.import_module(PKG + ".ops")
    g = torch.Generator().manual_seed(cin + h)
    x = torch.randn((16, h, w, cin), generator=g).to(DEV)
    wt = (torch.randn((4, 4, cin, cout), generator=g) / (4 * cin ** 0.5)).to(DEV)
    bias = (0.1 * torch.randn(cout, generator=g) + 0.3).to(DEV)
    y0 = ops.convt4_fwd(x, wt, bias)
    lib = pkg_lib()
    nparts = lib.runet_convt4_igemm_stats_parts(16, h, w, cout)
    fs = {"part": torch.empty(nparts * cout * 3, device=DEV), "nparts": nparts}
    y1 = torch.empty_like(y0)
    assert lib.runet_convt4_igemm_stats(x.data_ptr(), cin, wt.data_ptr(), bias.data_ptr(), y1.data_ptr(), cout, 16, h, w, cin, cout,
                                        fs["part"].data_ptr(), ops.stream()) == 0
    via = {}
    ops.convt4_fwd(x, wt, bias, stats=via)
    assert ("part" in via) == (cout >= 32 and ops.EPILOGUE_STATS)      # the model's dispatch: the epilogue only where it was measured faster
    sm = B.Small(x.device)
    st0, st1 = _bn_state(cout, 1), _bn_state(cout, 1)
    _, _, m0, i0, _ = B.bn_coeff(y0, st0, True, sm)
    _, _, m1, i1, _ = B.bn_coeff(y1, st1, True, sm, fused=fs)
    torch.cuda.synchronize()
    assert _same(y0, y1)
    v0, v1 = 1.0 / i0.double() ** 2, 1.0 / i1.double() ** 2
    assert float(((v1 - v0).abs() / v0).max()) <= 1e-5
    assert float(((m1.double() - m0.double()).abs() / (m0.double().abs() + v0.sqrt())).max()) <= 1e-5
    assert float(((st1.running_var.double() - st0.running_var.double()).abs() / st0.running_var.double()).max()) <= 1e-5
    assert int(st1.nbt) == 1


def pkg_lib():
    return importlib.import_module(PKG + "._lib").lib


def test_leaky_pool_custom_op(pkg):
    """runet::bn_leaky_maxpool2_nhwc against aten (values, bytes, and the gradients of t, scale and shift in float64), and opcheck."""
    importlib.import_module(PKG + ".custom_ops")
    g = torch.Generator().manual_seed(21)
    t = torch.randn((2, 12, 20, 16), generator=g)
    s, sh = torch.randn(16, generator=g), torch.randn(16, generator=g)
    td, sd, hd = (v.to(DEV).requires_grad_(True) for v in (t, s, sh))
    y, idx = torch.ops.runet.bn_leaky_maxpool2_nhwc(td, sd, hd, SLOPE)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy.to(DEV))
    tr, sr, hr = (v.double().requires_grad_(True) for v in (t, s, sh))
    zr = tr.permute(0, 3, 1, 2) * sr.view(1, -1, 1, 1) + hr.view(1, -1, 1, 1)
    yr, ir = F.max_pool2d(F.leaky_relu(zr, SLOPE), 2, 2, return_indices=True)
    yr.backward(gy.double().permute(0, 3, 1, 2))
    assert float((y.detach().cpu().double() - yr.detach().permute(0, 2, 3, 1)).abs().max()) <= 1e-5 * float(yr.abs().max())
    hh, ww = ir // 20, ir % 20
    assert torch.equal(idx.cpu(), ((hh & 1) * 2 + (ww & 1)).to(torch.uint8).permute(0, 2, 3, 1))
    for a, b in ((td.grad, tr.grad), (sd.grad, sr.grad), (hd.grad, hr.grad)):
        b = b.detach()
        assert float((a.cpu().double() - b).abs().max()) <= 1e-5 * max(1.0, float(b.abs().max())), (a, b)
    torch.library.opcheck(torch.ops.runet.bn_leaky_maxpool2_nhwc.default, (t.to(DEV), s.to(DEV), sh.to(DEV), SLOPE),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
    torch.library.opcheck(torch.ops.runet.bn_leaky_maxpool2_nhwc_bwd.default,
                          (gy.to(DEV), idx.detach(), t.to(DEV), s.to(DEV), sh.to(DEV), SLOPE), test_utils=("test_schema", "test_faketensor"))


# ----------------------------------------------------------------------------------------------------------------- model
_PRE_BN = {f"{name}.bias" for name, _, kind in yref.module_spec() if kind in ("conv", "convt") and name != f"seg_head.{3 * len(yref.DEC)}"}


def _pre_bn_bias(k):
    """conv bias in front of a train-mode BatchNorm (every conv but the head): analytically zero gradient, rounding noise on both sides"""
    return k in _PRE_BN


def _net(pkg, st):
    net = pkg.YOLOSeg()
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
def test_yolo_train_step_matches_reference(pkg, tag):
    meta = json.load(open(os.path.join(GOLDEN, f"yolo_{tag}.json")))
    gold = load_npz(f"yolo_{tag}.npz")
    st = yref.init_state(seed=meta["seed"], perturb_bn=True)
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
    real = np.array([not _pre_bn_bias(k) for k in names])
    rel = np.abs(gn - ref) / (ref + 1e-3 * ref.max())
    assert rel[real].max() < 2e-2, (names[int(np.argmax(np.where(real, rel, 0)))], rel[real].max())
    gmax = max(float(np.abs(v).max()) for kk, v in gold.items() if kk.startswith("grad/") and not kk.endswith("/meta"))
    for k, p in net.named_parameters():
        if _pre_bn_bias(k):
            continue
        a, b = _pick(gold, "grad/" + k, p.grad)
        scale = max(float(np.abs(b).max()), 1e-3 * gmax)
        err = np.abs(a - b)
        assert err.max() <= 0.2 * scale and int((err > 3e-2 * scale).sum()) <= max(1, err.size // 100), (k, err.max(), scale)
        assert float(np.linalg.norm(a - b)) <= 1e-2 * scale * np.sqrt(err.size), (k, float(np.linalg.norm(a - b)), scale)
    for k, buf in net.named_buffers():
        if f"buf/{k}" in gold:
            np.testing.assert_allclose(buf.cpu().numpy(), gold[f"buf/{k}"], rtol=1e-3, atol=1e-4, err_msg=k)
    opt.step()
    delta = np.array([(p.detach().cpu().double() - st[k].double()).abs().sum().item() for k, p in net.named_parameters()])
    np.testing.assert_allclose(delta[real], gold["param_delta_abs_sum"][real], rtol=2e-2, atol=1e-9)
    for k, p in net.named_parameters():
        a, b = _pick(gold, "adam/" + k, p)
        assert np.abs(a - b).max() <= 2.1e-4, (k, np.abs(a - b).max())
    net.eval()
    with torch.no_grad():
        pe = net(x.to(DEV))
    a, b = _pick(gold, "eval_prob", pe)
    assert np.abs(a - b).max() <= 2e-3, np.abs(a - b).max()


def _record_decisions(monkeypatch, size):
    """Wraps yolo.yolo_backward: while the saved context is alive, record the step's LeakyReLU branches (z > 0 from the saved BatchNorm input
    and coefficients with bn_apply's own arithmetic) and pool winners (ATen flat indices) in the restatement's call order."""
    import decisions_seq as DS
    B = _B()
    yolo = importlib.import_module(PKG + ".yolo")
    got = {}
    real = yolo.yolo_backward

    def mask(c):
        return (B.bn_apply(c["t"], c["s"], c["h"], None, relu=False) > 0).permute(0, 3, 1, 2).cpu()

    def spy(net_, C, dprob):
        dec = []
        for si, (layers, _) in enumerate(yolo.LAYOUT):
            for ci, _ in layers:
                dec.append(mask(C[ci]))
            dec.append(DS.pool_flat_2x2(C[layers[-1][0]]["idx"].permute(0, 3, 1, 2).cpu().long(), size >> si))
        for i in range(len(yolo.DEC)):
            dec.append(mask(C[f"dec{i}"]))
        got["dec"] = dec
        return real(net_, C, dprob)

    monkeypatch.setattr(yolo, "yolo_backward", spy)
    return got


def _oracle(st, x, y, forced=None):
    import decisions_yolo as DY
    names = yref.param_names()
    P = {k: v.clone() for k, v in st.items()}
    for k in names:
        P[k].requires_grad_(True)
    out = {}

    def step(rec):
        out["p"], out["z"] = yref.forward(P, x, True, want_logit=True)
        return (lambda q: out.setdefault("loss", yref.bce_mean(q, y))), out["p"], None
    log, pr = DY.run_oracle(yref, step, forced)
    return log, {k: P[k].grad for k in names}, pr


@pytest.mark.parametrize("n,size,seed", [(2, 64, 5), (2, 128, 6)])
def test_yolo_gradients_under_the_hip_decisions(pkg, n, size, seed, monkeypatch):
    """tests/decisions_seq.py's two-part check: LeakyReLU branches and pool winners on which the HIP step and the restatement differ are
    near-ties, and under the HIP step's own decisions every element of every gradient is within 5e-4 of its tensor's scale, median within 3e-5."""
    import decisions_seq as DS
    st = yref.init_state(seed=seed, perturb_bn=True)
    net = _net(pkg, st)
    x, y = pkg.synthetic_batch(n, size, seed=seed)
    got = _record_decisions(monkeypatch, size)
    prob = net(x.to(DEV))
    pkg.bce_loss(prob, y.to(DEV)).backward()
    torch.cuda.synchronize()
    names = yref.param_names()
    log, _, ref_prob = _oracle(st, x, y)
    assert float((prob.detach().cpu() - ref_prob).abs().max()) <= 1e-3
    flips = DS.differing(got["dec"], log)
    DS.assert_near_ties(flips)
    _, gref, _ = _oracle(st, x, y, got["dec"])
    skip = {k for k in names if _pre_bn_bias(k)}
    rows = DS.grad_errors({k: p.grad.detach().cpu() for k, p in net.named_parameters()}, gref, skip)
    med = float(np.median([r[0] for r in rows]))
    print(f"\nYOLOSeg {n} x {size}^2: {len(flips)} near-tie decisions forced; worst gradient errors / scale "
          f"{[(f'{e:.1e}', k) for e, k in rows[:4]]}, median {med:.1e}")
    assert rows[0][0] <= 5e-4, rows[:4]
    assert med <= 3e-5, med


def test_yolo_benchmark_size_is_deterministic_and_captures(pkg):
    """16 x 256^2: finite loss; two steps from an identical state give identical bits; TrainStep(graph=True) replay == eager, bit for bit."""
    trainer = importlib.import_module(PKG + ".trainer")
    st = yref.init_state(seed=3, perturb_bn=True)
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


def test_yolo_trains_under_model_evaluator(pkg):
    """ModelEvaluator.train_model / evaluate_model (Main_Final.py:549-...) drive YOLOSeg unchanged; the eval-mode forward of the trained
    weights equals the restatement on the same state."""
    net = _net(pkg, yref.init_state(seed=1))
    with pytest.raises(ValueError):
        net(torch.zeros((1, 3, 40, 48), device=DEV))
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
        want = yref.forward(st, x, training=False)
    assert float((got - want).abs().max()) <= 1e-3


@pytest.mark.parametrize("env", ["RUNET_NO_FUSED_LEAKY_POOL", "RUNET_NO_EPILOGUE_STATS"])
def test_yolo_unfused_partners_give_the_same_step(pkg, env):
    """The A/B partners (each switch in a fresh process, as the flags are read at import) give the same loss and gradients: bit for bit without
    the fused pool; within 2e-3 of each tensor's scale without the epilogue statistics (the partials are combined in another order, which may move a near-tie LeakyReLU branch)."""
    import subprocess
    import sys
    code = ("import importlib, sys, torch; sys.path[:0] = [%r, %r]; pkg = importlib.import_module(%r); import yolo_ref as yref\n"
            "net = pkg.YOLOSeg(); net.load_state_dict(yref.init_state(seed=4)); net = net.to('cuda:0').train()\n"
            "x, y = pkg.synthetic_batch(2, 64, seed=4); loss = pkg.bce_loss(net(x.to('cuda:0')), y.to('cuda:0')); loss.backward()\n"
            "torch.save([loss.detach().cpu()] + [p.grad.cpu() for p in net.parameters()], sys.argv[1])\n"
            % (os.path.dirname(GOLDEN[:-len('/golden')]), os.path.dirname(GOLDEN), PKG))
    outs = []
    for flag in ("0", "1"):
        path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"yolo_ab_{env}_{flag}_{os.getpid()}.pt")
        r = subprocess.run([sys.executable, "-c", code, path], env=dict(os.environ, **{env: flag}), timeout=600, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(torch.load(path))
        os.remove(path)
    for a, b in zip(*outs):
        if env == "RUNET_NO_FUSED_LEAKY_POOL":
            assert _same(a, b)
        else:
            assert float((a - b).abs().max()) <= 2e-3 * max(1e-3, float(b.abs().max()))
