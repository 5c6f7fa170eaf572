"""GPU: the 64 -> 1 output head folded into the tail kernels of the ResidualBlock in front of it (blocks.FUSED_HEAD).

runet_rb_out_head                          == runet_rb_out_ex (no pool) + runet_outc_fwd on the `out` it wrote
runet_outc_bwd_dl + runet_rb_bwd1_rank1    == runet_outc_bwd + runet_rb_bwd1_ex on the dx it wrote

Both rewrites perform the same operations on the same operands (the 16 lanes of a pixel are the same 16 lanes in all of these kernels at
C = 64), so every comparison with the separate launches is torch.equal.  Both also go against a float64 restatement under the bound of
tests/test_gpu_attention_kernels.py, which pins rb_out / rb_bwd1: 1e-5 of each reference tensor's largest magnitude, the reference evaluated
under the kernel's own ReLU mask, and a mask element on which the two differ is a near-tie (|ReLU input| <= 2e-5 of the tensor's scale).
Any other width than 64 keeps the separate launches."""
import copy
import importlib

import pytest
import torch

from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TOL = 1e-5            # tests/test_gpu_attention_kernels.py
NEAR_TIE = 2e-5
SHAPES = [(2, 6, 10, 64), (1, 16, 16, 64)]


def _lib():
    L = importlib.import_module(PKG_NAME + "._lib")
    return L.lib, L.check


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


def same(a, b, name):
    assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    assert torch.equal(a, b), (name, int((a != b).sum()))


def close(got, ref, name):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), name
    err = float((got - ref).abs().max()) / float(ref.abs().max())
    print(f"{name}: {err:.2e} of scale")
    assert err <= TOL, (name, err)


def pack_bits(out):
    c = out.shape[-1]
    on = (out > 0).reshape(-1, c // 4, 4).to(torch.int32)
    w = torch.tensor([1, 2, 4, 8], device=out.device, dtype=torch.int32)
    return (on * w).sum(-1).to(torch.uint8)


def unpack_bits(bits, shape):
    b = bits.to(torch.int32)
    return torch.stack([(b >> e) & 1 for e in range(4)], dim=-1).reshape(shape) != 0


def inputs(n, h, w, c, seed):
    g = torch.Generator().manual_seed(seed)
    t2, r = torch.randn((n, h, w, c), generator=g), torch.randn((n, h, w, c), generator=g)
    sa = torch.rand((n, h, w), generator=g)
    A, B = torch.randn((n, c), generator=g), torch.randn((n, c), generator=g) * 0.3
    rs, rh = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    hw, hb = torch.randn(c, generator=g) * 0.2, torch.randn(1, generator=g)
    return [v.to(DEV) for v in (t2, r, sa, A, B, rs, rh, hw, hb)]


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("n,h,w,c", SHAPES)
def test_forward(n, h, w, c, affine):
    lib, check = _lib()
    st = _st()
    assert lib.runet_rb_out_head_supported(c) == 1
    t2, r, sa, A, B, rs, rh, hw, hb = inputs(n, h, w, c, seed=41 + h)
    if not affine:
        rs = rh = None
    P = n * h * w
    head = (t2.data_ptr(), c, A.data_ptr(), B.data_ptr(), sa.data_ptr(), r.data_ptr(), c, _ptr(rs), _ptr(rh))
    out0, bits0 = torch.empty_like(t2), torch.empty((P, c // 4), device=DEV, dtype=torch.uint8)
    logit0, prob0 = torch.empty(P, device=DEV), torch.empty(P, device=DEV)
    check(lib.runet_rb_out_ex(*head, out0.data_ptr(), c, bits0.data_ptr(), None, 0, None, n, h, w, c, st))
    check(lib.runet_outc_fwd(out0.data_ptr(), c, hw.data_ptr(), hb.data_ptr(), logit0.data_ptr(), prob0.data_ptr(), P, c, st))
    for want_bits, want_logit in ((True, True), (True, False), (False, True)):
        out = torch.full_like(t2, float("nan"))
        bits = torch.full((P, c // 4), 0xff, device=DEV, dtype=torch.uint8) if want_bits else None
        logit = torch.full((P,), float("nan"), device=DEV) if want_logit else None
        prob = torch.full((P,), float("nan"), device=DEV)
        check(lib.runet_rb_out_head(*head, out.data_ptr(), c, _ptr(bits), hw.data_ptr(), hb.data_ptr(), _ptr(logit), prob.data_ptr(), n, h, w, c, st))
        same(out, out0, "out")
        same(prob, prob0, "prob")
        if want_bits:
            same(bits, bits0, "relu_bits")
        if want_logit:
            same(logit, logit0, "logit")
    # float64: the tail under the kernel's own ReLU mask, the head on the kernel's own `out`
    d = [v.double() if v is not None else None for v in (t2, r, sa, A, B, rs, rh, hw, hb)]
    res = d[1] * d[5] + d[6] if affine else d[1]
    pre = (d[0] * d[3][:, None, None, :] + d[4][:, None, None, :]) * d[2][..., None] + res
    on = unpack_bits(bits0, pre.shape)
    differ = on != (pre > 0)
    assert float(differ.double().mean()) <= 5e-4
    assert not bool(differ.any()) or float(pre[differ].abs().max()) <= NEAR_TIE * float(pre.abs().max())
    assert 0.3 < float(on.double().mean()) < 0.7
    close(out0, torch.where(on, pre, torch.zeros_like(pre)), "out")
    l64 = (out0.double() * d[7]).sum(-1).reshape(-1) + d[8]
    close(logit0, l64, "logit")
    close(prob0, torch.sigmoid(l64), "prob")


@pytest.mark.parametrize("n,h,w,c", SHAPES)
def test_backward(n, h, w, c):
    lib, check = _lib()
    st = _st()
    t2, _, sa, A, B, _, _, hw, _ = inputs(n, h, w, c, seed=53 + h)
    g = torch.Generator().manual_seed(59 + h)
    x = torch.relu(torch.randn((n, h, w, c), generator=g)).to(DEV)          # the block's output: what the head reads, and the ReLU mask
    P = n * h * w
    dprob, prob = torch.randn(P, generator=g).to(DEV), torch.sigmoid(torch.randn(P, generator=g)).to(DEV)
    bits = pack_bits(x)
    wsf = lib.runet_reduce_workspace_floats(1, P, c)
    ws = torch.zeros(wsf, device=DEV)
    dx0, dw0 = torch.empty_like(x), torch.empty(c + 1, device=DEV)
    check(lib.runet_outc_bwd(dprob.data_ptr(), prob.data_ptr(), x.data_ptr(), c, hw.data_ptr(), dx0.data_ptr(), c, ws.data_ptr(), dw0.data_ptr(), P, c, st))
    dv0, dq0 = torch.empty_like(x), torch.empty(P, device=DEV)
    check(lib.runet_rb_bwd1_ex(dx0.data_ptr(), c, None, 0, None, None, c, bits.data_ptr(), t2.data_ptr(), c, A.data_ptr(), B.data_ptr(), sa.data_ptr(),
                               dv0.data_ptr(), c, dq0.data_ptr(), n, h, w, c, st))
    dl, dw = torch.full((P,), float("nan"), device=DEV), torch.full((c + 1,), float("nan"), device=DEV)
    ws.zero_()
    check(lib.runet_outc_bwd_dl(dprob.data_ptr(), prob.data_ptr(), x.data_ptr(), c, dl.data_ptr(), ws.data_ptr(), dw.data_ptr(), P, c, st))
    dv, dq = torch.full_like(x, float("nan")), torch.full((P,), float("nan"), device=DEV)
    check(lib.runet_rb_bwd1_rank1(dl.data_ptr(), hw.data_ptr(), bits.data_ptr(), t2.data_ptr(), c, A.data_ptr(), B.data_ptr(), sa.data_ptr(), dv.data_ptr(),
                                  c, dq.data_ptr(), n, h, w, c, st))
    same(dw, dw0, "dw_db")
    same(dv, dv0, "dv")
    same(dq, dq0, "dq")
    assert float(dv0.abs().max()) > 0 and float(dq0.abs().max()) > 0
    # float64
    d_dprob, d_prob, d_x, d_w = dprob.double(), prob.double(), x.double(), hw.double()
    dl64 = d_dprob * d_prob * (1 - d_prob)
    close(dl, dl64, "dl")
    dv64 = (dl64.reshape(n, h, w, 1) * d_w) * (d_x > 0)
    close(dv0, dv64, "dv")
    u = t2.double() * A.double()[:, None, None, :] + B.double()[:, None, None, :]
    s = sa.double()
    close(dq0, ((dv64 * u).sum(-1) * s * (1 - s)).reshape(-1), "dq")
    close(dw0[:c], (dl64[:, None] * d_x.reshape(P, c)).sum(0), "dw")
    close(dw0[c:], dl64.sum().reshape(1), "db")


def test_other_widths_keep_the_separate_launches(monkeypatch):
    """C = 32: the entry point refuses, blocks.fuses_head says no, and a RobustUNet of base width 32 goes through outc_forward / outc_backward"""
    lib, check = _lib()
    M = importlib.import_module(PKG_NAME + ".model")
    blocks = importlib.import_module(PKG_NAME + ".blocks")
    assert blocks.FUSED_HEAD and blocks.FUSED_RB_EDGES
    assert lib.runet_rb_out_head_supported(32) == 0
    assert not blocks.fuses_head("fwd", 32) and not blocks.fuses_head("bwd", 32)
    assert blocks.fuses_head("fwd", 64) and blocks.fuses_head("bwd", 64)
    n, h, w, c = 1, 4, 4, 32
    t2, r, sa, A, B, rs, rh, hw, hb = inputs(n, h, w, c, seed=7)
    out, prob = torch.empty_like(t2), torch.empty(n * h * w, device=DEV)
    rc = lib.runet_rb_out_head(t2.data_ptr(), c, A.data_ptr(), B.data_ptr(), sa.data_ptr(), r.data_ptr(), c, None, None, out.data_ptr(), c, None,
                               hw.data_ptr(), hb.data_ptr(), None, prob.data_ptr(), n, h, w, c, _st())
    assert rc != 0 and b"c == 64" in lib.runet_last_error()
    calls = []
    real_f, real_b = blocks.outc_forward, blocks.outc_backward
    monkeypatch.setattr(blocks, "outc_forward", lambda *a, **k: calls.append("fwd") or real_f(*a, **k))
    monkeypatch.setattr(blocks, "outc_backward", lambda *a, **k: calls.append("bwd") or real_b(*a, **k))
    torch.manual_seed(2)
    model = M.RobustUNet(3, 1, 32).to(DEV).train()
    x = torch.randn(1, 3, 64, 64, device=DEV)
    model(x).mean().backward()
    torch.cuda.synchronize()
    assert calls == ["fwd", "bwd"]
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())


def test_model_step_with_the_head_fused_and_not(monkeypatch, pkg, oracle):
    """One train step of RobustUNet(3, 1, 64) at 2 x 64^2: loss, probabilities, logits, every gradient, BatchNorm buffer and updated parameter"""
    blocks = importlib.import_module(PKG_NAME + ".blocks")
    n, size, base, seed = 2, 64, 64, 3
    torch.manual_seed(seed)
    model = pkg.RobustUNet(3, 1, base).to(DEV).train()
    model.set_dropout_masks(oracle.dropout_masks(n, base, seed=seed))
    x, y = pkg.synthetic_batch(n, size, seed=seed)
    x, y = x.to(DEV), y.to(DEV)
    state = copy.deepcopy(model.state_dict())
    seen = {False: [], True: []}
    real_out, real_bwd = blocks.outc_forward, blocks.outc_backward
    res = {}
    for on in (False, True):
        monkeypatch.setattr(blocks, "FUSED_HEAD", on)
        monkeypatch.setattr(blocks, "outc_forward", lambda *a, _on=on, **k: seen[_on].append("fwd") or real_out(*a, **k))
        monkeypatch.setattr(blocks, "outc_backward", lambda *a, _on=on, **k: seen[_on].append("bwd") or real_bwd(*a, **k))
        model.load_state_dict(state)
        for p in model.parameters():
            p.grad = None
        prob, logit = model(x, return_logits=True)
        loss = pkg.bce_loss(prob, y)
        loss.backward()
        grads = {"grad " + k: p.grad.clone() for k, p in model.named_parameters()}
        with torch.no_grad():
            for p in model.parameters():
                p.sub_(0.05 * p.grad)
        torch.cuda.synchronize()
        res[on] = dict(loss=loss.detach().clone(), prob=prob.detach().clone(), logit=logit.detach().clone(), **grads,
                       **{"param " + k: p.detach().clone() for k, p in model.named_parameters()},
                       **{"buffer " + k: b.clone() for k, b in model.named_buffers()})
    assert seen == {False: ["fwd", "bwd"], True: []}
    assert res[False].keys() == res[True].keys()
    for k in res[False]:
        same(res[True][k], res[False][k], k)
    assert float(res[True]["grad inc.conv1.weight"].abs().max()) > 0
