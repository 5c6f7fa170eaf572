"""GPU: the ResidualBlock's edges folded into its tail kernels (blocks.FUSED_RB_EDGES) against the separate launches they replace.

runet_rb_out_ex   == runet_rb_out + runet_maxpool2_fwd, plus the ReLU sign bytes
runet_rb_bwd1_ex  == runet_maxpool2_bwd(accumulate=1) + runet_rb_bwd1
runet_rb_bwd3_sc  == runet_rb_bwd3 + runet_bn_bwd_apply(out=dv)

Every rewrite performs the same operations on the same operands, so every comparison is torch.equal: a differing bit is a bug."""
import copy
import importlib

import pytest
import torch

from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _lib():
    L = importlib.import_module(PKG_NAME + "._lib")
    return L.lib, L.check


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


def pack_bits(out):
    """[N,H,W,C] -> [N*H*W, C/4] uint8, bit e of byte j set when out[p, 4j+e] > 0"""
    c = out.shape[-1]
    on = (out > 0).reshape(-1, c // 4, 4).to(torch.int32)
    w = torch.tensor([1, 2, 4, 8], device=out.device, dtype=torch.int32)
    return (on * w).sum(-1).to(torch.uint8)


def same(a, b, name):
    assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    assert torch.equal(a, b), (name, int((a != b).sum()))


def tail_inputs(n, h, w, c, seed):
    """What rb_out reads.  About half of the pre-ReLU values are negative (whole windows of zeros: winner 0); the window at the origin of
    the last image holds one pixel's t2, r and sa four times (four equal values, positive in about half of the channels: winner 0)."""
    g = torch.Generator().manual_seed(seed)
    t2 = torch.randn((n, h, w, c), generator=g)
    r = torch.randn((n, h, w, c), generator=g)
    sa = torch.rand((n, h, w), generator=g)
    for dy in (0, 1):
        for dx in (0, 1):
            t2[n - 1, dy, dx], r[n - 1, dy, dx], sa[n - 1, dy, dx] = t2[n - 1, 0, 0], r[n - 1, 0, 0], sa[n - 1, 0, 0]
    A = torch.randn((n, c), generator=g)
    B = torch.randn((n, c), generator=g) * 0.3
    rs = torch.rand(c, generator=g) + 0.5
    rh = torch.randn(c, generator=g) * 0.3
    return [v.to(DEV) for v in (t2, r, sa, A, B, rs, rh)]


SHAPES = [(2, 4, 6, 64), (1, 4, 4, 128), (1, 2, 2, 512)]


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("n,h,w,c", SHAPES)
def test_forward_edge(n, h, w, c, affine):
    lib, check = _lib()
    st = _st()
    t2, r, sa, A, B, rs, rh = tail_inputs(n, h, w, c, seed=11 + c)
    if not affine:
        rs = rh = None
    P, hw = n * h * w, h * w
    out0 = torch.empty_like(t2)
    check(lib.runet_rb_out(t2.data_ptr(), c, A.data_ptr(), B.data_ptr(), sa.data_ptr(), r.data_ptr(), c, _ptr(rs), _ptr(rh), out0.data_ptr(), c, P, hw,
                           c, st))
    pooled0 = torch.empty((n, h // 2, w // 2, c), device=DEV)
    idx0 = torch.empty((n, h // 2, w // 2, c), device=DEV, dtype=torch.uint8)
    check(lib.runet_maxpool2_fwd(out0.data_ptr(), c, pooled0.data_ptr(), c, idx0.data_ptr(), n, h, w, c, st))
    bits0 = pack_bits(out0)
    # the inputs do hold what the test is about
    zero_win = (pooled0 == 0)
    assert bool(zero_win.any()) and bool((idx0[zero_win] == 0).all())
    tie = pooled0[n - 1, 0, 0] > 0
    assert bool(tie.any()) and bool((idx0[n - 1, 0, 0][tie] == 0).all())
    assert 0.3 < float((out0 > 0).float().mean()) < 0.7
    for want_bits, want_pool in ((True, True), (True, False), (False, True)):
        out = torch.full_like(t2, float("nan"))
        bits = torch.full((P, c // 4), 0xff, device=DEV, dtype=torch.uint8) if want_bits else None
        pooled = torch.full_like(pooled0, float("nan")) if want_pool else None
        idx = torch.full_like(idx0, 0xff) if want_pool else None
        check(lib.runet_rb_out_ex(t2.data_ptr(), c, A.data_ptr(), B.data_ptr(), sa.data_ptr(), r.data_ptr(), c, _ptr(rs), _ptr(rh), out.data_ptr(), c,
                                  _ptr(bits), _ptr(pooled), c if want_pool else 0, _ptr(idx), n, h, w, c, st))
        same(out, out0, "out")
        if want_bits:
            same(bits, bits0, "relu_bits")
        if want_pool:
            same(pooled, pooled0, "pooled")
            same(idx, idx0, "pool_idx")


@pytest.mark.parametrize("n,h,w,c,pool", [s + (True,) for s in SHAPES] + [(1, 2, 2, 1024, False)])
def test_backward_edge(n, h, w, c, pool):
    lib, check = _lib()
    st = _st()
    t2, r, sa, A, B, _, _ = tail_inputs(n, h, w, c, seed=23 + c)
    g = torch.Generator().manual_seed(29 + c)
    out = torch.relu(torch.randn((n, h, w, c), generator=g)).to(DEV)
    dout = torch.randn((n, h, w, c), generator=g).to(DEV)
    dpool = torch.randn((n, h // 2, w // 2, c), generator=g).to(DEV)
    pidx = torch.randint(0, 4, (n, h // 2, w // 2, c), generator=g).to(torch.uint8).to(DEV)
    bits = pack_bits(out)
    P, hw = n * h * w, h * w
    g0 = dout.clone()
    if pool:
        check(lib.runet_maxpool2_bwd(dpool.data_ptr(), c, pidx.data_ptr(), g0.data_ptr(), c, n, h, w, c, 1, st))
    dv0, dq0 = torch.empty_like(dout), torch.empty(P, device=DEV)
    check(lib.runet_rb_bwd1(g0.data_ptr(), c, out.data_ptr(), c, t2.data_ptr(), c, A.data_ptr(), B.data_ptr(), sa.data_ptr(), dv0.data_ptr(), c,
                            dq0.data_ptr(), P, hw, c, st))
    assert float(dv0.abs().max()) > 0 and float(dq0.abs().max()) > 0
    keep = dout.clone()
    for use_bits in (True, False) if pool else (True,):
        dv, dq = torch.full_like(dout, float("nan")), torch.full((P,), float("nan"), device=DEV)
        check(lib.runet_rb_bwd1_ex(dout.data_ptr(), c, dpool.data_ptr() if pool else None, c if pool else 0, pidx.data_ptr() if pool else None,
                                   None if use_bits else out.data_ptr(), c, bits.data_ptr() if use_bits else None, t2.data_ptr(), c, A.data_ptr(),
                                   B.data_ptr(), sa.data_ptr(), dv.data_ptr(), c, dq.data_ptr(), n, h, w, c, st))
        same(dv, dv0, "dv")
        same(dq, dq0, "dq")
        same(dout, keep, "dout is left unmodified")


@pytest.mark.parametrize("n,h,w,c", [(2, 3, 5, 64), (1, 3, 5, 128), (1, 2, 2, 512)])
def test_rb_bwd3_with_the_shortcut_batchnorm(n, h, w, c):
    lib, check = _lib()
    st = _st()
    g = torch.Generator().manual_seed(31 + c)
    P, hw = n * h * w, h * w

    def rn(*shape, s=1.0):
        return (torch.randn(shape, generator=g) * s).to(DEV)
    dv, t2, r = rn(n, h, w, c), rn(n, h, w, c), rn(n, h, w, c)
    sa = torch.rand(P, generator=g).to(DEV)
    dsm = rn(P, 2)
    amax = torch.randint(0, c, (P,), generator=g, dtype=torch.int32).to(DEV)
    ca, davg, dmx = torch.rand((n, c), generator=g).to(DEV), rn(n, c), rn(n, c)
    idx = torch.randint(0, hw, (n, c), generator=g, dtype=torch.int32).to(DEV)
    mean2, s2, sums2 = rn(c, s=0.1), rn(c), rn(2 * c)
    invstd2 = (torch.rand(c, generator=g) + 0.5).to(DEV)
    mean_s, scale_s, sums_s = rn(c, s=0.1), rn(c), rn(2 * c)
    invstd_s = (torch.rand(c, generator=g) + 0.5).to(DEV)
    for use_s, m_total, m_s in ((sums_s, 0, 0), (sums_s, 3 * P, 5 * P), (torch.zeros(2 * c, device=DEV), 0, 0)):
        dt0 = torch.empty_like(dv)
        dr0 = dv.clone()
        check(lib.runet_rb_bwd3(dr0.data_ptr(), c, t2.data_ptr(), c, sa.data_ptr(), dsm.data_ptr(), amax.data_ptr(), ca.data_ptr(), davg.data_ptr(),
                                dmx.data_ptr(), idx.data_ptr(), mean2.data_ptr(), invstd2.data_ptr(), s2.data_ptr(), sums2.data_ptr(), dt0.data_ptr(), c,
                                P, hw, c, m_total, st))
        check(lib.runet_bn_bwd_apply(dr0.data_ptr(), c, r.data_ptr(), c, None, 0, dr0.data_ptr(), c, P, hw, c, mean_s.data_ptr(), invstd_s.data_ptr(),
                                     scale_s.data_ptr(), use_s.data_ptr(), None, m_s, None, st))
        dt, dr = torch.full_like(dv, float("nan")), dv.clone()
        check(lib.runet_rb_bwd3_sc(dr.data_ptr(), c, t2.data_ptr(), c, sa.data_ptr(), dsm.data_ptr(), amax.data_ptr(), ca.data_ptr(), davg.data_ptr(),
                                   dmx.data_ptr(), idx.data_ptr(), mean2.data_ptr(), invstd2.data_ptr(), s2.data_ptr(), sums2.data_ptr(), dt.data_ptr(), c,
                                   r.data_ptr(), c, mean_s.data_ptr(), invstd_s.data_ptr(), scale_s.data_ptr(), use_s.data_ptr(), m_s, P, hw, c, m_total,
                                   st))
        same(dt, dt0, "dt2")
        same(dr, dr0, "dr")
        assert not torch.equal(dr, dv)


@pytest.mark.parametrize("cin,cout", [(64, 128), (128, 128)])
def test_block_with_the_edges_on_and_off(monkeypatch, cin, cout):
    """One ResidualBlock forward + backward through blocks.rb_forward / rb_backward, pooled, train mode with a dropout mask."""
    M = importlib.import_module(PKG_NAME + ".model")
    blocks = importlib.import_module(PKG_NAME + ".blocks")
    torch.manual_seed(5)
    mod = M.ResidualBlock(cin, cout, dropout_rate=0.2).to(DEV)
    with torch.no_grad():
        for p in mod.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    mod.train()
    n, h, w = 2, 16, 16
    mask = (torch.bernoulli(torch.full((n, cout), 0.8)) / 0.8).to(DEV)
    x = torch.randn(n, h, w, cin, device=DEV)
    dout = torch.randn(n, h, w, cout, device=DEV)
    dpool = torch.randn(n, h // 2, w // 2, cout, device=DEV)
    state = copy.deepcopy(mod.state_dict())
    res = {}
    for on in (False, True):
        monkeypatch.setattr(blocks, "FUSED_RB_EDGES", on)
        mod.load_state_dict(state)
        out, ctx, pooled, pidx = blocks.rb_forward(x, mod.handles(), True, mask, pool=True)
        assert ctx["pool_idx"] is pidx and (ctx["relu_bits"] is not None) == on
        assert all(ctx[k] is not None for k in ("out", "amax", "idx"))
        sink = blocks.DictSink(DEV)
        keep = (out.clone(), pooled.clone(), pidx.clone())
        dx = blocks.rb_backward(ctx, dout.clone(), sink, dpool=dpool, pool_idx=pidx)
        torch.cuda.synchronize()
        res[on] = dict(out=keep[0], pooled=keep[1], pool_idx=keep[2], dx=dx.clone(), **{"grad " + k: v.clone() for k, v in sink.g.items()},
                       **{"buffer " + k: v.clone() for k, v in mod.named_buffers()})
    assert res[False].keys() == res[True].keys() and len(res[True]) > 12
    for k in res[False]:
        same(res[True][k], res[False][k], k)


def test_model_step_with_the_edges_on_and_off(monkeypatch, pkg, oracle):
    """One train step of RobustUNet(3, 1, 64) at 2 x 64^2: loss, every gradient and every BatchNorm buffer; tests/decisions.py's hip_step reads
    what the forward saves (pool winner bytes, out, amax, idx of every block) and must run with the edges fused."""
    blocks = importlib.import_module(PKG_NAME + ".blocks")
    decisions = importlib.import_module("decisions")
    n, size, base, seed = 2, 64, 64, 3
    torch.manual_seed(seed)
    model = pkg.RobustUNet(3, 1, base).to(DEV).train()
    model.set_dropout_masks(oracle.dropout_masks(n, base, seed=seed))
    x, y = pkg.synthetic_batch(n, size, seed=seed)
    x, y = x.to(DEV), y.to(DEV)
    state = copy.deepcopy(model.state_dict())
    res = {}
    for on in (False, True):
        monkeypatch.setattr(blocks, "FUSED_RB_EDGES", on)
        model.load_state_dict(state)
        for p in model.parameters():
            p.grad = None
        loss = pkg.bce_loss(model(x), y)
        loss.backward()
        torch.cuda.synchronize()
        res[on] = dict(loss=loss.detach().clone(), **{"grad " + k: p.grad.clone() for k, p in model.named_parameters()},
                       **{"buffer " + k: b.clone() for k, b in model.named_buffers()})
    for k in res[False]:
        same(res[True][k], res[False][k], k)
    assert blocks.FUSED_RB_EDGES
    model.load_state_dict(state)
    dec, prob, _ = decisions.hip_step(model, x, y)
    assert sorted(dec["pool"]) == [1, 2, 3, 4] and dec["pool"][1].shape == (n, base, size // 2, size // 2)
    assert int(dec["pool"][1].max()) <= 3 and torch.isfinite(prob).all()
