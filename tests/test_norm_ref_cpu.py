"""tests/norm_ref.py on the CPU: the reference the GPU tests of csrc/norm_act.hip and the pooling kernels of csrc/misc.hip compare with is
torch's own arithmetic, and its inputs (norm_ref.cases()) are such that a correct fp32 kernel must take the float64 reference's decisions.

  1. float64: coeffs / apply / backward / pooled_grad / maxpool / maxpool_scatter / maxunpool_gather / chan_sum equal F.batch_norm (training
     and eval) followed by relu x mask, leaky_relu, gelu or nothing, F.max_pool2d(return_indices=True), F.max_unpool2d and their autograd to
     1e-12 of each tensor's scale: values, dx, dgamma, dbeta and the running buffers, for every case.
  2. every case with a ReLU / LeakyReLU decision: min |z| >= 1e-4 max |z| outside the planted exact zeros (which are there, in a channel with
     shift = 0), one channel has a negative scale, and no pooling window has tied maxima other than exact zeros.  This is what lets the GPU test
     allow no differing decision at all.
  3. norm_ref.geom over cases() reaches every launch regime of today's chunking, each asserted by name.
  4. the fp32 floor: the reference in float32 against float64, per tensor, printed (pytest -s) - the figure the GPU test's tolerance rule
     refers to.  No kernel is involved.
"""
import pytest
import torch
import torch.nn.functional as F

import norm_ref as R

CASES = R.cases()


def of_kind(*kinds):
    return pytest.mark.parametrize("case", [c for c in CASES if c.kind in kinds], ids=lambda c: c.id)


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def _same(a, b, name):
    assert a.shape == b.shape, (name, tuple(a.shape), tuple(b.shape))
    a, b = a.detach(), b.detach()
    both_nan = torch.isnan(a) & torch.isnan(b)
    err = float(torch.where(both_nan, torch.zeros_like(a), a - b).abs().max())
    assert err <= 1e-12 * max(1.0, float(b[~torch.isnan(b)].abs().max())), (name, err)


def _winner_bytes(indices, w):
    """max_pool2d's flat input index h * W + w -> the byte k = (h & 1) * 2 + (w & 1)"""
    return ((((indices // w) & 1) * 2) + ((indices % w) & 1)).to(torch.uint8)


# ----------------------------------------------------------------------------- 1. the reference is torch's arithmetic
@of_kind("bn", "pooled")
def test_reference_is_torch_autograd(case):
    b = case.build()
    n, h, w, c = case.shape
    x64 = b.x.double()
    co = R.coeffs(x64, b.gamma, b.beta, b.running_mean, b.running_var, b.nbt, training=case.training)
    xt = nchw(x64).requires_grad_(True)
    gamma, beta = b.gamma.double().requires_grad_(True), b.beta.double().requires_grad_(True)
    rm, rv = b.running_mean.double().clone(), b.running_var.double().clone()
    zt = F.batch_norm(xt, rm, rv, gamma, beta, case.training, R.BN_MOMENTUM, R.BN_EPS)
    at = {None: lambda v: v, "relu": torch.relu, "leaky": lambda v: F.leaky_relu(v, R.SLOPE), "gelu": F.gelu}[case.act](zt)
    if b.mask_nc is not None:
        at = at * b.mask_nc.double()[:, :, None, None]
    mine_y = R.apply(x64, co.scale, co.shift, case.act, b.mask_nc)
    _same(mine_y, nhwc(at), "y")
    if case.kind == "pooled":
        pt, it = F.max_pool2d(at, 2, return_indices=True)
        pm, im = R.maxpool(mine_y)
        _same(pm, nhwc(pt), "pooled")
        assert torch.equal(im, nhwc(_winner_bytes(it, w))), "winner bytes"
        pt.backward(nchw(b.dpool.double()))
        g_in = R.pooled_grad(b.dpool.double(), im)
    else:
        at.backward(nchw(b.dy.double()))
        g_in = b.dy.double()
    # with the mask and no ReLU decision the kernels' backward does not apply the mask (blocks.enet_tail_backward puts it in front): there
    # the reference's g is dy, and torch's is dy * mask - compare through that
    if case.act is None and b.mask_nc is not None:
        g_in = g_in * b.mask_nc.double()[:, None, None, :]
    r = R.backward(g_in, x64, co.mean, co.invstd, co.scale, co.shift, case.act, b.mask_nc, training=case.training)
    _same(r.dx, nhwc(xt.grad), "dx")
    _same(r.sums[:c], gamma.grad, "dgamma")
    _same(r.sums[c:], beta.grad, "dbeta")
    _same(co.running_mean, rm, "running_mean")
    _same(co.running_var, rv, "running_var")
    assert co.nbt == b.nbt + (1 if case.training else 0)


@of_kind("pool")
def test_pool_reference_is_torch(case):
    b = case.build()
    n, h, w, c = case.shape
    xt = nchw(b.x.double()).requires_grad_(True)
    pt, it = F.max_pool2d(xt, 2, return_indices=True)
    pm, im = R.maxpool(b.x.double())
    _same(pm, nhwc(pt), "pooled")
    assert torch.equal(im, nhwc(_winner_bytes(it, w)))
    assert im[0, 0, 0, 0] == 0 and im[0, 0, 0, 1] == 1 and bool(torch.isnan(pm[n - 1, -1, -1, 3])) and im[n - 1, -1, -1, 3] == 1
    assert float(pm[0, 0, 0, 2]) < 0
    dpool = b.dpool.double()
    pt.backward(nchw(dpool))
    _same(R.maxpool_scatter(dpool, im), nhwc(xt.grad), "scatter")
    _same(R.maxpool_scatter(dpool, im, b.base.double()), nhwc(xt.grad) + b.base.double(), "scatter, accumulate")
    pin = nchw(dpool).requires_grad_(True)
    ut = F.max_unpool2d(pin, it, 2)
    _same(R.maxpool_scatter(dpool, im), nhwc(ut), "unpool forward")
    ut.backward(nchw(b.du.double()))
    _same(R.maxunpool_gather(b.du.double(), im), nhwc(pin.grad), "unpool gather")


@of_kind("chansum")
def test_chan_sum_reference(case):
    b = case.build()
    s, scale = R.chan_sum(b.x.double(), b.out0)
    _same(s, b.x.double().sum(dim=(0, 1, 2)) + b.out0.double(), "sum")
    assert scale >= float(s.abs().max()) - float(b.out0.abs().max())


# ----------------------------------------------------------------------------- 2. decision margins
@pytest.mark.parametrize("case", [c for c in CASES if c.decision], ids=lambda c: c.id)
def test_decision_margins(case):
    b = case.build()
    n, h, w, c = case.shape
    z = R.reference(case).z
    planted = torch.zeros(z.shape, dtype=torch.bool)
    planted.reshape(-1, c)[:, 0] = b.planted
    assert int(planted.sum()) >= 2 and float(b.shift[0]) == 0.0
    assert bool((z[planted] == 0).all()), "planted zeros give z exactly zero"
    signs = torch.signbit(b.x[planted])
    assert bool(signs.any()) and not bool(signs.all()), "+0.0 and -0.0"
    lo, hi = float(z[~planted].abs().min()), float(z.abs().max())
    print(case.id, f"min |z| / max |z| = {lo / hi:.2e}, positive share {float((z > 0).double().mean()):.2f}")
    assert lo >= R.MARGIN * hi, (lo, hi)
    assert c == 1 or (bool((b.scale < 0).any()) and bool((b.scale > 0).any())), "a channel with a negative scale beside positive ones"
    assert 0.05 < float((z > 0).double().mean()) < 0.95
    if case.kind == "pooled":
        a = R.activation(z, case.act)
        top = torch.stack(R._windows(a)).sort(dim=0, descending=True).values
        tied = (top[0] == top[1]) & (top[0] != 0)
        assert not bool(tied.any()), "tied pooling maxima other than exact zeros"


@pytest.mark.parametrize("case", [c for c in CASES if c.mask], ids=lambda c: c.id)
def test_masks_drop_planes(case):
    """Dropout2d(0.3) masks: dropped and kept planes, and from two channels on one channel dropped in every image (its BatchNorm-backward
    sums are zero, so dx there is a product with a zero: where the two ReLU forms of the backward once differed in the sign of that zero)"""
    m = case.build().mask_nc
    assert bool((m == 0).any()) and bool((m > 1).any()) and set(m.unique().tolist()) <= {0.0, float(torch.tensor(1.0 / 0.7, dtype=torch.float32))}
    assert case.shape[3] == 1 or bool((m == 0).all(dim=0).any())


def test_single_channel_cases_have_both_scale_signs():
    signs = [float(c.build().scale[0]) < 0 for c in CASES if c.decision and c.shape[3] == 1]
    assert any(signs) and not all(signs)


# ----------------------------------------------------------------------------- 3. regime coverage
def test_cases_reach_every_launch_regime():
    G = {c.id: (c, R.geom(c.shape[0], c.shape[1] * c.shape[2], c.shape[3])) for c in CASES if c.kind in ("bn", "pooled")}
    for cid, (c, g) in G.items():
        print(cid, {k: v for k, v in vars(g).items()})

    def some(name, pred, among=lambda c: c.kind == "bn"):
        hit = [cid for cid, (c, g) in G.items() if among(c) and pred(c, g)]
        assert hit, "no case reaches: " + name
        return hit
    hw = lambda c: c.shape[1] * c.shape[2]
    some("one reduce pass per thread row", lambda c, g: g.r_counts == {1})
    some("two reduce passes: the pair loop alone", lambda c, g: 2 in g.r_counts)
    some("three reduce passes: the pair loop, then the single-pixel tail", lambda c, g: 3 in g.r_counts)
    some("rows taking the pair loop beside rows taking the tail", lambda c, g: {1, 2} <= g.r_counts and g.rows == 256)
    some("idle threads", lambda c, g: g.idle > 0)
    some("one idle thread (rows = 85)", lambda c, g: g.rows == 85 and g.idle == 1)
    some("rows = 1 with idle threads", lambda c, g: g.rows == 1 and g.idle == 127)
    some("rows = 1, ppc = 1", lambda c, g: g.rows == 1 and g.r_ppc == 1 and g.idle == 0)
    some("fewer pixels than thread rows", lambda c, g: hw(c) < g.rows)
    some("one value per image", lambda c, g: hw(c) == 1)
    some("VEC = 1", lambda c, g: g.vec == 1)
    some("VEC = 1 with more than one reduce chunk", lambda c, g: g.vec == 1 and g.r_chunks > 1)
    some("VEC = 1 with 3 stream passes", lambda c, g: g.vec == 1 and g.s_passes == 3)
    some("VEC = 1 with 9 stream passes", lambda c, g: g.vec == 1 and g.s_passes == 9)
    some("nparts below 256", lambda c, g: g.nparts < 256)
    some("nparts at least 256: final width 4", lambda c, g: g.nparts >= 256 and g.final_cw == 4)
    some("final width below 32", lambda c, g: g.final_cw < 32 and g.nparts < 256 and c.shape[3] > 1)
    some("final kernel with c % 32 != 0 and several blocks", lambda c, g: c.shape[3] > 32 and c.shape[3] % g.final_cw != 0)
    some("a ragged last reduce chunk", lambda c, g: g.r_ragged and g.r_chunks > 1)
    some("a reduce chunk shorter than the thread rows (idle rows)", lambda c, g: g.r_chunks > 1 and g.r_ppc < g.rows)
    some("one stream pass", lambda c, g: g.s_passes == 1)
    some("several stream passes with a ragged last one", lambda c, g: g.s_passes >= 3 and g.s_ragged)
    some("five stream passes at rows = 85", lambda c, g: g.rows == 85 and g.s_passes == 5)
    some("several stream chunks per image", lambda c, g: g.s_chunks > 1)
    for act in ("relu", "leaky", "gelu"):      # every activation at c = 12, 64, 516, 1024 and 1, training and eval
        for ch in (12, 64, 516, 1024, 1):
            for training in (True, False):
                some(f"{act} c = {ch} training = {training}", lambda c, g: c.act == act and c.shape[3] == ch and c.training == training)
    for act in ("relu", "leaky"):
        some(f"pooled {act}: nparts >= 256", lambda c, g: c.act == act and g.nparts >= 256, among=lambda c: c.kind == "pooled")
        some(f"pooled {act}: rows = 1", lambda c, g: c.act == act and g.rows == 1, among=lambda c: c.kind == "pooled")
        some(f"pooled {act}: one window per image", lambda c, g: c.act == act and hw(c) == 4, among=lambda c: c.kind == "pooled")
    cs = [R.chan_sum_geom(c.shape[0] * c.shape[1] * c.shape[2], c.shape[3]) for c in CASES if c.kind == "chansum"]
    assert any(g.chunks == 1 for g in cs) and any(g.chunks > 1 for g in cs), "chan_sum: one chunk and several"


# ----------------------------------------------------------------------------- 4. the fp32 floor
@pytest.mark.parametrize("case", [c for c in CASES if c.kind != "pool"], ids=lambda c: c.id)
def test_fp32_floor(case):
    """Prints the floor; asserts only that float32 stays a float32 (1e-4 of scale: a wrong formula in one dtype's path would not)."""
    floor = R.fp32_floor(case)
    print("fp32 floor", case.id, " ".join(f"{k}={v:.1e}" for k, v in floor.items()))
    if case.cond:
        print("   dx by the kernels' form g sc + x ca + cb in float32:", f"{R.kernel_form_floor(case):.1e}")
    assert all(v <= 1e-4 for v in floor.values()), floor


def test_largest_floor():
    """the figure the GPU test's docstring quotes: the largest floor of any tensor of any case"""
    worst = max(((v, c.id, k) for c in CASES if c.kind != "pool" for k, v in R.fp32_floor(c).items()))
    print("largest fp32 floor:", worst)
    assert worst[0] <= 1e-4
