"""GPU: the kernels of csrc/attention.hip - channel attention, spatial attention, the ResidualBlock tail and the attention gate, forward and
backward - against tests/attention_ref.py in float64, at the shapes where their launch plans change and with negative BatchNorm gammas.

The inputs are attention_ref.cases(); tests/test_attention_ref_cpu.py shows on the CPU that the reference is the oracle's arithmetic and
that every arg-max of every case is decided by at least 2e-5 of its tensor's scale.

The tail and the gate are driven through the production path (blocks.rb_forward / rb_backward, blocks.gate_forward / gate_backward with the
strided concat views of upgate_forward), and the reference is evaluated on the kernels' OWN convolution outputs (ctx["t2"], ctx["r"], gc["g1"],
gc["x1"]) in float64, so no convolution rounding enters a comparison.

Decisions (the idiom of tests/decisions_seq.py):
  * the channel-attention pixel (idx) and the spatial-attention channel (amax) equal the reference's exactly;
  * a ReLU mask element or a pooling winner on which the kernel and the reference differ is a near-tie in the reference (|ReLU input|, or the
    gap between the two winners' values, at most 2e-5 of the tensor's scale), and at most 0.05 % of the elements differ;
  * the reference is then evaluated under the kernel's own ReLU mask and pooling winners, and nothing is left out of any comparison.

Tolerance: 1e-5 of each reference tensor's largest magnitude, for every tensor (the float32 floor that test_attention_ref_cpu.py prints is
at most 2.8e-6 for any of them, so no bound needed the 4 x floor rule).  The three convolution biases in front of a train-mode BatchNorm
(W_g.0.bias, W_x.0.bias, psi.0.bias) have an analytically zero gradient: their sums cancel to rounding level on both sides, so their error is
taken relative to the largest per-channel sum of the |terms| (attention_ref.gate_run), which is what bounds a sum's rounding error; in eval
mode they are ordinary tensors under the ordinary bound.

Every test prints its worst error per tensor (pytest -s).
"""
import importlib

import pytest
import torch

import attention_ref as R
from conftest import PKG_NAME
from decisions_seq import pool_flat_2x2

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TOL = 1e-5
NEAR_TIE = 2e-5
MAX_FLIPS = 5e-4
CASES = R.cases()


def _mods():
    return tuple(importlib.import_module(f"{PKG_NAME}.{m}") for m in ("model", "blocks", "ops"))


def of_kind(kind):
    return pytest.mark.parametrize("case", [c for c in CASES if c.kind == kind], ids=lambda c: c.id)


def nhwc_dev(t):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV)


def nchw(t):
    """NHWC device tensor -> NCHW on the CPU (float64 for floating types, int64 else)"""
    t = t.detach().cpu().permute(0, 3, 1, 2)
    return t.double() if t.is_floating_point() else t.long()


def logical(t):
    """a sink's physical gradient -> the parameter's logical shape (HWIO -> OIHW), on the CPU"""
    t = t.detach().cpu().double()
    return t.permute(3, 2, 0, 1) if t.dim() == 4 else t


def unpack_bits(bits, n, h, w, c):
    """relu_bits [n*h*w, c/4] (bit e of byte j: channel 4j + e) -> bool NCHW"""
    b = bits.cpu().to(torch.int32)
    on = torch.stack([(b >> e) & 1 for e in range(4)], dim=-1).reshape(n, h, w, c)
    return on.permute(0, 3, 1, 2) != 0


class Report:
    """collects (tensor, error / scale) rows, prints them, and fails at the end if any exceeds its bound"""

    def __init__(self, title):
        self.title, self.rows, self.bad = title, [], []

    def close(self, name, got, ref, scale=None, tol=TOL):
        got, ref = got.detach().cpu().double(), ref.detach().double()
        assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
        assert bool(torch.isfinite(got).all()), name
        err = R.rel_err(got, ref, scale)
        self.rows.append((name, err))
        if not err <= tol:
            self.bad.append(f"{name}: {err:.2e} of scale > {tol:.0e}")

    def equal(self, name, got, ref):
        got, ref = got.detach().cpu().long(), ref.detach().long()
        assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
        ndiff = int((got != ref).sum())
        self.rows.append((name + " (exact)", float(ndiff)))
        if ndiff:
            self.bad.append(f"{name}: {ndiff} of {ref.numel()} differ")

    def decisions(self, name, differ, margin, scale):
        """differ: bool tensor of the decisions on which the kernel and the reference disagree; margin: how far the reference is from a tie there"""
        share = float(differ.double().mean())
        worst = float(margin[differ].max()) / scale if bool(differ.any()) else 0.0
        self.rows.append((f"{name} flipped share", share))
        self.rows.append((f"{name} worst flipped margin", worst))
        if share > MAX_FLIPS:
            self.bad.append(f"{name}: {share:.2e} of the decisions differ > {MAX_FLIPS:.0e}")
        if worst > NEAR_TIE:
            self.bad.append(f"{name}: differs where the reference is {worst:.2e} of scale from a tie > {NEAR_TIE:.0e}")

    def done(self):
        print(f"\n{self.title}: " + "  ".join(f"{k}={v:.1e}" for k, v in self.rows))
        assert not self.bad, self.bad


# ----------------------------------------------------------------------------- standalone attentions
@of_kind("ca")
def test_channel_attention(case, monkeypatch):
    """model.ChannelAttention: Cr = 1 (C = 16), 3 (C = 48, one thread of ca_hidden idle and rows of rb_bwd2 / rb_bwd3 with idle threads),
    64 (C = 1024, rows == 1); 2 x 20 x 36 x 48 is more than one chunk per image.  tie: two pixels hold the maximum of every fourth channel."""
    M, blocks, _ = _mods()
    b = case.build()
    n, h, w, c = case.shape
    saved = {}
    real = blocks.ca_forward

    def spy(*a, **k):
        y, ctx = real(*a, **k)
        saved.update(ctx)
        return y, ctx
    monkeypatch.setattr(blocks, "ca_forward", spy)
    mod = M.ChannelAttention(c)
    mod.load_state_dict(b.P, strict=True)
    mod.to(DEV)
    x = b.x.to(DEV).requires_grad_(True)
    y = mod(x)
    y.backward(b.dy.to(DEV))
    torch.cuda.synchronize()
    ref, g = R.ca_run(b.x, b.P, b.dy)
    rep = Report(case.id)
    rep.equal("idx", saved["idx"].view(n, c), ref.idx)
    if case.tie:
        assert bool((saved["idx"].view(n, c).cpu()[:, b.ties] == h * w // 3).all()), "the first of two equal maxima must win"
    for k in ("avg", "mx", "ca"):
        rep.close(k, saved[k].view(n, c), getattr(ref, k))
    rep.close("y", y, ref.y)
    rep.close("dx", x.grad, g["dx"])
    rep.close("fc.0.weight", mod.fc[0].weight.grad, g["fc.0.weight"])
    rep.close("fc.2.weight", mod.fc[2].weight.grad, g["fc.2.weight"])
    rep.done()


@of_kind("sa")
def test_spatial_attention(case, monkeypatch):
    """model.SpatialAttention: images smaller than the 7 x 7 window (5 x 7, 6 x 3), partial 16 x 16 tiles and several tiles whose weight-gradient
    partials reduce_rows sums (20 x 36, 17 x 33), C < 64 (lanes of the 16 per pixel that hold no channel: C = 4, 16, 32), C = 128 (two
    steps).  tie: two channels, in different lanes, hold the maximum at every third pixel."""
    M, blocks, _ = _mods()
    b = case.build()
    n, h, w, c = case.shape
    saved = {}
    real = blocks.sa_forward

    def spy(*a, **k):
        y, ctx = real(*a, **k)
        saved.update(ctx)
        return y, ctx
    monkeypatch.setattr(blocks, "sa_forward", spy)
    mod = M.SpatialAttention()
    mod.load_state_dict(b.P, strict=True)
    mod.to(DEV)
    x = b.x.to(DEV).requires_grad_(True)
    y = mod(x)
    y.backward(b.dy.to(DEV))
    torch.cuda.synchronize()
    ref, g = R.sa_run(b.x, b.P, b.dy)
    rep = Report(case.id)
    rep.equal("amax", saved["amax"].view(n, h, w), ref.amax)
    if case.tie:
        assert bool((saved["amax"].cpu()[b.ties] == c // 4).all()), "the first of two equal maxima must win"
    rep.close("smap", nchw(saved["smap"].view(n, h, w, 2)), ref.smap)
    rep.close("sa", saved["sa"].view(n, 1, h, w), ref.sa)
    rep.close("y", y, ref.y)
    rep.close("dx", x.grad, g["dx"])
    rep.close("conv1.weight", mod.conv1.weight.grad, g["conv1.weight"])
    rep.done()


# ----------------------------------------------------------------------------- ResidualBlock tail
@of_kind("tail")
def test_residual_block_tail(case, monkeypatch):
    """blocks.rb_forward / rb_backward.  Reached here and by no earlier test: negative bn2 / shortcut gammas (ca_coeff's s < 0 branch: the
    channel maximum from min_nc / imin_nc, through idx / tval into ca_bwd and rb_bwd3); Cr = 1 (C = 16), 3 (C = 48), 64 (C = 1024); idle
    threads in a row group (C = 48) and rows == 1 (C = 1024); more than one chunk per image (2 x 20 x 36 x 64: HW * C = 46080); images
    smaller than the 7 x 7 window (6 x 10, 2 x 2, 4 x 4) and partial 16 x 16 tiles (20 x 36); C < 64 in the 16-lane kernels."""
    M, blocks, ops = _mods()
    b = case.build()
    n, h, w, cin, c = case.shape
    tr = case.training
    if case.switch:
        monkeypatch.setattr(blocks, *case.switch)
    mod = M.ResidualBlock(cin, c, dropout_rate=0.2)
    mod.load_state_dict(b.P, strict=True)
    mod.to(DEV).train(tr)
    x = nhwc_dev(b.x)
    res = blocks.rb_forward(x, mod.handles(), tr, b.mask.to(DEV) if tr else None, pool=case.pool)
    out, ctx = res[0], res[1]
    pooled, pidx = (res[2], res[3]) if case.pool else (None, None)
    edges = blocks.FUSED_RB_EDGES
    assert (ctx["relu_bits"] is not None) == edges

    seen = {}
    real_dgrad, real_wgrad = ops.conv_dgrad, ops.conv_wgrad

    def dgrad_spy(dy, *a, **k):
        seen.setdefault("dt2", dy.clone())
        return real_dgrad(dy, *a, **k)

    def wgrad_spy(x_, dy, kh, kw, *a, **k):
        if kh == 1:
            seen.setdefault("dr", dy.clone())
        return real_wgrad(x_, dy, kh, kw, *a, **k)
    monkeypatch.setattr(ops, "conv_dgrad", dgrad_spy)
    monkeypatch.setattr(ops, "conv_wgrad", wgrad_spy)
    dout = nhwc_dev(b.dout)
    dpool = nhwc_dev(b.dpool) if case.pool else None
    keep_out = out.clone()
    sink = blocks.DictSink(DEV)
    blocks.rb_backward(ctx, dout.clone(), sink, dpool=dpool, pool_idx=pidx)
    torch.cuda.synchronize()

    # ---- reference on the kernels' own convolution outputs
    t2, r = nchw(ctx["t2"]), nchw(ctx["r"])
    hip_out = nchw(keep_out)
    hip_mask = hip_out > 0
    if edges:
        assert torch.equal(unpack_bits(ctx["relu_bits"], n, h, w, c), hip_mask), "relu_bits are the signs of the values stored to `out`"
    hip_flat = pool_flat_2x2(nchw(pidx), w) if case.pool else None
    free, _ = R.tail_run(t2, r, b.P, tr, b.dout, b.dpool)                                    # the reference's own decisions
    ref, g = R.tail_run(t2, r, b.P, tr, b.dout, b.dpool, hip_flat, hip_mask)                 # ... and under the kernel's
    rep = Report(case.id)
    rep.equal("idx", ctx["idx"].view(n, c), ref.idx)
    rep.equal("amax", ctx["amax"].view(n, h, w), ref.amax)
    pre = free.pre.detach()
    rep.decisions("relu", hip_mask != (pre > 0), pre.abs(), float(pre.abs().max()))
    if case.pool:
        fo = free.out.detach().reshape(n, c, h * w)
        gap = torch.gather(fo, 2, free.pool_flat.reshape(n, c, -1)) - torch.gather(fo, 2, hip_flat.reshape(n, c, -1))
        rep.decisions("pool", (hip_flat != free.pool_flat).reshape(n, c, -1), gap, float(fo.abs().max()))
        assert int(pidx.max()) <= 3
        rep.close("pooled", nchw(pooled), ref.pooled)
    for k in ("s2", "h2", "mean2", "invstd2"):
        rep.close(k, ctx[k], getattr(ref, k))
    for k in ("avg", "mx", "tval", "ca", "A", "B"):
        rep.close(k, ctx[k].view(n, c), getattr(ref, k))
    rep.close("smap", nchw(ctx["smap"].view(n, h, w, 2)), ref.smap)
    rep.close("sa", ctx["sa"].view(n, 1, h, w), ref.sa)
    rep.close("out", hip_out, ref.out)
    assert bool((ref.s2 < 0).any()) and bool((ref.s2 > 0).any()), "the case is about both branches of ca_coeff"
    # ---- backward
    for k in R.TAIL_GRADS:
        if k in g:
            rep.close("grad " + k, logical(sink.g[k]), g[k])
    rep.close("dt2", nchw(seen["dt2"]), g["dt2"])
    if cin != c:
        rep.close("dr", nchw(seen["dr"]), g["dr"])
    rep.done()


# ----------------------------------------------------------------------------- attention gate
@of_kind("gate")
def test_attention_gate(case, monkeypatch):
    """blocks.gate_forward / gate_backward on the two halves of one [n, h, w, 2c] buffer (pixel stride 2c for `up`, `att_out`, `datt`, `dup`),
    negative W_g.1 / W_x.1 / psi.1 gammas; F = 8 and 12 (lanes of ag_psi without a channel, row groups of ag_bwd2 with idle threads),
    F = 256 (rows == 4), several chunks (2 x 20 x 36 x 64)."""
    M, blocks, ops = _mods()
    b = case.build()
    n, h, w, c, f = case.shape
    tr = case.training
    if case.switch:
        monkeypatch.setattr(blocks, *case.switch)
    mod = M.AttentionGate(c, c, f)
    mod.load_state_dict(b.P, strict=True)
    mod.to(DEV).train(tr)
    p = mod.handles()
    cat = torch.full((n, h, w, 2 * c), float("nan"), device=DEV)
    cat[..., c:] = nhwc_dev(b.up)
    up, att_out = cat[..., c:], cat[..., :c]
    skip = nhwc_dev(b.skip)
    gc = blocks.gate_forward(up, skip, p, tr, att_out, blocks.Small(DEV))

    seen = {"d1x1": []}
    real_wgrad, real_apply, real_bwd = ops.conv_wgrad, blocks.bn_bwd_apply, blocks.bn_backward

    def wgrad_spy(x_, dy, kh, kw, *a, **k):
        seen["d1x1"].append(dy.clone())
        return real_wgrad(x_, dy, kh, kw, *a, **k)

    def apply_spy(dy, xx, *a, **k):
        if xx is gc["g1"]:          # the first BatchNorm backward over dpre = ds * wpsi * [pre > 0], fresh from ag_bwd2
            seen.setdefault("mask", (dy != 0).clone())
        return real_apply(dy, xx, *a, **k)

    def bwd_spy(dy, xx, *a, **k):
        if xx is gc["g1"]:
            seen.setdefault("mask", (dy != 0).clone())
        return real_bwd(dy, xx, *a, **k)
    monkeypatch.setattr(ops, "conv_wgrad", wgrad_spy)
    monkeypatch.setattr(blocks, "bn_bwd_apply", apply_spy)
    monkeypatch.setattr(blocks, "bn_backward", bwd_spy)
    dcat = nhwc_dev(b.dcat)
    dcat0 = dcat.clone()
    cat0 = cat.clone()
    sink = blocks.DictSink(DEV)
    blocks.gate_backward(gc, up, skip, p, dcat[..., :c], dcat[..., c:], sink)
    torch.cuda.synchronize()
    assert torch.equal(cat, cat0) and torch.equal(dcat[..., :c], dcat0[..., :c]), "the backward pass reads cat and datt"
    assert torch.equal(cat[..., c:], nhwc_dev(b.up)), "the `up` half of the buffer is the caller's"
    assert len(seen["d1x1"]) == 2

    g1, x1 = nchw(gc["g1"]), nchw(gc["x1"])
    datt = b.dcat[:, :c]
    hip_mask = nchw(seen["mask"].to(torch.uint8)) != 0
    free, _ = R.gate_run(g1, x1, b.skip, b.P, tr, datt)
    ref, g = R.gate_run(g1, x1, b.skip, b.P, tr, datt, hip_mask)
    rep = Report(case.id)
    pre = free.pre.detach()
    rep.decisions("relu", hip_mask != (pre > 0), pre.abs(), float(pre.abs().max()))
    rep.close("s", nchw(gc["s"]), ref.s)
    for k in R.GATE_FWD[1:-1]:
        rep.close(k, gc[k], getattr(ref, k))
    rep.close("att", nchw(cat[..., :c]), ref.att)
    signs = torch.cat([ref.sg, ref.sx]).detach()
    assert bool((signs < 0).any()) and bool((signs > 0).any())
    for k in R.GATE_GRADS + ("W_g.0.bias", "W_x.0.bias"):
        rep.close("grad " + k, logical(sink.g[k]), g[k], scale=ref.cancel.get(k))
    rep.close("dg1", nchw(seen["d1x1"][0]), g["dg1"])
    rep.close("dx1", nchw(seen["d1x1"][1]), g["dx1"])
    rep.done()
