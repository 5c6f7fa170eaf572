"""GPU: the shared BatchNorm / activation / 2x2 pooling kernels of csrc/norm_act.hip and csrc/misc.hip - runet_bn_apply, runet_bn_bwd_reduce,
runet_bn_bwd_apply, their LeakyReLU, GELU and pooled instances, runet_chan_sum, runet_maxpool2_fwd / _bwd, runet_maxunpool2_bwd - against
tests/norm_ref.py in float64, at the shapes where their launch plans change.  These kernels are the yardstick of every "fused == composition"
test of the suite; this file measures the yardstick.

The inputs are norm_ref.cases(); tests/test_norm_ref_cpu.py shows on the CPU that the reference is torch's own arithmetic, that every
activation decision of every case is at least 1e-4 of max |z| from zero (except the planted exact zeros, where z > 0 must be false) and that
the cases reach every launch regime.  The kernels are driven through the production wrappers (blocks.bn_apply / bn_backward / ..., which take
pixel strides from ops.ld), dense and as channel slices of wider buffers with a different stride for every operand.

Kernel-level cases hand scale, shift, mean, invstd to the kernel and to the reference, so with the margin above NO decision may differ and
nothing is left out of any comparison.

Tolerance: every float tensor within max(1e-5, 4 x floor) of the reference tensor's largest magnitude, the floor being the error of the
reference's own float32 restatement against float64 for that case and tensor (norm_ref.fp32_floor, printed by test_norm_ref_cpu.py; never
the kernels' output).  The floors on record: at most 2.5e-6 for every tensor of every kernel-level case (largest: y of the mean / std = 100
case, 1.5e-6), so their bound is the flat 1e-5; the end-to-end y of the mean / std = 100 cases has a floor of 4.2e-6 at 3 x 5 x 7 x 12 and
3.4e-6 at 16 x 40 x 40 x 36 (x scale + shift cancels two numbers 100 times the result), hence bounds of 1.7e-5 and 1.4e-5 there; every other
end-to-end floor is below 2.5e-6.  dx by the kernels' form g sc + x ca + cb, restated in float32, is 3.0e-7 / 1.0e-7 off at mean / std = 100.
The (dgamma | dbeta) sums and runet_chan_sum are taken relative to the largest per-channel sum of the |terms|, which is what bounds a sum's
rounding error.

Exact results are compared as bits: pool values and winner bytes (ties, an all-negative window, a NaN), the scatter with and without
accumulation, the unpool gather, the bytes of a wide buffer outside the slice, in-place against out-of-place, act against relu_shift, sliced
against dense.

What these tests found: with a Dropout2d mask, the saved-activation form (act) and the recomputing form (relu_shift) of the backward differed
in the sign of a zero - g = +0 against dy * 0 = +-0 in a dropped plane, which reaches dx where a channel is dropped in every image of the
batch (zero sums, so dx = g * scale + 0).  The recomputing form (and runet_wino4_input_bn_bwd, its bit-identical partner) now takes the
ReLU-off branch in a dropped plane; "act form" below compares all bits.

Every test prints its worst error per tensor (pytest -s).
"""
import importlib
from types import SimpleNamespace as NS

import pytest
import torch
import torch.nn.functional as F

import norm_ref as R
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TOL = 1e-5
SENT = -7777.25
CASES = R.cases()


def _mods():
    return tuple(importlib.import_module(f"{PKG_NAME}.{m}") for m in ("blocks", "ops", "segformer", "_lib"))


def of_kind(kind, keep=lambda c: True):
    return pytest.mark.parametrize("case", [c for c in CASES if c.kind == kind and keep(c)], ids=lambda c: c.id)


def dev(t):
    return None if t is None else t.to(DEV)


def bound(case, name):
    """max(1e-5, 4 x the float32 floor of this case and tensor)"""
    return max(TOL, 4.0 * R.fp32_floor(case).get(name, 0.0))


def wide(t, ld, off, shape=None):
    """-> (a [n, h, w, ld] buffer full of the sentinel, its channel slice [off : off + c] holding t)"""
    n, h, w, c = shape if shape is not None else t.shape
    buf = torch.full((n, h, w, ld), SENT, device=DEV, dtype=torch.float32)
    view = buf[..., off:off + c]
    if t is not None:
        view.copy_(t)
    return buf, view


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


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
            self.bad.append(f"{name}: {err:.2e} of scale > {tol:.1e}")

    def bits(self, name, got, ref):
        """every bit equal (float32 as int32, so NaN == NaN and -0.0 != +0.0)"""
        assert got.shape == ref.shape and got.dtype == ref.dtype, (name, tuple(got.shape), tuple(ref.shape), got.dtype, ref.dtype)
        ndiff = int((_bits(got).cpu() != _bits(ref).cpu()).sum())
        self.rows.append((name + " (bits)", float(ndiff)))
        if ndiff:
            self.bad.append(f"{name}: {ndiff} of {ref.numel()} differ")

    def untouched(self, name, buf, off, c):
        """the bytes of a wide buffer outside its slice still hold the sentinel"""
        outside = torch.cat([buf[..., :off], buf[..., off + c:]], dim=-1)
        self.bits(name + " outside the slice", outside, torch.full_like(outside, SENT))

    def done(self):
        print(f"\n{self.title}: " + "  ".join(f"{k}={v:.1e}" for k, v in self.rows))
        assert not self.bad, self.bad


def _lds(c):
    """a pixel stride and channel offset of its own for every operand (multiples of 4)"""
    return {"x": (c + 8, 4), "dy": (c + 12, 8), "act": (c + 4, 0), "dx": (c + 16, 12), "y": (c + 20, 8), "dpool": (c + 8, 0)}


class Run:
    """one "bn" / "pooled" case on the device: the wrappers behind one call signature"""

    def __init__(self, case):
        self.B, self.ops, self.sf, L = _mods()
        self.lib, self.check = L.lib, L.check
        self.case, self.b, self.ref = case, case.build(), R.reference(case)
        b = self.b
        self.c = case.shape[3]
        self.x, self.scale, self.shift, self.mean, self.invstd, self.mask = (dev(v) for v in (b.x, b.scale, b.shift, b.mean, b.invstd, b.mask_nc))

    def st(self):
        return self.ops.stream()

    def apply(self, xv, out=None):
        a, B = self.case.act, self.B
        if a == "leaky":
            return B.bn_apply_leaky(xv, self.scale, self.shift, R.SLOPE, out=out)
        if a == "gelu":
            if out is None:
                return self.sf.bn_apply_gelu(xv, self.scale, self.shift)
            n, h, w, c = xv.shape      # the wrapper has no `out`: the entry point itself
            self.check(self.lib.runet_bn_apply_gelu(xv.data_ptr(), self.ops.ld(xv), out.data_ptr(), self.ops.ld(out), n * h * w, h * w, c,
                                                    self.scale.data_ptr(), self.shift.data_ptr(), self.st()))
            return out
        return B.bn_apply(xv, self.scale, self.shift, mask=self.mask, relu=a == "relu", out=out)

    def backward(self, dyv, xv, out=None, act=None, sync=None):
        """-> (dx, sums).  act: the saved activation (ReLU cases; default: the relu_shift form)"""
        a, B, t = self.case.act, self.B, self.case.training
        sums = torch.full((2 * self.c,), float("nan"), device=DEV)
        if a == "leaky":
            dx = B.bn_backward_leaky(dyv, xv, self.mean, self.invstd, self.scale, sums, self.shift, R.SLOPE, training=t, out=out)
        elif a == "gelu":
            if out is None:
                dx = self.sf.bn_backward_gelu(dyv, xv, self.mean, self.invstd, self.scale, sums, self.shift, training=t)
            else:
                dx = self._gelu_into(dyv, xv, out, sums)
        else:
            kw = {}
            if a == "relu":
                kw = dict(act=act) if act is not None else dict(relu_shift=self.shift)
            dx = B.bn_backward(dyv, xv, self.mean, self.invstd, self.scale, sums, mask=self.mask, out=out, sync=sync, training=t, **kw)
        return dx, sums

    def _gelu_into(self, dyv, xv, out, sums):
        """segformer.bn_backward_gelu with a destination (the wrapper has none)"""
        n, h, w, c = xv.shape
        hw, ld, p = h * w, self.ops.ld, lambda v: v.data_ptr()
        self.check(self.lib.runet_bn_bwd_reduce_gelu(p(dyv), ld(dyv), p(xv), ld(xv), n, hw, c, p(self.mean), p(self.invstd),
                                                     p(self.B._ws(n, hw, c, xv.device)), p(sums), p(self.scale), p(self.shift), self.st()))
        use = sums if self.case.training else self.B.zeros(2 * c, xv.device)
        self.check(self.lib.runet_bn_bwd_apply_gelu(p(dyv), ld(dyv), p(xv), ld(xv), p(out), ld(out), n * hw, hw, c, p(self.mean), p(self.invstd),
                                                    p(self.scale), p(use), 0, p(self.shift), self.st()))
        return out

    def pooled(self, dpv, idx, xv):
        B, t = self.B, self.case.training
        sums = torch.full((2 * self.c,), float("nan"), device=DEV)
        if self.case.act == "leaky":
            dx = B.bn_backward_pooled_leaky(dpv, idx, xv, self.mean, self.invstd, self.scale, sums, self.shift, R.SLOPE, training=t)
        else:
            dx = B.bn_backward_pooled(dpv, idx, xv, self.mean, self.invstd, self.scale, sums, self.shift, training=t)
        return dx, sums

    def against_reference(self, rep, tag, dx, sums):
        c, ref, case = self.c, self.ref, self.case
        rep.close(tag + "dx", dx, ref.dx, tol=bound(case, "dx"))
        rep.close(tag + "dgamma", sums[:c], ref.sums[:c], ref.sum_scale[0], tol=bound(case, "dgamma"))
        rep.close(tag + "dbeta", sums[c:], ref.sums[c:], ref.sum_scale[1], tol=bound(case, "dbeta"))


# ----------------------------------------------------------------------------- forward
@of_kind("bn")
def test_bn_apply(case):
    """relu {0, 1} x mask {none, given}, LeakyReLU, GELU: dense, and x / y as slices of wider buffers with their own strides; the wide
    output's bytes outside the slice stay.  No decision differs from the reference's: y > 0 exactly where the reference's y > 0, and the
    planted z == 0 elements give 0 (ReLU) / 0 * slope (LeakyReLU)."""
    r = Run(case)
    c, ld = r.c, _lds(r.c)
    rep = Report(case.id)
    y = r.apply(r.x)
    rep.close("y", y, r.ref.y, tol=bound(case, "y"))
    if case.decision:
        rep.bits("decisions", y.cpu() > 0, r.ref.y > 0)
        planted = y.cpu().reshape(-1, c)[:, 0][r.b.planted]
        assert planted.numel() >= 2 and bool((planted == 0).all()), "z == 0 is not > 0"
    _, xv = wide(r.x, *ld["x"])
    ybuf, yv = wide(None, *ld["y"], shape=case.shape)
    r.apply(xv, out=yv)
    rep.bits("sliced y", yv, y)
    rep.untouched("y", ybuf, ld["y"][1], c)
    rep.done()


# ----------------------------------------------------------------------------- backward
@of_kind("bn")
def test_bn_backward(case):
    """runet_bn_bwd_reduce + runet_bn_bwd_apply (and the LeakyReLU / GELU instances) against the reference: training (M = pixels) or eval
    (zero sums into apply).  Then, each to the bits of the dense out-of-place run: dy, x, act, dx as slices with a stride each; in place
    (out = dy, as production calls it); the saved-activation form against the relu_shift form.  SyncBN form (training): the sums entering
    apply are twice the local ones with m_total = twice the pixels - the reference is dx of the batch duplicated, which is dx."""
    r = Run(case)
    c, ld, b = r.c, _lds(r.c), r.b
    rep = Report(case.id)
    dy = dev(b.dy)
    dx, sums = r.backward(dy, r.x)
    r.against_reference(rep, "", dx, sums)

    _, dyv = wide(dy, *ld["dy"])
    _, xv = wide(r.x, *ld["x"])
    dxbuf, dxv = wide(None, *ld["dx"], shape=case.shape)
    dx_s, sums_s = r.backward(dyv, xv, out=dxv)
    rep.bits("sliced dx", dx_s, dx)
    rep.bits("sliced sums", sums_s, sums)
    rep.untouched("dx", dxbuf, ld["dx"][1], c)

    g = dy.clone()
    dx_i, sums_i = r.backward(g, r.x, out=g)
    rep.bits("in-place dx", dx_i, dx)
    rep.bits("in-place sums", sums_i, sums)
    gbuf, gv = wide(dy, *ld["dy"])
    dx_i, _ = r.backward(gv, xv, out=gv)
    rep.bits("in-place sliced dx", dx_i, dx)
    rep.untouched("in-place dx", gbuf, ld["dy"][1], c)

    if case.act == "relu":
        act = r.apply(r.x)
        dx_a, sums_a = r.backward(dy, r.x, act=act)
        rep.bits("act form dx", dx_a, dx)
        rep.bits("act form sums", sums_a, sums)
        _, av = wide(act, *ld["act"])
        dx_a, sums_a = r.backward(dyv, xv, out=dxv, act=av)
        rep.bits("act form, sliced, dx", dx_a, dx)
        rep.bits("act form, sliced, sums", sums_a, sums)

    if case.training and case.act in (None, "relu"):
        sync = NS(reduce_sums=lambda s, m: (s * 2.0, 2 * m))
        dx_y, sums_y = r.backward(dy, r.x, sync=sync)
        rep.close("SyncBN dx", dx_y, r.ref.dx, tol=bound(case, "dx"))
        rep.bits("SyncBN local sums", sums_y, sums)
    rep.done()


@of_kind("pooled")
def test_bn_backward_pooled(case):
    """The pooled forms: the full-resolution gradient is rebuilt from (dpool, idx) in registers.  idx is the reference pool of the reference
    activation (exact: margins, untied maxima); dpool and x are slices with their own strides.  Also to the bits of the two-launch path."""
    r = Run(case)
    c, ld, b = r.c, _lds(r.c), r.b
    rep = Report(case.id)
    dpool, idx = dev(b.dpool), dev(b.idx).contiguous()
    dx, sums = r.pooled(dpool, idx, r.x)
    r.against_reference(rep, "", dx, sums)
    _, dpv = wide(dpool, *ld["dpool"])
    _, xv = wide(r.x, *ld["x"])
    dx_s, sums_s = r.pooled(dpv, idx, xv)
    rep.bits("sliced dx", dx_s, dx)
    rep.bits("sliced sums", sums_s, sums)
    full = r.B.maxpool_backward(dpv, idx)
    rep.bits("scattered gradient", full, r.ref.g_in.float())
    dx_2, sums_2 = r.backward(full, r.x)
    rep.bits("two-launch dx", dx_2, dx)
    rep.bits("two-launch sums", sums_2, sums)
    rep.done()


# ----------------------------------------------------------------------------- pooling
@of_kind("pool")
def test_pool_scatter_gather(case):
    """runet_maxpool2_fwd / _bwd (accumulate 0 and 1) / runet_maxunpool2_bwd move values and compare them: every result is exact.  The
    input holds a window of four equal values, one with two equal maxima (k = 1 before k = 2), an all-negative one and a NaN."""
    B, ops, _, _ = _mods()
    b = case.build()
    n, h, w, c = case.shape
    ld = _lds(c)
    rep = Report(case.id)
    pool_ref, idx_ref = R.maxpool(b.x)
    x = dev(b.x)
    y, idx = B.maxpool_forward(x)
    rep.bits("pooled", y, pool_ref)
    rep.bits("winner bytes", idx, idx_ref)
    _, xv = wide(x, *ld["x"])
    y_s, idx_s = B.maxpool_forward(xv)
    rep.bits("pooled, sliced input", y_s, pool_ref)
    rep.bits("winner bytes, sliced input", idx_s, idx_ref)
    assert int(idx_ref[0, 0, 0, 0]) == 0 and int(idx_ref[0, 0, 0, 1]) == 1 and int(idx_ref[n - 1, -1, -1, 3]) == 1
    assert bool(torch.isnan(pool_ref[n - 1, -1, -1, 3])) and float(pool_ref[0, 0, 0, 2]) < 0

    _, dpv = wide(dev(b.dpool), *ld["dpool"])
    rep.bits("scatter", B.maxpool_backward(dpv, idx), R.maxpool_scatter(b.dpool, idx_ref))
    rep.bits("unpool forward", B.maxunpool_forward(dpv, idx), R.maxpool_scatter(b.dpool, idx_ref))
    gbuf, gv = wide(dev(b.base), *ld["dx"])
    B.maxpool_backward(dpv, idx, dx=gv)
    rep.bits("scatter, accumulate", gv, R.maxpool_scatter(b.dpool, idx_ref, b.base))
    rep.untouched("accumulated dx", gbuf, ld["dx"][1], c)
    _, duv = wide(dev(b.du), *ld["dy"])
    rep.bits("unpool gather", B.maxunpool_backward(duv, idx), R.maxunpool_gather(b.du, idx_ref))
    rep.done()


# ----------------------------------------------------------------------------- channel sums
@of_kind("chansum")
def test_chan_sum(case):
    """accumulate = 0 (blocks.chan_sum) and 1 (the entry point: no wrapper passes it), on a channel slice"""
    B, ops, _, L = _mods()
    b = case.build()
    n, h, w, c = case.shape
    rep = Report(case.id)
    _, xv = wide(dev(b.x), *_lds(c)["x"])
    s_ref, scale = R.chan_sum(b.x.double())
    out = torch.full((c,), float("nan"), device=DEV)
    B.chan_sum(xv, out)
    rep.close("sum", out, s_ref, scale, tol=bound(case, "sum"))
    acc = dev(b.out0).clone()
    L.check(L.lib.runet_chan_sum(xv.data_ptr(), ops.ld(xv), n * h * w, c, B._ws(n, h * w, c, DEV).data_ptr(), acc.data_ptr(), 1, ops.stream()))
    rep.close("sum, accumulate", acc, R.chan_sum(b.x.double(), b.out0)[0], scale + float(b.out0.abs().max()), tol=bound(case, "sum"))
    rep.done()


# ----------------------------------------------------------------------------- end to end: statistics -> coefficients -> apply -> backward
E2E_SHAPES = ((3, 5, 7, 12), (2, 3, 5, 1024), (3, 20, 28, 1))
E2E = [c for c in CASES if c.kind == "bn" and c.act is None and not c.mask and c.training and (c.cond or c.shape in E2E_SHAPES)]
E2E_EVAL = [c for c in CASES if c.kind == "bn" and c.act is None and not c.mask and not c.training]
ROUTES = ("bn_stats", "chan_stats + bn_finalize", "partials 1", "partials 3", "partials 300")


def _partials(x, k, seed):
    """(count, mean, M2) per channel of k disjoint pixel sets of unequal size that cover x [P, c] (float64), one empty set among them,
    rounded once -> [k + 1, c, 3] float32"""
    p, c = x.shape
    g = torch.Generator().manual_seed(seed)
    k = max(1, min(k, p // 2))
    order = torch.randperm(p, generator=g)
    cuts = sorted((torch.randperm(p - 1, generator=g)[:k - 1] + 1).tolist())
    sets = [order[a:z] for a, z in zip([0] + cuts, cuts + [p])]
    assert len(sets) == k and sum(len(s) for s in sets) == p and (k < 3 or len({len(s) for s in sets}) > 1)
    sets.insert(0 if k == 1 else k // 2, order[:0])
    part = torch.zeros((len(sets), c, 3), dtype=torch.float64)
    for i, s in enumerate(sets):
        if len(s):
            v = x[s]
            m = v.mean(dim=0)
            part[i, :, 0], part[i, :, 1], part[i, :, 2] = len(s), m, ((v - m) ** 2).sum(dim=0)
    return part.float()


def _torch_bn(case):
    """F.batch_norm and its autograd in float64 on the case's inputs -> y, dx, dgamma, dbeta (NHWC), running buffers after the call"""
    b = case.build()
    xt = b.x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    gamma, beta = b.gamma.double().requires_grad_(True), b.beta.double().requires_grad_(True)
    rm, rv = b.running_mean.double().clone(), b.running_var.double().clone()
    y = F.batch_norm(xt, rm, rv, gamma, beta, case.training, R.BN_MOMENTUM, R.BN_EPS)
    y.backward(b.dy.double().permute(0, 3, 1, 2))
    return NS(y=y.detach().permute(0, 2, 3, 1), dx=xt.grad.permute(0, 2, 3, 1), dgamma=gamma.grad, dbeta=beta.grad, running_mean=rm, running_var=rv)


_torch_ref = {}


def _e2e(case, route, monkeypatch):
    B, ops, _, _ = _mods()
    b = case.build()
    n, h, w, c = case.shape
    if case.id not in _torch_ref:
        _torch_ref[case.id] = (_torch_bn(case), R.end_to_end(case))
    t, ref = _torch_ref[case.id]
    rep = Report(f"{case.id} / {route}")
    ld = _lds(c)
    _, xv = wide(dev(b.x), *ld["x"])
    _, dyv = wide(dev(b.dy), *ld["dy"])
    st = B.BNState(dev(b.gamma), dev(b.beta), dev(b.running_mean).clone(), dev(b.running_var).clone(),
                   torch.tensor(b.nbt, dtype=torch.int64, device=DEV))
    sm = B.Small(DEV)
    monkeypatch.setattr(B, "FUSED_BN_STATS", True)
    if route == "eval":
        scale, shift, mean, invstd, _ = B.bn_coeff(xv, st, False, sm)
    elif route == "bn_stats":
        scale, shift, mean, invstd, _ = B.bn_coeff(xv, st, True, sm)
    elif route == "chan_stats + bn_finalize":
        scale, shift, mean, invstd, _ = B.bn_coeff(xv, st, True, sm, want_minmax=True)
    else:
        part = dev(_partials(b.x.double().reshape(-1, c), int(route.split()[1]), case.seed))
        scale, shift, mean, invstd, _ = B.bn_coeff(xv, st, True, sm, fused={"part": part, "nparts": part.shape[0]})
    y = B.bn_apply(xv, scale, shift)
    sums = torch.full((2 * c,), float("nan"), device=DEV)
    dx = B.bn_backward(dyv, xv, mean, invstd, scale, sums, training=case.training)
    for k, got in (("scale", scale), ("shift", shift), ("mean", mean), ("invstd", invstd), ("running_mean", st.running_mean),
                   ("running_var", st.running_var)):
        rep.close(k, got, getattr(ref.co, k), tol=bound(case, "e2e " + k))
    assert int(st.nbt) == b.nbt + (1 if case.training else 0)
    rep.close("running_mean against torch", st.running_mean, t.running_mean, tol=bound(case, "e2e running_mean"))
    rep.close("running_var against torch", st.running_var, t.running_var, tol=bound(case, "e2e running_var"))
    rep.close("y", y, t.y, tol=bound(case, "e2e y"))
    rep.close("dx", dx, t.dx, tol=bound(case, "e2e dx"))
    rep.close("dgamma", sums[:c], t.dgamma, ref.sum_scale[0], tol=bound(case, "e2e dgamma"))
    rep.close("dbeta", sums[c:], t.dbeta, ref.sum_scale[1], tol=bound(case, "e2e dbeta"))
    rep.done()


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("case", E2E, ids=lambda c: c.id)
def test_end_to_end_training(case, route, monkeypatch):
    """Identity activation, so no decision is involved: the three routes to the coefficients - runet_bn_stats; runet_chan_stats +
    runet_bn_finalize; runet_bn_stats_finalize on hand-made partials (1, 3 and 300 disjoint sets of unequal size and an empty one, built in
    float64 and rounded once) - on a sliced input with negative gammas, then bn_apply and bn_backward, against F.batch_norm autograd in float64."""
    _e2e(case, route, monkeypatch)


@pytest.mark.parametrize("case", E2E_EVAL, ids=lambda c: c.id)
def test_end_to_end_eval(case, monkeypatch):
    """runet_bn_finalize(training = 0): running statistics, buffers and num_batches_tracked unchanged, dx = dy * scale"""
    _e2e(case, "eval", monkeypatch)


# ----------------------------------------------------------------------------- argument checks
def test_entry_points_reject_bad_shapes():
    """Every rejected call would stay inside its buffers had it been launched (strides below the allocation's, a misaligned pointer into a
    larger buffer, n_img = 0); the entry points return an error and name themselves and the condition in runet_last_error."""
    B, ops, _, L = _mods()
    lib = L.lib
    n, h, w, c = 2, 4, 4, 8
    hw, st = h * w, ops.stream()
    t = lambda *s: torch.zeros(s, device=DEV)
    big, big2, v, v2 = t(n, h, w, c + 8), t(n, h, w, c + 8), t(c), t(2 * c)
    idx = torch.zeros((n, h // 2, w // 2, c + 8), device=DEV, dtype=torch.uint8)
    ws = B._ws(n, hw, c, DEV)
    p = lambda x: x.data_ptr()

    def rejected(rc, fn, text):
        err = lib.runet_last_error().decode("utf-8", "replace")
        assert rc != 0 and fn + ":" in err and text in err, (rc, err)
        with pytest.raises(RuntimeError):
            L.check(rc)

    def reduce(lddy=c, ldx=c, act=None, ldact=0, n_img=n, hw_=hw, c_=c):
        return lib.runet_bn_bwd_reduce(p(big), lddy, p(big2), ldx, act, ldact, n_img, hw_, c_, p(v), p(v), None, p(ws), p(v2), None, None, st)
    rejected(reduce(lddy=c - 4), "runet_bn_bwd_reduce", "bad shape")
    rejected(reduce(ldx=c - 4), "runet_bn_bwd_reduce", "bad shape")
    rejected(reduce(act=p(big), ldact=c - 4), "runet_bn_bwd_reduce", "bad shape")
    rejected(reduce(n_img=0), "runet_bn_bwd_reduce", "bad shape")
    rejected(reduce(hw_=0), "runet_bn_bwd_reduce", "bad shape")
    rejected(reduce(c_=6), "runet_bn_bwd_reduce", "channels must be 1 or a multiple of 4")

    def apply(lddy=c, ldx=c, act=None, ldact=0, lddx=c, pixels=n * hw, hw_=hw, c_=c):
        return lib.runet_bn_bwd_apply(p(big), lddy, p(big2), ldx, act, ldact, p(big), lddx, pixels, hw_, c_, p(v), p(v), p(v), p(v2), None, 0, None,
                                      st)
    rejected(apply(lddy=c - 4), "runet_bn_bwd_apply", "bad shape")
    rejected(apply(ldx=c - 4), "runet_bn_bwd_apply", "bad shape")
    rejected(apply(lddx=c - 4), "runet_bn_bwd_apply", "bad shape")
    rejected(apply(act=p(big2), ldact=c - 4), "runet_bn_bwd_apply", "bad shape")
    rejected(apply(pixels=0), "runet_bn_bwd_apply", "bad shape")
    rejected(apply(c_=6), "runet_bn_bwd_apply", "channels must be 1 or a multiple of 4")

    def pool_fwd(x=p(big), ldx=c, y=p(big2), ldy=c, i=p(idx), n_img=n, c_=c):
        return lib.runet_maxpool2_fwd(x, ldx, y, ldy, i, n_img, h, w, c_, st)
    rejected(pool_fwd(ldx=c - 4), "runet_maxpool2_fwd", "bad shape")
    rejected(pool_fwd(ldy=c - 4), "runet_maxpool2_fwd", "bad shape")
    rejected(pool_fwd(ldx=c + 2), "runet_maxpool2_fwd", "bad shape")
    rejected(pool_fwd(n_img=0), "runet_maxpool2_fwd", "bad shape")
    rejected(pool_fwd(x=p(big) + 4), "runet_maxpool2_fwd", "alignment")
    rejected(pool_fwd(y=p(big2) + 8), "runet_maxpool2_fwd", "alignment")
    rejected(pool_fwd(i=p(idx) + 2), "runet_maxpool2_fwd", "alignment")
    rejected(pool_fwd(c_=6), "runet_maxpool2_fwd", "c a multiple of 4")

    def pool_bwd(dy=p(big), lddy=c, dx=p(big2), lddx=c, i=p(idx), n_img=n, c_=c):
        return lib.runet_maxpool2_bwd(dy, lddy, i, dx, lddx, n_img, h, w, c_, 0, st)
    rejected(pool_bwd(lddy=c - 4), "runet_maxpool2_bwd", "bad shape")
    rejected(pool_bwd(lddx=c - 4), "runet_maxpool2_bwd", "bad shape")
    rejected(pool_bwd(lddx=c + 2), "runet_maxpool2_bwd", "bad shape")
    rejected(pool_bwd(n_img=0), "runet_maxpool2_bwd", "bad shape")
    rejected(pool_bwd(dy=p(big) + 4), "runet_maxpool2_bwd", "alignment")
    rejected(pool_bwd(dx=p(big2) + 8), "runet_maxpool2_bwd", "alignment")
    rejected(pool_bwd(i=p(idx) + 2), "runet_maxpool2_bwd", "alignment")
    rejected(pool_bwd(c_=6), "runet_maxpool2_bwd", "c a multiple of 4")
    torch.cuda.synchronize()
