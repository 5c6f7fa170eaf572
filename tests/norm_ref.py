"""Plain-torch restatement of the shared BatchNorm / activation / 2x2 pooling kernels of csrc/norm_act.hip and csrc/misc.hip, for any floating
dtype (float64 is the reference, float32 the rounding floor).  Test infrastructure only.

  coeffs            bn_coeffs / bn_running_update: scale, shift, saved statistics, running buffers (unbiased variance), num_batches_tracked
  apply             z = x * scale + shift, then nothing | ReLU [* Dropout2d factor mask_nc[n, c]] | LeakyReLU (z > 0 ? z : z * slope) | erf-GELU
  backward          g as the header of runet_bn_bwd_reduce defines it (no ReLU decision: the mask is not applied), sums = (sum g xhat | sum g),
                    dx = scale (g - sums[C + c] / M - xhat sums[c] / M), M = m_total if positive else the pixel count; eval: zero sums into dx
  pooled_grad       g(y, x) = idx[y / 2, x / 2] == (y & 1) * 2 + (x & 1) ? dpool[y / 2, x / 2] : 0
  maxpool / maxpool_scatter / maxunpool_gather     2x2 max-pool with winner byte k = dy * 2 + dx (first maximum, NaN wins), its scatter, the gather
  chan_sum          per-channel sum over all pixels
  geom              reduce_geom / pick_chunks, stream_geom / stream_chunks, final_cw of norm_act.hip in Python - used only to show that cases()
                    reaches every launch regime (tests/test_norm_ref_cpu.py); a changed chunking makes that test ask for new shapes

Tensors are NHWC, as the kernels see them.  `cases()` is the one list of inputs that tests/test_norm_ref_cpu.py and
tests/test_gpu_norm_kernels.py share; every value is drawn in float32, so both sides read the same numbers.  The kernel-level cases hand
scale, shift, mean and invstd (float32) to the kernel AND the reference as inputs, so an activation decision depends on one element of x only,
and x is built so that every |z| is at least MARGIN of max |z| - except the planted exact zeros (a channel with shift = 0 and x = +0.0 / -0.0).
"""
from __future__ import annotations

import math
from types import SimpleNamespace as NS

import torch

BN_EPS = 1e-5
BN_MOMENTUM = 0.1
SLOPE = 0.1
MARGIN = 1e-4
TPB = 256


# ----------------------------------------------------------------------------- the operations
def coeffs(x, gamma, beta, running_mean, running_var, nbt=0, momentum=BN_MOMENTUM, eps=BN_EPS, training=True):
    """-> scale, shift, mean, invstd (what the forward applies and the backward reads), the running buffers and nbt after the call"""
    dt = x.dtype
    gamma, beta, rm, rv = (v.to(dt) for v in (gamma, beta, running_mean, running_var))
    flat = x.reshape(-1, x.shape[-1])
    if training:
        m = flat.shape[0]
        mean = flat.mean(dim=0)
        var = ((flat - mean) ** 2).mean(dim=0)
        rm = (1.0 - momentum) * rm + momentum * mean
        rv = (1.0 - momentum) * rv + momentum * (var * (m / (m - 1.0)))
        nbt = nbt + 1
    else:
        mean, var = rm, rv
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * invstd
    return NS(scale=scale, shift=beta - mean * scale, mean=mean, invstd=invstd, running_mean=rm, running_var=rv, nbt=nbt)


def pre(x, scale, shift):
    return x * scale.to(x.dtype) + shift.to(x.dtype)


def _nc(mask_nc, like):
    return mask_nc.to(like.dtype)[:, None, None, :]


def activation(z, act=None, mask_nc=None, slope=SLOPE):
    if act == "relu":
        y = torch.clamp_min(z, 0.0)
    elif act == "leaky":
        y = torch.where(z > 0, z, z * slope)
    elif act == "gelu":
        y = z * 0.5 * (1.0 + torch.erf(z * math.sqrt(0.5)))
    else:
        assert act is None, act
        y = z
    if mask_nc is not None and act in (None, "relu"):
        y = y * _nc(mask_nc, z)
    return y


def apply(x, scale, shift, act=None, mask_nc=None, slope=SLOPE):
    return activation(pre(x, scale, shift), act, mask_nc, slope)


def act_grad(dy, z, act=None, mask_nc=None, slope=SLOPE):
    """the gradient in front of the activation; the Dropout2d factor goes with the ReLU decision only"""
    if act == "relu":
        gm = dy * _nc(mask_nc, dy) if mask_nc is not None else dy
        return torch.where(z > 0, gm, torch.zeros_like(gm))
    if act == "leaky":
        return torch.where(z > 0, dy, dy * slope)
    if act == "gelu":
        cdf = 0.5 * (1.0 + torch.erf(z * math.sqrt(0.5)))
        pdf = torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
        return dy * (cdf + z * pdf)
    assert act is None, act
    return dy


def backward(dy, x, mean, invstd, scale, shift, act=None, mask_nc=None, slope=SLOPE, training=True, m_total=0, sums_in=None):
    """dy: the gradient behind the activation (for the pooled forms: pooled_grad(dpool, idx)).  sums_in: the sums that enter dx when they are
    not the local ones (SyncBN).  -> g, sums [2c] = (dgamma | dbeta), dx, and sum_scale = the largest per-channel (sum |g xhat|, sum |g|)"""
    dt = x.dtype
    mean, invstd, scale, shift = (v.to(dt) for v in (mean, invstd, scale, shift))
    dy = dy.to(dt)
    c = x.shape[-1]
    g = act_grad(dy, pre(x, scale, shift), act, mask_nc, slope)
    xhat = (x - mean) * invstd
    gx = (g * xhat).reshape(-1, c)
    gf = g.reshape(-1, c)
    sums = torch.cat([gx.sum(dim=0), gf.sum(dim=0)])
    sum_scale = (float(gx.abs().sum(dim=0).max()), float(gf.abs().sum(dim=0).max()))
    if training:
        use = sums if sums_in is None else sums_in.to(dt)
        m = float(m_total if m_total > 0 else gf.shape[0])
        dx = scale * (g - use[c:] / m - xhat * (use[:c] / m))
    else:
        dx = scale * g
    return NS(g=g, sums=sums, dx=dx, sum_scale=sum_scale)


def _windows(x):
    """the four window positions k = dy * 2 + dx of every 2x2 window: [4][n, h/2, w/2, c]"""
    return [x[:, (k >> 1)::2, (k & 1)::2, :] for k in range(4)]


def maxpool(x):
    """-> (values, winner bytes): the first maximum in scan order wins, a NaN wins over everything before it"""
    v = _windows(x)
    m, sel = v[0], torch.zeros(v[0].shape, dtype=torch.uint8)
    for k in (1, 2, 3):
        take = (v[k] > m) | torch.isnan(v[k])
        m = torch.where(take, v[k], m)
        sel = torch.where(take, torch.full_like(sel, k), sel)
    return m, sel


def pooled_grad(dpool, idx):
    n, ho, wo, c = dpool.shape
    g = torch.zeros((n, ho, 2, wo, 2, c), dtype=dpool.dtype)
    for k in range(4):
        g[:, :, k >> 1, :, k & 1, :] = torch.where(idx == k, dpool, torch.zeros_like(dpool))
    return g.reshape(n, 2 * ho, 2 * wo, c)


def maxpool_scatter(dpool, idx, into=None):
    """runet_maxpool2_bwd: overwrite (into None) or accumulate"""
    g = pooled_grad(dpool, idx)
    return g if into is None else into + g


def maxunpool_gather(du, idx):
    v = _windows(du)
    out = v[0]
    for k in (1, 2, 3):
        out = torch.where(idx == k, v[k], out)
    return out


def chan_sum(x, out0=None):
    """-> (sums [c] (+ out0), the largest per-channel sum of |terms|)"""
    flat = x.reshape(-1, x.shape[-1])
    s = flat.sum(dim=0)
    return (s if out0 is None else s + out0.to(x.dtype)), float(flat.abs().sum(dim=0).max())


# ----------------------------------------------------------------------------- launch geometry (norm_act.hip, restated)
def _cdiv(a, b):
    return (a + b - 1) // b


def _row_counts(hw, ppc, chunks, rows):
    """how many pixels a thread row takes in a chunk, over all rows of all chunks (0 left out)"""
    out = set()
    for k in range(chunks):
        m = max(0, min(hw, (k + 1) * ppc) - k * ppc)
        out.update({_cdiv(m - r, rows) for r in range(min(rows, m))})
    return out


def geom(n, hw, c):
    vec = 4 if c % 4 == 0 else 1
    cvec = c // vec
    rows = TPB // cvec
    # reduce_geom / pick_chunks
    per = max(_cdiv(hw * c, 32768), _cdiv(768, n), 1)
    per = min(per, 1024, _cdiv(hw, rows))
    r_chunks, r_ppc = per, _cdiv(hw, per)
    # stream_geom / stream_chunks
    per = max(min(_cdiv(hw * c, 16384), _cdiv(hw, rows), 4096), 1)
    s_ppc = _cdiv(hw, per)
    s_chunks = _cdiv(hw, s_ppc)
    nparts = r_chunks * n
    return NS(vec=vec, rows=rows, idle=TPB - rows * cvec, r_chunks=r_chunks, r_ppc=r_ppc, r_counts=_row_counts(hw, r_ppc, r_chunks, rows),
              r_ragged=hw % r_ppc != 0, s_chunks=s_chunks, s_ppc=s_ppc, s_passes=_cdiv(s_ppc, rows), s_ragged=s_ppc % rows != 0,
              nparts=nparts, final_cw=min(c, 4 if nparts >= 256 else 32))


def chan_sum_geom(pixels, c):
    chunks = max(1, min(2048, _cdiv(pixels * c, 32768)))
    ppc = _cdiv(pixels, chunks)
    chunks = _cdiv(pixels, ppc)
    return NS(chunks=chunks, ppc=ppc, final_cw=min(c, 4 if chunks >= 256 else 32))


# ----------------------------------------------------------------------------- the inputs
def _randn(g, *shape):
    return torch.randn(shape, generator=g, dtype=torch.float32)


def _rand(g, *shape):
    return torch.rand(shape, generator=g, dtype=torch.float32)


class Case:
    """kind: "bn" (apply + backward), "pooled" (the pooled backward), "pool" (pool / scatter / gather), "chansum"."""

    def __init__(self, kind, shape, seed, act=None, mask=False, training=True, cond=False):
        self.kind, self.shape, self.seed, self.act, self.mask, self.training, self.cond = kind, shape, seed, act, mask, training, cond
        self.decision = kind in ("bn", "pooled") and act in ("relu", "leaky")
        self.id = "-".join([kind, "x".join(str(v) for v in shape), act or "id"] + (["mask"] if mask else []) + ([] if training else ["eval"])
                           + (["cond"] if cond else []))
        self._built = None

    def __repr__(self):
        return self.id

    def build(self):
        """built once; the tests read it and leave it unchanged"""
        if self._built is None:
            g = torch.Generator().manual_seed(self.seed)
            self._built = {"bn": self._bn, "pooled": self._bn, "pool": self._pool, "chansum": self._chansum}[self.kind](g)
        return self._built

    def _bn(self, g):
        n, h, w, c = self.shape
        if self.cond:          # mean / std = 100: dx = g sc + x ca + cb cancels as |mean| invstd grows
            sx, mx = torch.full((c,), 0.5), torch.full((c,), 50.0)
        else:
            sx, mx = 0.5 + 1.5 * _rand(g, c), _randn(g, c)
        x = _randn(g, n, h, w, c) * sx + mx
        gamma = 1.0 + 0.3 * _randn(g, c)
        gamma[c - 1] = -gamma[c - 1].abs() if (c > 1 or self.seed % 2) else gamma[c - 1].abs()
        gamma[3::5] = -gamma[3::5].abs()
        beta = 0.3 * _randn(g, c)
        rm, rv = mx + 0.1 * sx * _randn(g, c), sx * sx * (0.8 + 0.4 * _rand(g, c))
        dy = _randn(g, n, h, w, c)
        mask_nc = None
        if self.mask:          # Dropout2d(0.3): whole (image, channel) planes dropped, the others scaled by 1 / 0.7
            keep = float(torch.tensor(1.0 / 0.7, dtype=torch.float32))
            mask_nc = (_rand(g, n, c) >= 0.3).float() * keep
            if c > 1:          # the channel of the planted zeros is kept; another one is dropped in EVERY image: its sums, so its dx, are zero
                mask_nc[:, 0], mask_nc[:, 1] = keep, 0.0
            else:
                mask_nc[0, 0], mask_nc[n - 1, 0] = 0.0, keep
        dpool = _randn(g, n, h // 2, w // 2, c) if self.kind == "pooled" else None
        co = coeffs(x.double(), gamma, beta, rm, rv, training=self.training)
        if self.training and n * h * w <= 2:
            # two values per channel: with the batch's own statistics xhat = +-1 and dx vanishes identically, so dx would be rounding noise and
            # its relative error meaningless.  The coefficients are inputs: take the statistics the values were drawn from instead.
            co = coeffs(x.double(), gamma, beta, mx, sx * sx, training=False)
        scale, shift, mean, invstd = (v.float() for v in (co.scale, co.shift, co.mean, co.invstd))
        planted = torch.zeros((n * h * w,), dtype=torch.bool)
        if self.decision:
            shift[0] = 0.0
            p = n * h * w
            where = [0, p - 1] + ([p // 3, p // 2] if p >= 8 else [])
            col = x.reshape(-1, c)[:, 0]
            for i, q in enumerate(where):
                col[q] = 0.0 if i % 2 == 0 else -0.0
                planted[q] = True
            x = self._margin(x, scale, shift, planted)
        b = NS(x=x, dy=dy, gamma=gamma, beta=beta, running_mean=rm, running_var=rv, nbt=3, mask_nc=mask_nc, scale=scale, shift=shift, mean=mean,
               invstd=invstd, planted=planted, dpool=dpool, idx=None)
        if self.kind == "pooled":
            b.idx = maxpool(apply(x.double(), scale, shift, self.act))[1]
        return b

    @staticmethod
    def _margin(x, scale, shift, planted):
        """move every element whose |z| is below MARGIN of max |z| to twice that distance, on its own side; the planted zeros stay"""
        c = x.shape[-1]
        z = pre(x.double(), scale, shift)
        thr = MARGIN * float(z.abs().max())
        keep = torch.zeros(z.shape, dtype=torch.bool)
        keep.reshape(-1, c)[:, 0] = planted
        bad = (z.abs() < thr) & ~keep
        target = torch.where(z >= 0, torch.full_like(z, 2 * thr), torch.full_like(z, -2 * thr))
        moved = ((target - shift.double()) / scale.double()).float()
        return torch.where(bad, moved, x)

    def _pool(self, g):
        n, h, w, c = self.shape
        x = _randn(g, n, h, w, c)
        x[0, 0:2, 0:2, 0] = 0.75                                   # four equal values: the first wins
        x[0, 0:2, 0:2, 1] = torch.tensor([[-1.0, 2.5], [2.5, 0.5]])  # two equal maxima at k = 1 and k = 2: k = 1 wins
        x[0, 0:2, 0:2, 2] = -x[0, 0:2, 0:2, 2].abs() - 0.125         # an all-negative window
        x[n - 1, h - 2:h, w - 2:w, 3] = torch.tensor([[3.0, float("nan")], [4.0, 1.0]])    # NaN at k = 1, a larger value behind it: the NaN stays
        return NS(x=x, dpool=_randn(g, n, h // 2, w // 2, c), base=_randn(g, n, h, w, c), du=_randn(g, n, h, w, c))

    def _chansum(self, g):
        n, h, w, c = self.shape
        return NS(x=_randn(g, n, h, w, c) + 0.25, out0=_randn(g, c) * 10)


ALL_SHAPES = [(2, 1, 1, 4), (1, 2, 1, 4), (2, 1, 3, 1), (3, 5, 7, 12), (2, 18, 22, 12), (2, 5, 7, 64), (2, 6, 10, 516), (2, 3, 5, 1024),
              (2, 28, 28, 1024), (16, 40, 40, 36), (48, 72, 72, 4), (3, 20, 28, 1), (2, 66, 34, 1)]
MAIN = [(3, 5, 7, 12), (2, 5, 7, 64), (2, 6, 10, 516), (2, 3, 5, 1024), (3, 20, 28, 1)]      # c = 12, 64, 516, 1024 and 1
POOLED_SHAPES = [(2, 2, 2, 4), (3, 6, 10, 12), (2, 10, 6, 516), (16, 40, 40, 36)]
CHANSUM_SHAPES = [(3, 20, 28, 1), (3, 5, 7, 12), (2, 6, 10, 516), (2, 3, 5, 1024), (48, 72, 72, 4)]
COND_SHAPES = [(3, 5, 7, 12), (16, 40, 40, 36)]
_cases = None


def cases():
    global _cases
    if _cases is None:
        out = []

        def add(kind, shapes, **kw):
            for s in shapes:
                out.append(Case(kind, s, 1000 + len(out), **kw))
        add("bn", ALL_SHAPES)
        add("bn", MAIN, mask=True)
        add("bn", MAIN, training=False)
        add("bn", COND_SHAPES, cond=True)
        add("bn", ALL_SHAPES, act="relu")
        add("bn", MAIN + [(16, 40, 40, 36)], act="relu", mask=True)
        add("bn", MAIN, act="relu", training=False)
        add("bn", MAIN + [(2, 18, 22, 12), (2, 28, 28, 1024), (2, 66, 34, 1)], act="leaky")
        add("bn", MAIN, act="leaky", training=False)
        add("bn", MAIN + [(2, 1, 3, 1), (2, 28, 28, 1024), (16, 40, 40, 36)], act="gelu")
        add("bn", MAIN, act="gelu", training=False)
        for act in ("relu", "leaky"):
            add("pooled", POOLED_SHAPES, act=act)
            add("pooled", [(3, 6, 10, 12)], act=act, training=False)
        add("pool", POOLED_SHAPES)
        add("chansum", CHANSUM_SHAPES)
        _cases = out
    return _cases


# ----------------------------------------------------------------------------- running a case
def run(case, dtype=torch.float64):
    """A "bn" / "pooled" case in `dtype` from its float32 inputs -> y (bn only), z, g_in (the gradient behind the activation), and backward()'s
    results.  Shared by the CPU test, the GPU test and fp32_floor."""
    b = case.build()
    x = b.x.to(dtype)
    z = pre(x, b.scale, b.shift)
    y = activation(z, case.act, b.mask_nc) if case.kind == "bn" else None
    g_in = pooled_grad(b.dpool.to(dtype), b.idx) if case.kind == "pooled" else b.dy.to(dtype)
    r = backward(g_in, x, b.mean, b.invstd, b.scale, b.shift, case.act, b.mask_nc, training=case.training)
    r.y, r.z, r.g_in = y, z, g_in
    return r


_ref = {}


def reference(case):
    """run(case) in float64, computed once and shared; callers leave it unchanged"""
    if case.id not in _ref:
        _ref[case.id] = run(case)
    return _ref[case.id]


def rel_err(a, b, scale=None):
    """max |a - b| over b's largest magnitude (b: the reference), or over `scale` where given (the sums: the largest per-channel sum of |terms|)"""
    b = b.detach().double()
    return float((a.detach().double() - b).abs().max()) / (scale if scale else max(float(b.abs().max()), 1e-300))


def end_to_end(case, dtype=torch.float64):
    """An identity-activation "bn" case with the coefficients taken from x in `dtype`: coefficients, running buffers, y, sums and dx"""
    b = case.build()
    x = b.x.to(dtype)
    co = coeffs(x, b.gamma, b.beta, b.running_mean, b.running_var, b.nbt, training=case.training)
    r = backward(b.dy.to(dtype), x, co.mean, co.invstd, co.scale, co.shift, training=case.training)
    r.y = pre(x, co.scale, co.shift)
    r.co = co
    return r


def b_pixels(case):
    return case.shape[0] * case.shape[1] * case.shape[2]


COEF = ("scale", "shift", "mean", "invstd", "running_mean", "running_var")
_floor = {}


def fp32_floor(case):
    """{tensor: error of the float32 restatement against the float64 one, relative to the tensor's largest magnitude (sums: to sum_scale)},
    both from the same float32 inputs.  No kernel is involved.  "e2e ..." rows: the same with the coefficients derived from x in each dtype."""
    if case.id in _floor:
        return _floor[case.id]
    out = {}
    if case.kind == "chansum":
        b = case.build()
        (s64, sc), (s32, _) = chan_sum(b.x.double(), b.out0), chan_sum(b.x, b.out0)
        out["sum"] = rel_err(s32, s64, sc)
    elif case.kind in ("bn", "pooled"):
        r64, r32 = reference(case), run(case, torch.float32)
        c = case.shape[3]
        if case.decision:
            assert torch.equal(r32.z > 0, r64.z > 0), "a float32 decision differs from the float64 one: the margin does not hold"
        if r64.y is not None:
            out["y"] = rel_err(r32.y, r64.y)
        out["dgamma"] = rel_err(r32.sums[:c], r64.sums[:c], r64.sum_scale[0])
        out["dbeta"] = rel_err(r32.sums[c:], r64.sums[c:], r64.sum_scale[1])
        out["dx"] = rel_err(r32.dx, r64.dx)
        if case.kind == "bn" and case.act is None and not case.mask and b_pixels(case) > 2:
            e64, e32 = end_to_end(case), end_to_end(case, torch.float32)
            for k in COEF:
                out["e2e " + k] = rel_err(getattr(e32.co, k), getattr(e64.co, k))
            out["e2e y"] = rel_err(e32.y, e64.y)
            out["e2e dgamma"] = rel_err(e32.sums[:c], e64.sums[:c], e64.sum_scale[0])
            out["e2e dbeta"] = rel_err(e32.sums[c:], e64.sums[c:], e64.sum_scale[1])
            out["e2e dx"] = rel_err(e32.dx, e64.dx)
    _floor[case.id] = out
    return out


def kernel_form_floor(case):
    """dx by the kernels' own expression g sc + x ca + cb (bn_bwd_coef / bn_bwd_dx of runet_common.h, without their fused multiply-adds) in
    float32 against the float64 reference: what that FORM costs at a large |mean| invstd.  Printed by the CPU test, not a bound."""
    b, r64 = case.build(), reference(case)
    c = case.shape[3]
    x, g = b.x, r64.g.float()
    sums = r64.sums.float()
    inv_m = torch.tensor(1.0 / (x.numel() // c), dtype=torch.float32)
    k1, k2 = sums[c:] * inv_m, sums[:c] * inv_m
    ca = -b.scale * k2 * b.invstd
    cb = b.scale * (b.mean * b.invstd * k2 - k1)
    return rel_err(g * b.scale + (x * ca + cb), r64.dx)
