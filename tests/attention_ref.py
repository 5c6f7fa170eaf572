"""Plain-torch restatement of what csrc/attention.hip computes, for any floating dtype (float64 is the reference, float32 the rounding floor).
Test infrastructure only.

  channel_attention   Main_Final.py:82-101
  spatial_attention   Main_Final.py:104-117
  tail                Main_Final.py:186-194, from the conv2 output on: bn2 -> channel attention -> spatial attention -> + residual -> ReLU
  gate                Main_Final.py:120-148, from the raw W_g.0 / W_x.0 outputs on

Every function is differentiable (autograd supplies the backward reference) and returns each intermediate the kernels expose.  Both
arg-maxima are taken with `max(dim=...)`, whose CPU kernel returns the FIRST occurrence and whose backward routes the gradient to that one
index (`amax` / `adaptive_max_pool2d` would agree on the value; `amax` splits the gradient among ties).

Tensors are NCHW; a state `P` maps the module's own parameter names ("bn2.weight", "ca.fc.0.weight", "W_g.1.running_var", ...) to tensors.

`cases()` is the one list of inputs that tests/test_attention_ref_cpu.py (conditions on the float64 reference) and
tests/test_gpu_attention_kernels.py (the kernels) share.  The seeds were found by a search on the CPU for inputs on which a correct fp32
kernel must take the float64 reference's arg-max decisions (see the CPU test); every value is drawn in float32, so both sides read the
same numbers.
"""
from __future__ import annotations

import math
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

BN_EPS = 1e-5
NEG_GAMMA = 0.3            # share of negative gammas in every BatchNorm of a case


# ----------------------------------------------------------------------------- the operations
def bn_coeff(x, P, name, training):
    """BatchNorm2d as a per-channel affine map: -> (scale, shift, mean, invstd), batch (biased variance) or running statistics"""
    if training:
        mean = x.mean(dim=(0, 2, 3))
        var = ((x - mean[None, :, None, None]) ** 2).mean(dim=(0, 2, 3))
    else:
        mean, var = P[f"{name}.running_mean"].to(x.dtype), P[f"{name}.running_var"].to(x.dtype)
    invstd = 1.0 / torch.sqrt(var + BN_EPS)
    scale = P[f"{name}.weight"] * invstd
    return scale, P[f"{name}.bias"] - mean * scale, mean, invstd


def _ch(v):
    return v[None, :, None, None]


def channel_attention(x, w0, w2):
    """x [n,c,h,w]; w0 [cr,c,1,1], w2 [c,cr,1,1].  -> y = x * ca and (avg, mx, idx: the first pixel h*W+w holding the maximum, ca), all [n,c]"""
    n, c, h, w = x.shape
    flat = x.reshape(n, c, h * w)
    avg = flat.mean(dim=2)
    mx, idx = flat.max(dim=2)
    W0, W2 = w0.reshape(w0.shape[0], c), w2.reshape(c, w2.shape[1])
    mlp = lambda v: torch.relu(v @ W0.t()) @ W2.t()
    ca = torch.sigmoid(mlp(avg) + mlp(mx))
    return NS(y=x * ca[:, :, None, None], avg=avg, mx=mx, idx=idx, ca=ca)


def spatial_attention(x, wsa):
    """x [n,c,h,w]; wsa [1,2,7,7].  -> y = x * sa and (smap [n,2,h,w] = (mean_c, max_c), amax [n,h,w]: the first channel holding the maximum,
    sa [n,1,h,w])"""
    mxc, amax = x.max(dim=1, keepdim=True)
    smap = torch.cat([x.mean(dim=1, keepdim=True), mxc], dim=1)
    sa = torch.sigmoid(F.conv2d(smap, wsa, padding=3))
    return NS(y=x * sa, smap=smap, amax=amax[:, 0], sa=sa)


def tail(t2, r, P, training, relu_mask=None):
    """t2: conv2's raw output; r: the shortcut convolution's raw output ("shortcut.1.weight" in P) or the block's input.
    relu_mask (0/1, out's shape): out = pre * relu_mask instead of relu(pre) - the reference under somebody else's ReLU decisions."""
    s2, h2, mean2, invstd2 = bn_coeff(t2, P, "bn2", training)
    u0 = t2 * _ch(s2) + _ch(h2)
    ca = channel_attention(u0, P["ca.fc.0.weight"], P["ca.fc.2.weight"])
    n, c, h, w = t2.shape
    tval = torch.gather(t2.reshape(n, c, h * w), 2, ca.idx[:, :, None])[:, :, 0]
    sa = spatial_attention(ca.y, P["sa.conv1.weight"])
    ss = hs = mean_s = invstd_s = None
    res = r
    if "shortcut.1.weight" in P:
        ss, hs, mean_s, invstd_s = bn_coeff(r, P, "shortcut.1", training)
        res = r * _ch(ss) + _ch(hs)
    pre = sa.y + res
    out = torch.relu(pre) if relu_mask is None else pre * relu_mask.to(pre.dtype)
    return NS(out=out, pre=pre, s2=s2, h2=h2, mean2=mean2, invstd2=invstd2, avg=ca.avg, mx=ca.mx, idx=ca.idx, tval=tval, ca=ca.ca,
              A=s2[None] * ca.ca, B=h2[None] * ca.ca, u=ca.y, smap=sa.smap, amax=sa.amax, sa=sa.sa, ss=ss, hs=hs, mean_s=mean_s, invstd_s=invstd_s)


def gate(g1, x1, skip, P, training, relu_mask=None):
    """g1 / x1: the raw outputs of W_g.0 / W_x.0 (bias included).  -> att = skip * sigmoid(bn(psi(relu(bn g1 + bn x1)))), s (psi.0's output,
    [n,1,h,w]) and the three BatchNorms' coefficients.  relu_mask as in tail()."""
    sg, hg, mean_g, invstd_g = bn_coeff(g1, P, "W_g.1", training)
    sx, hx, mean_x, invstd_x = bn_coeff(x1, P, "W_x.1", training)
    pre = g1 * _ch(sg) + _ch(hg) + x1 * _ch(sx) + _ch(hx)
    act = torch.relu(pre) if relu_mask is None else pre * relu_mask.to(pre.dtype)
    s = F.conv2d(act, P["psi.0.weight"], P["psi.0.bias"])
    sp, hp, mean_p, invstd_p = bn_coeff(s, P, "psi.1", training)
    sig = torch.sigmoid(s * _ch(sp) + _ch(hp))
    return NS(att=skip * sig, s=s, pre=pre, sig=sig, sg=sg, hg=hg, mean_g=mean_g, invstd_g=invstd_g, sx=sx, hx=hx, mean_x=mean_x,
              invstd_x=invstd_x, sp=sp, hp=hp, mean_p=mean_p, invstd_p=invstd_p)


def tail_inputs(x, P, training, mask=None):
    """The block in front of the tail with F.conv2d: -> (t2, r) as tail() takes them.  mask: [n,c] Dropout2d factors (training only)."""
    t1 = F.conv2d(x, P["conv1.weight"], padding=1)
    s1, h1, _, _ = bn_coeff(t1, P, "bn1", training)
    a1 = torch.relu(t1 * _ch(s1) + _ch(h1))
    if training and mask is not None:
        a1 = a1 * mask[:, :, None, None].to(a1.dtype)
    t2 = F.conv2d(a1, P["conv2.weight"], padding=1)
    r = F.conv2d(x, P["shortcut.0.weight"]) if "shortcut.0.weight" in P else x
    return t2, r


def gate_inputs(g, x, P):
    return F.conv2d(g, P["W_g.0.weight"], P["W_g.0.bias"]), F.conv2d(x, P["W_x.0.weight"], P["W_x.0.bias"])


# ----------------------------------------------------------------------------- the cases
def _randn(g, *shape, std=1.0):
    return torch.randn(shape, generator=g, dtype=torch.float32) * std


def _bn_state(g, c, pre, P, var=1.0):
    """gamma: magnitude in [0.5, 1.5], NEG_GAMMA of them negative (at least one of each sign from two channels on); beta N(0, 0.1);
    running statistics near those of the tensor the BatchNorm sees (variance `var`), not at them"""
    gamma = torch.rand(c, generator=g, dtype=torch.float32) + 0.5
    neg = torch.rand(c, generator=g, dtype=torch.float32) < NEG_GAMMA
    if c >= 2:
        neg[int(torch.randint(0, c, (1,), generator=g))] = True
        if bool(neg.all()):
            neg[0] = False
    P[f"{pre}.weight"] = torch.where(neg, -gamma, gamma)
    P[f"{pre}.bias"] = _randn(g, c, std=0.1)
    P[f"{pre}.running_mean"] = _randn(g, c, std=0.1 * math.sqrt(var))
    P[f"{pre}.running_var"] = (torch.rand(c, generator=g, dtype=torch.float32) + 0.5) * var
    P[f"{pre}.num_batches_tracked"] = torch.zeros((), dtype=torch.int64)


class Case:
    """kind "tail": shape (n, h, w, cin, cout); "gate": (n, h, w, c, f); "ca" / "sa": (n, h, w, c).  flags: training, pool, tie, and the
    blocks.py switch the GPU test sets (`switch`).  build() -> float32 CPU tensors, NCHW, OIHW: the same on every call."""

    def __init__(self, kind, shape, seed, **flags):
        self.kind, self.shape, self.seed = kind, tuple(shape), seed
        self.training = flags.pop("training", True)
        self.pool = flags.pop("pool", False)
        self.tie = flags.pop("tie", False)
        self.switch = flags.pop("switch", None)        # (name of a blocks.py flag, value) or None
        assert not flags, flags
        self.id = f"{kind}-" + "x".join(str(v) for v in self.shape) + ("" if self.training else "-eval") + ("-pool" if self.pool else "") + (
            "-tie" if self.tie else "") + (f"-{self.switch[0]}={int(self.switch[1])}" if self.switch else "")

    def build(self):
        g = torch.Generator().manual_seed(self.seed)
        return getattr(self, "_" + self.kind)(g)

    def _tail(self, g):
        n, h, w, cin, cout = self.shape
        cr = cout // 16
        P = {}
        # conv1 / conv2: variance-preserving for a unit-variance input and for relu(bn) * mask in front of conv2
        P["conv1.weight"] = _randn(g, cout, cin, 3, 3, std=math.sqrt(1.0 / (9 * cin)))
        _bn_state(g, cout, "bn1", P)
        P["conv2.weight"] = _randn(g, cout, cout, 3, 3, std=math.sqrt(2.0 / (9 * cout)))
        _bn_state(g, cout, "bn2", P)
        # the attention weights keep both sigmoids out of saturation: |fc(.)| ~ 1, |conv7(.)| ~ 1
        P["ca.fc.0.weight"] = _randn(g, cr, cout, 1, 1, std=0.5 / math.sqrt(cout))
        P["ca.fc.2.weight"] = _randn(g, cout, cr, 1, 1, std=1.0 / math.sqrt(cr))
        P["sa.conv1.weight"] = _randn(g, 1, 2, 7, 7, std=0.12)
        if cin != cout:
            P["shortcut.0.weight"] = _randn(g, cout, cin, 1, 1, std=math.sqrt(1.0 / cin))
            _bn_state(g, cout, "shortcut.1", P)
        x = _randn(g, n, cin, h, w)
        keep = (torch.rand((n, cout), generator=g, dtype=torch.float32) < 0.8).float() / 0.8
        dout = _randn(g, n, cout, h, w)
        dpool = _randn(g, n, cout, h // 2, w // 2) if self.pool else None
        return NS(P=P, x=x, mask=keep if self.training else None, dout=dout, dpool=dpool)

    def _gate(self, g):
        n, h, w, c, f = self.shape
        P = {}
        P["W_g.0.weight"], P["W_g.0.bias"] = _randn(g, f, c, 1, 1, std=math.sqrt(1.0 / c)), _randn(g, f, std=0.1)
        _bn_state(g, f, "W_g.1", P)
        P["W_x.0.weight"], P["W_x.0.bias"] = _randn(g, f, c, 1, 1, std=math.sqrt(1.0 / c)), _randn(g, f, std=0.1)
        _bn_state(g, f, "W_x.1", P)
        P["psi.0.weight"], P["psi.0.bias"] = _randn(g, 1, f, 1, 1, std=math.sqrt(1.0 / f)), _randn(g, 1, std=0.1)
        _bn_state(g, 1, "psi.1", P, var=0.7)
        up, skip = _randn(g, n, c, h, w), _randn(g, n, c, h, w)
        dcat = _randn(g, n, 2 * c, h, w)
        return NS(P=P, up=up, skip=skip, dcat=dcat)

    def _ca(self, g):
        n, h, w, c = self.shape
        cr = c // 16
        P = {"fc.0.weight": _randn(g, cr, c, 1, 1, std=0.5 / math.sqrt(c)), "fc.2.weight": _randn(g, c, cr, 1, 1, std=1.0 / math.sqrt(cr))}
        x = _randn(g, n, c, h, w)
        ties = None
        if self.tie:        # every fourth channel: the maximum twice, at the pixels hw // 3 and hw - 1 (the lower index must win)
            flat = x.reshape(n, c, h * w)
            top = flat.max(dim=2).values + 0.5
            ties = torch.arange(0, c, 4)
            flat[:, ties, h * w // 3] = top[:, ties]
            flat[:, ties, h * w - 1] = top[:, ties]
        return NS(P=P, x=x, dy=_randn(g, n, c, h, w), ties=ties)

    def _sa(self, g):
        n, h, w, c = self.shape
        P = {"conv1.weight": _randn(g, 1, 2, 7, 7, std=0.12)}
        x = _randn(g, n, c, h, w)
        ties = None
        if self.tie:        # every third pixel: the maximum twice, in channels c // 4 and c - 1 (two lanes of the kernel's 16 from c = 8 on)
            flat = x.permute(0, 2, 3, 1).reshape(-1, c)
            top = flat.max(dim=1).values + 0.5
            ties = torch.arange(0, flat.shape[0], 3)
            flat[ties, c // 4] = top[ties]
            flat[ties, c - 1] = top[ties]
            x = flat.reshape(n, h, w, c).permute(0, 3, 1, 2).contiguous()
        return NS(P=P, x=x, dy=_randn(g, n, c, h, w), ties=ties)


def cases():
    """Seeds: tests/test_attention_ref_cpu.py's input conditions hold for each (found by a search over seeds from 1 upwards)."""
    T, G = "tail", "gate"
    return [
        Case("ca", (2, 8, 8, 32), 1), Case("ca", (3, 5, 7, 16), 1), Case("ca", (1, 2, 2, 1024), 1), Case("ca", (2, 20, 36, 48), 1),
        Case("ca", (2, 8, 8, 32), 1, tie=True),
        Case("sa", (2, 8, 8, 32), 1), Case("sa", (3, 5, 7, 4), 1), Case("sa", (2, 6, 3, 16), 1), Case("sa", (2, 20, 36, 64), 1),
        Case("sa", (1, 17, 33, 128), 1), Case("sa", (2, 8, 8, 32), 1, tie=True),
        Case(T, (2, 8, 8, 32, 48), 1), Case(T, (2, 8, 8, 32, 48), 1, training=False),
        Case(T, (3, 6, 10, 8, 16), 1, pool=True), Case(T, (2, 20, 36, 32, 64), 4, pool=True),
        Case(T, (2, 16, 16, 128, 128), 1, pool=True), Case(T, (1, 2, 2, 1024, 1024), 3), Case(T, (1, 4, 4, 256, 1024), 1),
        Case(T, (2, 20, 36, 32, 64), 4, switch=("FUSED_SHORTCUT_BN_SUMS", True)),
        Case(T, (2, 20, 36, 32, 64), 4, switch=("FUSED_RB_EDGES", False)),
        Case(G, (2, 8, 8, 32, 16), 1), Case(G, (3, 6, 10, 16, 8), 1), Case(G, (2, 20, 36, 24, 12), 1), Case(G, (2, 20, 36, 64, 32), 1),
        Case(G, (2, 2, 2, 512, 256), 1), Case(G, (2, 8, 8, 32, 16), 1, training=False),
        Case(G, (2, 8, 8, 32, 16), 1, switch=("FUSED_GATE_BN_SUMS", False)),
    ]


def f64(v):
    """a build()'s tensors (or a state dict) in float64"""
    if isinstance(v, dict):
        return {k: (t.double() if t.is_floating_point() else t) for k, t in v.items()}
    return v.double() if v is not None else None


# ----------------------------------------------------------------------------- what the tests assert about a case (float64 reference alone)
MARGIN = 2e-5          # twice the forward tolerance of the GPU tests


def top2_margin(v, dim):
    t = torch.topk(v, 2, dim=dim).values
    return t.select(dim, 0) - t.select(dim, 1)


def conditions(case, dtype=torch.float64):
    """-> dict of the figures the input conditions are about, from the reference in `dtype`:
    ch_margin / sp_margin: smallest top-1 minus top-2 over the channels of u at a pixel / over the pixels of u0 for an (n, c), relative to the
    tensor's largest magnitude, planted ties left out (tie_exact says that those are exact); near_zero: share of ReLU inputs within MARGIN of
    scale of zero; ca_mid / sa_mid: share of the sigmoid outputs in [0.1, 0.9]; positive: share of ReLU inputs above zero."""
    b = case.build()
    P = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in b.P.items()}
    out = {}
    mid = lambda v: float(((v >= 0.1) & (v <= 0.9)).double().mean())
    if case.kind == "tail":
        t2, r = tail_inputs(b.x.to(dtype), P, case.training, b.mask)
        ref = tail(t2, r, P, case.training)
        n, c, h, w = t2.shape
        u0 = t2 * _ch(ref.s2) + _ch(ref.h2)
        out["ch_margin"] = float(top2_margin(ref.u, 1).min() / ref.u.abs().max())
        out["sp_margin"] = float(top2_margin(u0.reshape(n, c, h * w), 2).min() / u0.abs().max())
        out["near_zero"] = float((ref.pre.abs() <= MARGIN * ref.pre.abs().max()).double().mean())
        out["ca_mid"], out["sa_mid"] = mid(ref.ca), mid(ref.sa)
        out["positive"] = float((ref.pre > 0).double().mean())
    elif case.kind == "gate":
        g1, x1 = gate_inputs(b.up.to(dtype), b.skip.to(dtype), P)
        ref = gate(g1, x1, b.skip.to(dtype), P, case.training)
        out["near_zero"] = float((ref.pre.abs() <= MARGIN * ref.pre.abs().max()).double().mean())
        out["sa_mid"] = mid(ref.sig)
        out["positive"] = float((ref.pre > 0).double().mean())
    elif case.kind == "ca":
        x = b.x.to(dtype)
        n, c, h, w = x.shape
        ref = channel_attention(x, P["fc.0.weight"], P["fc.2.weight"])
        m = top2_margin(x.reshape(n, c, h * w), 2)
        if b.ties is not None:
            out["tie_exact"] = bool((m[:, b.ties] == 0).all()) and bool((ref.idx[:, b.ties] == h * w // 3).all())
            m[:, b.ties] = float("inf")
        out["sp_margin"] = float(m.min() / x.abs().max())
        out["ca_mid"] = mid(ref.ca)
    else:
        x = b.x.to(dtype)
        n, c, h, w = x.shape
        ref = spatial_attention(x, P["conv1.weight"])
        m = top2_margin(x, 1).reshape(-1)
        if b.ties is not None:
            out["tie_exact"] = bool((m[b.ties] == 0).all()) and bool((ref.amax.reshape(-1)[b.ties] == c // 4).all())
            m[b.ties] = float("inf")
        out["ch_margin"] = float(m.min() / x.abs().max())
        out["sa_mid"] = mid(ref.sa)
    return out


def conditions_hold(fig):
    """-> list of the conditions that fail (empty: the case is usable)"""
    bad = []
    for k in ("ch_margin", "sp_margin"):
        if k in fig and not fig[k] >= MARGIN:
            bad.append(f"{k} {fig[k]:.2e} < {MARGIN:.0e}")
    if "near_zero" in fig and not fig["near_zero"] <= 2e-4:
        bad.append(f"near_zero {fig['near_zero']:.2e} > 2e-4")
    for k in ("ca_mid", "sa_mid"):
        if k in fig and not fig[k] >= 0.25:
            bad.append(f"{k} {fig[k]:.2f} < 0.25")
    if "positive" in fig and not 0.35 <= fig["positive"] <= 0.65:
        bad.append(f"positive {fig['positive']:.2f} outside [0.35, 0.65]")
    if fig.get("tie_exact") is False:
        bad.append("the planted ties are not exact")
    return bad


# ----------------------------------------------------------------------------- forward + backward in one call (reference and fp32 floor)
def _leaf(t):
    return t.detach().clone().requires_grad_(True)


def _leaves(P, dtype):
    return {k: (_leaf(v.to(dtype)) if v.is_floating_point() and "running" not in k else v.to(dtype) if v.is_floating_point() else v)
            for k, v in P.items()}


TAIL_GRADS = ("bn2.weight", "bn2.bias", "ca.fc.0.weight", "ca.fc.2.weight", "sa.conv1.weight", "shortcut.1.weight", "shortcut.1.bias")
GATE_GRADS = ("psi.0.weight", "psi.0.bias", "psi.1.weight", "psi.1.bias", "W_g.1.weight", "W_g.1.bias", "W_x.1.weight", "W_x.1.bias")


def tail_run(t2, r, P, training, dout, dpool=None, pool_flat=None, relu_mask=None, dtype=torch.float64):
    """tail() forward and backward in `dtype`.  The loss is sum(out * dout) + sum(pooled * dpool); pool_flat (flat h * W + w winners,
    [n,c,h/2,w/2]) replaces max_pool2d's own winners.  -> (forward namespace with `pooled` / `pool_flat` added, {name: gradient}) with the
    gradients of TAIL_GRADS, "dt2" and, with a convolution shortcut, "dr"."""
    Pl = _leaves(P, dtype)
    t2l, rl = _leaf(t2.to(dtype)), _leaf(r.to(dtype))
    ref = tail(t2l, rl, Pl, training, relu_mask)
    loss = (ref.out * dout.to(dtype)).sum()
    ref.pooled = ref.pool_flat = None
    if dpool is not None:
        n, c, h, w = ref.out.shape
        own, own_idx = F.max_pool2d(ref.out, 2, return_indices=True)
        ref.pool_flat = own_idx
        ref.pooled = own if pool_flat is None else torch.gather(ref.out.reshape(n, c, h * w), 2, pool_flat.reshape(n, c, -1)).reshape(own.shape)
        loss = loss + (ref.pooled * dpool.to(dtype)).sum()
    loss.backward()
    grads = {k: Pl[k].grad for k in TAIL_GRADS if k in Pl}
    grads["dt2"] = t2l.grad
    if "shortcut.1.weight" in Pl:
        grads["dr"] = rl.grad
    return ref, grads


def gate_run(g1, x1, skip, P, training, datt, relu_mask=None, dtype=torch.float64):
    """gate() forward and backward (loss sum(att * datt)).  -> (forward namespace, {name: gradient}): GATE_GRADS, "dg1", "dx1", "ds" (the
    gradient of psi.0's output) and the two convolution biases "W_g.0.bias" / "W_x.0.bias", the channel sums of dg1 / dx1."""
    Pl = _leaves(P, dtype)
    g1l, x1l = _leaf(g1.to(dtype)), _leaf(x1.to(dtype))
    ref = gate(g1l, x1l, skip.to(dtype), Pl, training, relu_mask)
    ref.s.retain_grad()
    (ref.att * datt.to(dtype)).sum().backward()
    grads = {k: Pl[k].grad for k in GATE_GRADS}
    grads.update(dg1=g1l.grad, dx1=x1l.grad, ds=ref.s.grad)
    grads["W_g.0.bias"], grads["W_x.0.bias"] = g1l.grad.sum(dim=(0, 2, 3)), x1l.grad.sum(dim=(0, 2, 3))
    # a bias in front of a train-mode BatchNorm has an analytically zero gradient: these three sums cancel to rounding level, and "the tensor's
    # largest magnitude" is noise.  Their errors are measured against the largest per-channel sum of the |terms| instead (what bounds the
    # rounding error of a sum); in eval mode they are ordinary tensors.
    ref.cancel = {}
    if training:
        ref.cancel = {"W_g.0.bias": float(g1l.grad.abs().sum(dim=(0, 2, 3)).max()), "W_x.0.bias": float(x1l.grad.abs().sum(dim=(0, 2, 3)).max()),
                      "psi.0.bias": float(ref.s.grad.abs().sum())}
    return ref, grads


def ca_run(x, P, dy, dtype=torch.float64):
    Pl, xl = _leaves(P, dtype), _leaf(x.to(dtype))
    ref = channel_attention(xl, Pl["fc.0.weight"], Pl["fc.2.weight"])
    (ref.y * dy.to(dtype)).sum().backward()
    return ref, {"dx": xl.grad, "fc.0.weight": Pl["fc.0.weight"].grad, "fc.2.weight": Pl["fc.2.weight"].grad}


def sa_run(x, P, dy, dtype=torch.float64):
    Pl, xl = _leaves(P, dtype), _leaf(x.to(dtype))
    ref = spatial_attention(xl, Pl["conv1.weight"])
    (ref.y * dy.to(dtype)).sum().backward()
    return ref, {"dx": xl.grad, "conv1.weight": Pl["conv1.weight"].grad}


TAIL_FWD = ("s2", "h2", "mean2", "invstd2", "avg", "mx", "tval", "ca", "A", "B", "smap", "sa", "out", "pooled")
GATE_FWD = ("s", "sg", "hg", "mean_g", "invstd_g", "sx", "hx", "mean_x", "invstd_x", "sp", "hp", "mean_p", "invstd_p", "att")


def rel_err(a, b, scale=None):
    """max |a - b| over b's largest magnitude (b: the reference), or over `scale` where given (gate_run's cancelling sums)"""
    b = b.detach().double()
    return float((a.detach().double() - b).abs().max()) / (scale if scale else max(float(b.abs().max()), 1e-300))


def fp32_floor(case):
    """{tensor name: error of the float32 reference against the float64 one, relative to the tensor's largest magnitude}, both started from
    the same float32 inputs of the tail / the gate (as the kernels are) and under the float64 run's ReLU and pooling decisions."""
    b = case.build()
    with torch.no_grad():
        P64 = f64(b.P)
        if case.kind == "tail":
            t2, r = (v.float() for v in tail_inputs(b.x.double(), P64, case.training, b.mask))
        elif case.kind == "gate":
            g1, x1 = (v.float() for v in gate_inputs(b.up.double(), b.skip.double(), P64))
    if case.kind == "tail":
        r64, g64 = tail_run(t2, r, b.P, case.training, b.dout, b.dpool)
        mask = (r64.pre > 0).detach()
        r32, g32 = tail_run(t2, r, b.P, case.training, b.dout, b.dpool, r64.pool_flat, mask, torch.float32)
        fwd = TAIL_FWD
        assert torch.equal(r32.idx, r64.idx) and torch.equal(r32.amax, r64.amax)
    elif case.kind == "gate":
        datt = b.dcat[:, :case.shape[3]]
        r64, g64 = gate_run(g1, x1, b.skip, b.P, case.training, datt)
        r32, g32 = gate_run(g1, x1, b.skip, b.P, case.training, datt, (r64.pre > 0).detach(), torch.float32)
        fwd = GATE_FWD
    elif case.kind == "ca":
        (r64, g64), (r32, g32) = ca_run(b.x, b.P, b.dy), ca_run(b.x, b.P, b.dy, torch.float32)
        fwd = ("y", "avg", "mx", "ca")
    else:
        (r64, g64), (r32, g32) = sa_run(b.x, b.P, b.dy), sa_run(b.x, b.P, b.dy, torch.float32)
        fwd = ("y", "smap", "sa")
    out = {k: rel_err(getattr(r32, k), getattr(r64, k)) for k in fwd if getattr(r64, k) is not None}
    out.update({"grad " + k: rel_err(g32[k], g64[k], getattr(r64, "cancel", {}).get(k)) for k in g64})
    return out
