"""Forward / backward of the Robust U-Net building blocks as explicit kernel sequences.

Every function here takes NHWC fp32 device tensors (see ops.ld) and calls the C ABI directly;
the backward functions consume the context returned by the matching forward.  No autograd,
no torch compute ops: torch only allocates device memory.  model.py wraps these in
autograd.Functions so that `loss.backward()` on the drop-in nn.Module works.

Reference semantics: /root/reference/Main_Final.py ResidualBlock :151-196, DilatedBlock :199-223,
AttentionGate :120-148 + ConvTranspose2d + torch.cat :301-303, outc :274-277, MaxPool2d :235.
"""
from __future__ import annotations

import os

import torch

from . import ops
from ._lib import check, lib

BN_EPS = 1e-5
BN_MOMENTUM = 0.1


class Small:
    """Carves small per-channel scratch vectors out of pooled device buffers (fewer allocator calls)."""

    CHUNK = 1 << 16

    def __init__(self, device):
        self.device = device
        self.buf = None
        self.off = 0

    def _take(self, n, dtype):
        n4 = (n + 3) // 4 * 4
        if n4 > self.CHUNK:
            return torch.empty(n, device=self.device, dtype=dtype)
        if self.buf is None or self.off + n4 > self.CHUNK:
            self.buf = torch.empty(self.CHUNK, device=self.device, dtype=torch.float32)
            self.off = 0
        t = self.buf[self.off:self.off + n]
        self.off += n4
        return t if dtype == torch.float32 else t.view(dtype)

    def f(self, n):
        return self._take(n, torch.float32)

    def i(self, n):
        return self._take(n, torch.int32)


_scratch = {}


def scratch(nfloats, device):
    """Reduction workspace (partials) per device AND stream (forward branches / weight gradients run beside the main chain); grows monotonically."""
    return ops.grow(_scratch, (device.index, ops.stream()), nfloats, device, 1 << 21)


def _ws(n, hw, c, device):
    return scratch(lib.runet_reduce_workspace_floats(n, hw, c), device)


_zero_vec = {}


def zeros(n, device):
    """Read-only vector of zeros (eval-mode BatchNorm backward: the batch-statistics terms of dx vanish)."""
    buf = _zero_vec.get(device.index)
    if buf is None or buf.numel() < n:
        buf = torch.zeros(max(int(n), 4096), device=device, dtype=torch.float32)
        _zero_vec[device.index] = buf
    return buf


class DictSink:
    """Default gradient sink: fresh device tensors, collected in a dict keyed by parameter name."""

    def __init__(self, device):
        self.device = device
        self.g = {}

    def buf(self, prefix, items):
        """items: [(param name, physical shape)] laid out back to back -> flat float32 view over all of them."""
        total = sum(_numel(sh) for _, sh in items)
        flat = torch.empty(total, device=self.device, dtype=torch.float32)
        off = 0
        for name, sh in items:
            n = _numel(sh)
            self.g[prefix + name] = flat[off:off + n].view(sh)
            off += n
        return flat


def _numel(shape):
    n = 1
    for d in shape:
        n *= d
    return n


class BNState:
    """Physical handles of one BatchNorm2d (parameters + buffers)."""
    __slots__ = ("weight", "bias", "running_mean", "running_var", "nbt")

    def __init__(self, weight, bias, running_mean, running_var, nbt):
        self.weight, self.bias, self.running_mean, self.running_var, self.nbt = weight, bias, running_mean, running_var, nbt


FUSED_BN_STATS = os.environ.get("RUNET_BN_STATS_3", "0") != "1"      # RUNET_BN_STATS_3=1: statistics / combine / finalize as three launches


def bn_coeff(x, bn: BNState, training, sm: Small, want_minmax=False, stats_hook=None, fused=None):
    """Batch (training) or running (eval) statistics -> (scale, shift, save_mean, save_invstd[, per-(n,c) stats]).
    fused: the dict the producing convolution filled (ops.conv_fwd(stats=...)): its epilogue already holds (count, mean, M2) partials of x."""
    n, h, w, c = x.shape
    hw = h * w
    st = ops.stream()
    scale, shift, mean, invstd = sm.f(c), sm.f(c), sm.f(c), sm.f(c)
    nc = None
    if training and not want_minmax and stats_hook is None and FUSED_BN_STATS and fused and "part" in fused:
        check(lib.runet_bn_stats_finalize(fused["part"].data_ptr(), fused["nparts"], c, bn.weight.data_ptr(), bn.bias.data_ptr(),
                                          bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.nbt.data_ptr(), BN_MOMENTUM, BN_EPS,
                                          scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), invstd.data_ptr(), st))
        return scale, shift, mean, invstd, None
    if training and not want_minmax and stats_hook is None and FUSED_BN_STATS:
        # no per-image statistics wanted: partials -> batch statistics -> coefficients in two launches
        check(lib.runet_bn_stats(x.data_ptr(), ops.ld(x), n, hw, c, _ws(n, hw, c, x.device).data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(),
                                 bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.nbt.data_ptr(), BN_MOMENTUM, BN_EPS,
                                 scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), invstd.data_ptr(), st))
        return scale, shift, mean, invstd, None
    if training or want_minmax:
        mean_nc, m2_nc = sm.f(n * c), sm.f(n * c)
        if want_minmax:
            max_nc, min_nc, imax, imin = sm.f(n * c), sm.f(n * c), sm.i(n * c), sm.i(n * c)
            nc = (mean_nc, m2_nc, max_nc, min_nc, imax, imin)
        ws = _ws(n, hw, c, x.device)
        check(lib.runet_chan_stats(x.data_ptr(), ops.ld(x), n, hw, c, ws.data_ptr(), mean_nc.data_ptr(), m2_nc.data_ptr(),
                                   nc[2].data_ptr() if nc else None, nc[3].data_ptr() if nc else None,
                                   nc[4].data_ptr() if nc else None, nc[5].data_ptr() if nc else None, int(want_minmax), st))
        mean_all, m2_all, n_eff = mean_nc, m2_nc, n
        if stats_hook is not None and training:   # SyncBN: every rank's per-image (mean, M2) rows, Chan-combined by bn_finalize
            mean_all, m2_all, n_eff = stats_hook.gather_stats(mean_nc, m2_nc, n, c)
    if training:
        check(lib.runet_bn_finalize(mean_all.data_ptr(), m2_all.data_ptr(), n_eff, c, hw, bn.weight.data_ptr(), bn.bias.data_ptr(),
                                    bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.nbt.data_ptr(), BN_MOMENTUM, BN_EPS, 1,
                                    scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), invstd.data_ptr(), st))
    else:
        check(lib.runet_bn_finalize(None, None, n, c, hw, bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(),
                                    bn.running_var.data_ptr(), None, BN_MOMENTUM, BN_EPS, 0, scale.data_ptr(), shift.data_ptr(),
                                    mean.data_ptr(), invstd.data_ptr(), st))
    return scale, shift, mean, invstd, nc


def bn_coeff_pair(xa, bna: BNState, xb, bnb: BNState, training, sm: Small, stats_hook=None):
    """Two BatchNorms whose inputs are ready at the same point of the pass.  Under SyncBN their per-image statistics travel in ONE
    all-gather (the messages are latency-bound: a ResidualBlock's shortcut with its bn1, an attention gate's W_g with its W_x); otherwise
    two plain bn_coeff calls.  -> ((scale, shift, mean, invstd) of a, the same of b)"""
    if stats_hook is None or not training:
        return bn_coeff(xa, bna, training, sm)[:4], bn_coeff(xb, bnb, training, sm)[:4]
    st = ops.stream()
    local = []
    for x in (xa, xb):
        n, h, w, c = x.shape
        mean_nc, m2_nc = sm.f(n * c), sm.f(n * c)
        check(lib.runet_chan_stats(x.data_ptr(), ops.ld(x), n, h * w, c, _ws(n, h * w, c, x.device).data_ptr(), mean_nc.data_ptr(), m2_nc.data_ptr(),
                                   None, None, None, None, 0, st))
        local.append((mean_nc, m2_nc, n, c))
    res = []
    for x, bn, (mean_all, m2_all, n_eff) in zip((xa, xb), (bna, bnb), stats_hook.gather_stats_many(local)):
        n, h, w, c = x.shape
        scale, shift, mean, invstd = sm.f(c), sm.f(c), sm.f(c), sm.f(c)
        check(lib.runet_bn_finalize(mean_all.data_ptr(), m2_all.data_ptr(), n_eff, c, h * w, bn.weight.data_ptr(), bn.bias.data_ptr(),
                                    bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.nbt.data_ptr(), BN_MOMENTUM, BN_EPS, 1,
                                    scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), invstd.data_ptr(), st))
        res.append((scale, shift, mean, invstd))
    return res[0], res[1]


def bn_apply(x, scale, shift, mask=None, relu=False, out=None):
    n, h, w, c = x.shape
    if out is None:
        out = ops.empty_nhwc(n, h, w, c, x)
    check(lib.runet_bn_apply(x.data_ptr(), ops.ld(x), out.data_ptr(), ops.ld(out), n * h * w, h * w, c, scale.data_ptr(), shift.data_ptr(),
                             mask.data_ptr() if mask is not None else None, int(relu), ops.stream()))
    return out


def bn_bwd_reduce(dy, x, mean, invstd, scale, sums, act=None, mask=None, relu_shift=None):
    """First half of bn_backward: the LOCAL (dgamma | dbeta) sums into `sums` [2c]."""
    n, h, w, c = x.shape
    hw = h * w
    if relu_shift is not None:
        act = None
    actp, lda = (act.data_ptr(), ops.ld(act)) if act is not None else (None, 0)
    rsc, rsh = (scale.data_ptr(), relu_shift.data_ptr()) if relu_shift is not None else (None, None)
    check(lib.runet_bn_bwd_reduce(dy.data_ptr(), ops.ld(dy), x.data_ptr(), ops.ld(x), actp, lda, n, hw, c, mean.data_ptr(), invstd.data_ptr(),
                                  mask.data_ptr() if mask is not None else None, _ws(n, hw, c, x.device).data_ptr(), sums.data_ptr(), rsc, rsh,
                                  ops.stream()))


def bn_bwd_apply(dy, x, mean, invstd, scale, use, m_total, act=None, mask=None, out=None, relu_shift=None):
    """Second half: dx from the sums `use` that enter it (local, all-reduced with the global element count m_total, or zeros in eval mode)."""
    n, h, w, c = x.shape
    hw = h * w
    if relu_shift is not None:
        act = None
    actp, lda = (act.data_ptr(), ops.ld(act)) if act is not None else (None, 0)
    if out is None:
        out = ops.empty_nhwc(n, h, w, c, x)
    check(lib.runet_bn_bwd_apply(dy.data_ptr(), ops.ld(dy), x.data_ptr(), ops.ld(x), actp, lda, out.data_ptr(), ops.ld(out), n * hw, hw, c,
                                 mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(), use.data_ptr(), mask.data_ptr() if mask is not None else None,
                                 m_total, relu_shift.data_ptr() if relu_shift is not None else None, ops.stream()))
    return out


def dx_sums(sums, training, sync=None, count=0):
    """Which sums enter a BatchNorm backward's dx, given its LOCAL (dgamma | dbeta) sums over `count` elements -> (use, m_total): zeros in eval
    mode (the batch-statistics terms vanish); the local sums with m_total 0 (the kernel divides by its own element count); or, under SyncBN,
    the all-reduced sums with the global count."""
    if not training:
        return zeros(sums.numel(), sums.device), 0
    return (sums, 0) if sync is None else sync.reduce_sums(sums, count)


def bn_backward(dy, x, mean, invstd, scale, sums, act=None, mask=None, out=None, sync=None, relu_shift=None, training=True):
    """sums: [2c] destination for (dgamma | dbeta), always the LOCAL sums.  act/mask: fused relu(+dropout) backward from the saved
    activation; relu_shift (the forward's shift vector, with `scale` the forward's scale): the same from x alone, act is not read.
    sync (SyncBN): dx uses the all-reduced sums and the global element count.  training=False (the forward normalised with the
    RUNNING statistics, `mean` / `invstd` are those): BatchNorm is a per-channel affine map, dx = dy * scale with no batch-statistics
    terms, while dgamma / dbeta keep their form (sums over dy * xhat and dy).  -> dx"""
    n, h, w, c = x.shape
    bn_bwd_reduce(dy, x, mean, invstd, scale, sums, act, mask, relu_shift)
    use, m_total = dx_sums(sums, training, sync, n * h * w)
    return bn_bwd_apply(dy, x, mean, invstd, scale, use, m_total, act, mask, out, relu_shift)


CHAN_SUM_ON_SIDE = os.environ.get("RUNET_CHAN_SUM_MAIN", "0") != "1"
# the shortcut BatchNorm's backward sums taken in rb_bwd2 (runet_rb_bwd2_bn) instead of by bn_bwd_reduce(dv, r): one tensor read and one launch
# less per block, but measured SLOWER in the step (A/B 545.0 vs 540.5 img/s: the reduction kernel gets twice the LDS and registers, the pass it
# replaces ran at HBM speed) - opt-in (RUNET_FUSED_SHORTCUT_BN_SUMS=1), kept equal by tests/test_gpu_blocks.py
FUSED_SHORTCUT_BN_SUMS = os.environ.get("RUNET_FUSED_SHORTCUT_BN_SUMS", "0") == "1"
FUSED_GATE_BN_SUMS = os.environ.get("RUNET_NO_FUSED_GATE_BN_SUMS", "0") != "1"      # the attention gates' BatchNorm-backward sums taken in ag_bwd2
# The ResidualBlock's edges folded into its tail kernels (exact: same operations on the same operands, bit-identical results):
#   out   rb_out also writes a ReLU sign byte per 4 channels and, for the encoder blocks, the 2x2 max pool of its output (runet_rb_out_ex)
#   bwd1  rb_bwd1 adds the pooled gradient's term in its load of dout and takes the ReLU mask from the sign bytes (runet_rb_bwd1_ex)
#   bwd3  rb_bwd3 also applies the shortcut BatchNorm's backward, dr written over dv (runet_rb_bwd3_sc)
# RUNET_NO_FUSED_RB_EDGES=1 restores the separate maxpool2_fwd / maxpool2_bwd / bn_bwd_apply launches.  Read at call time.
FUSED_RB_EDGES = os.environ.get("RUNET_NO_FUSED_RB_EDGES", "0") != "1"
RB_EDGE_PARTS = frozenset(("out", "bwd1", "bwd3"))      # tools/rb_edges_step.py narrows this to time one part alone; no other user


def _edge(part):
    return FUSED_RB_EDGES and part in RB_EDGE_PARTS


# The 64 -> 1 output head folded into the tail of the ResidualBlock in front of it (exact, as the edges above; both need them):
#   fwd  rb_out forms the logit and the probability from the values it stores: no outc_fwd launch, no re-read of `out` (runet_rb_out_head)
#   bwd  outc_bwd leaves dl [P] instead of dx [P][C] (runet_outc_bwd_dl); rb_bwd1 forms w[c] * dl[p] in its load (runet_rb_bwd1_rank1)
# RUNET_NO_FUSED_HEAD=1 restores the separate runet_outc_fwd / runet_outc_bwd launches.  Read at call time.
FUSED_HEAD = os.environ.get("RUNET_NO_FUSED_HEAD", "0") != "1"
HEAD_PARTS = frozenset(("fwd", "bwd"))                  # narrowed to time one part alone, as RB_EDGE_PARTS


def fuses_head(part, c):
    """part "fwd": rb_forward(head=...) takes the head along; "bwd": rb_backward(head_grad=...) takes outc_backward_dl's pair"""
    if not (FUSED_HEAD and part in HEAD_PARTS and lib.runet_rb_out_head_supported(c)):      # C = 64; any other width keeps the separate launches
        return False
    return _edge("out") if part == "fwd" else _edge("bwd1")


def chan_sum(x, out):
    """Per-channel sum over all pixels (bias gradients).  Nothing in the backward chain waits for a bias gradient, so inside the backward
    pass (ops.wgrad_side_stream active) the two launches go to the weight-gradient stream like the weight gradients themselves."""
    n, h, w, c = x.shape

    def run():
        ws = _ws(n, h * w, c, x.device)
        check(lib.runet_chan_sum(x.data_ptr(), ops.ld(x), n * h * w, c, ws.data_ptr(), out.data_ptr(), 0, ops.stream()))
        return out
    if CHAN_SUM_ON_SIDE and ops.side_stream() is not None:
        return ops._on_side(run, (x, out))
    return run()


def vec(n, device):
    return torch.empty(n, device=device, dtype=torch.float32)


def _ptr(t):
    return t.data_ptr() if t is not None else None


# ------------------------------------------------------------------------------- Conv2d -> BatchNorm2d -> ReLU (the baselines' step)
def conv_bn_coeff(x, w, bias, bn: BNState, training, sm: Small, stride=1, stats=True, save=True):
    """Conv2d (w HWIO, padding k // 2; stride 1 through ops.conv_fwd, stride 2 through ops.conv_general_fwd) and the coefficients of the
    BatchNorm2d behind it.  stats: take the batch statistics from the convolution's epilogue where the kernel offers them (another
    summation order than bn_coeff's own pass: a call site keeps its choice).
    -> (t = conv x, scale, shift, the context conv_bn_relu_backward reads or None)"""
    fs = None
    if stride == 1:
        fs = {} if (stats and training) else None
        t = ops.conv_fwd(x, w, bias, stats=fs)
    else:
        t = ops.conv_general_fwd(x, w, bias, stride, w.shape[0] // 2)
    s, h, mean, invstd, _ = bn_coeff(t, bn, training, sm, fused=fs)
    return t, s, h, (dict(x=x, w=w, t=t, s=s, h=h, mean=mean, invstd=invstd, stride=stride) if save else None)


def conv_bn_relu_forward(x, w, bias, bn: BNState, training, sm: Small, stride=1, stats=True, save=True, out=None):
    """-> (relu(bn(conv x)), written to `out` - a concat slice - when given; context or None)"""
    t, s, h, cx = conv_bn_coeff(x, w, bias, bn, training, sm, stride, stats, save)
    return bn_apply(t, s, h, None, relu=True, out=out), cx


def conv_bn_relu_backward(cx, dy, G, seq, i, training, out=None):
    """dy: gradient of the activation.  The parameter gradients go into G (physical layouts) as {seq}.{i}.weight / .bias (the convolution;
    on the weight-gradient stream) and {seq}.{i + 1}.weight / .bias (the BatchNorm).  out: where the BatchNorm backward writes (out=dy: in
    place).  -> dt, the gradient of the convolution's output; the data gradient is the caller's"""
    k, _, cin_w, c = cx["w"].shape
    sums = vec(2 * c, dy.device)
    dt = bn_backward(dy, cx["t"], cx["mean"], cx["invstd"], cx["s"], sums, relu_shift=cx["h"], out=out, training=training)
    G[f"{seq}.{i + 1}.weight"], G[f"{seq}.{i + 1}.bias"] = sums[:c], sums[c:]
    if cx["stride"] == 1:
        G[f"{seq}.{i}.weight"] = ops.conv_wgrad(cx["x"], dt, k, k, cin_w=cin_w)
    else:
        G[f"{seq}.{i}.weight"] = ops.conv_general_wgrad(cx["x"], dt, k, k, cx["stride"], k // 2, cin_w=cin_w)
    G[f"{seq}.{i}.bias"] = chan_sum(dt, vec(c, dy.device))
    return dt


# =============================================================================== ResidualBlock
class RBParams:
    __slots__ = ("w1", "bn1", "w2", "bn2", "w0p", "w2p", "wsa", "ws", "bns", "cin_w")

    def __init__(self, w1, bn1, w2, bn2, w0p, w2p, wsa, ws=None, bns=None):
        self.w1, self.bn1, self.w2, self.bn2, self.w0p, self.w2p, self.wsa, self.ws, self.bns = w1, bn1, w2, bn2, w0p, w2p, wsa, ws, bns
        self.cin_w = w1.shape[2]


def rb_forward(x, p: RBParams, training, mask=None, save=True, stats_hook=None, pool=False, head=None):
    """x: [N,H,W,Cx] with Cx >= cin_w (stem: RGB zero-padded to 4).  -> (out [N,H,W,C], ctx or None)
    pool: the block feeds MaxPool2d(2) -> (out, ctx, pooled [N,H/2,W/2,C], winner bytes); ctx keeps the bytes as "pool_idx".
    head: dict(w=, b=, want_logit=) of the 64 -> 1 output head behind the block (the caller asked fuses_head("fwd", C)): receives "prob" and
    "logit" (or None), what outc_forward(out, w, b, want_logit) returns."""
    n, h, w, _ = x.shape
    c = p.w1.shape[3]
    cr = p.w0p.shape[3]
    hw, P = h * w, n * h * w
    st = ops.stream()
    sm = Small(x.device)
    kv1, kv2 = ({}, {}) if save else (None, None)      # F(4x4) layers: the transformed inputs are kept for the weight gradients
    t1, br, fstem = None, None, (None, None)
    if p.ws is not None:
        if ops._stem_case(x.shape[3], p.cin_w, c, 3) and p.ws.shape[2] == p.cin_w:
            fstem = ({}, {}) if (training and stats_hook is None) else (None, None)
            t1, r = ops.stem_conv(x, p.w1, p.ws, stats3=fstem[0], stats1=fstem[1])       # RGB stem: conv1 and the shortcut convolution in one launch
            if stats_hook is None:
                ss, hs, mean_s, invstd_s, _ = bn_coeff(r, p.bns, training, sm, fused=fstem[1])
        elif stats_hook is not None:
            r = ops.conv_fwd(x, p.ws)                  # SyncBN: no branch; the shortcut's statistics share bn1's message below
        else:
            # the shortcut branch (1x1 convolution + its BatchNorm statistics) runs beside conv1 .. the attention maps, joins at rb_out
            sm.f(4)                                    # the arena's buffer is allocated on the main stream
            r = ops.main_pool(ops.empty_nhwc(n, h, w, c, x))          # ... and so is the branch's result (side_branch.join)
            br = ops.side_branch(stats_hook is None)
            with br:
                fs = {} if training else None
                ops.conv_fwd(x, p.ws, out=r, stats=fs)
                ss, hs, mean_s, invstd_s, _ = bn_coeff(r, p.bns, training, sm, fused=fs)
    else:
        r, ss, hs, mean_s, invstd_s = x, None, None, None, None
    f1 = {} if (training and stats_hook is None) else None
    if t1 is None:
        t1 = ops.conv_fwd(x, p.w1, keep_v=kv1, stats=f1)
    elif fstem[0]:
        f1 = fstem[0]                              # the stem kernel took bn1's statistics in its epilogue
    if p.ws is not None and stats_hook is not None:
        (ss, hs, mean_s, invstd_s), (s1, h1, mean1, invstd1) = bn_coeff_pair(r, p.bns, t1, p.bn1, training, sm, stats_hook)
    else:
        s1, h1, mean1, invstd1, _ = bn_coeff(t1, p.bn1, training, sm, stats_hook=stats_hook, fused=f1)
    use_mask = mask if training else None
    if ops.fuses_act_input(t1, p.w2):
        # conv2 on the F(4x4) path: BatchNorm + ReLU + Dropout2d ride in its input transform's loads, a1 is never written (rb_a1 recomputes it
        # for whoever wants to look at it); the backward pass needs t1 and the kept V only
        a1 = None
        t2 = ops.conv_fwd(t1, p.w2, keep_v=kv2, pre=(s1, h1, use_mask))
    else:
        a1 = bn_apply(t1, s1, h1, use_mask, relu=True)
        t2 = ops.conv_fwd(a1, p.w2, keep_v=kv2)
    if not save:
        del t1
    s2, h2, mean2, invstd2, nc = bn_coeff(t2, p.bn2, training, sm, want_minmax=True, stats_hook=stats_hook)
    mean_nc, _, max_nc, min_nc, imax, imin = nc
    A, B, ca, avg, mx, tval = (sm.f(n * c) for _ in range(6))
    idx = sm.i(n * c)
    check(lib.runet_ca_coeff(mean_nc.data_ptr(), max_nc.data_ptr(), min_nc.data_ptr(), imax.data_ptr(), imin.data_ptr(), s2.data_ptr(),
                             h2.data_ptr(), p.w0p.data_ptr(), p.w2p.data_ptr(), n, c, cr, A.data_ptr(), B.data_ptr(), ca.data_ptr(),
                             avg.data_ptr(), mx.data_ptr(), idx.data_ptr(), tval.data_ptr(), st))
    smap = torch.empty((P, 2), device=x.device, dtype=torch.float32)
    amax = torch.empty(P, device=x.device, dtype=torch.int32)
    check(lib.runet_sa_reduce(t2.data_ptr(), ops.ld(t2), A.data_ptr(), B.data_ptr(), P, hw, c, smap.data_ptr(), amax.data_ptr(), st))
    sa = torch.empty(P, device=x.device, dtype=torch.float32)
    check(lib.runet_sa_conv7(smap.data_ptr(), p.wsa.data_ptr(), sa.data_ptr(), n, h, w, st))
    out = ops.empty_nhwc(n, h, w, c, x)
    if br is not None:
        br.join(r)
    relu_bits = pooled = pool_idx = None
    if _edge("out"):
        if save and _edge("bwd1"):
            relu_bits = torch.empty((P, c // 4), device=x.device, dtype=torch.uint8)
        if pool:
            pooled = ops.empty_nhwc(n, h // 2, w // 2, c, x)
            pool_idx = torch.empty((n, h // 2, w // 2, c), device=x.device, dtype=torch.uint8)
    if head is not None:
        assert not pool and fuses_head("fwd", c)
        head["prob"] = torch.empty((n, 1, h, w), device=x.device, dtype=torch.float32)
        head["logit"] = torch.empty((n, 1, h, w), device=x.device, dtype=torch.float32) if head["want_logit"] else None
        check(lib.runet_rb_out_head(t2.data_ptr(), ops.ld(t2), A.data_ptr(), B.data_ptr(), sa.data_ptr(), r.data_ptr(), ops.ld(r), _ptr(ss), _ptr(hs),
                                    out.data_ptr(), ops.ld(out), _ptr(relu_bits), head["w"].data_ptr(), head["b"].data_ptr(), _ptr(head["logit"]),
                                    head["prob"].data_ptr(), n, h, w, c, st))
    else:
        check(lib.runet_rb_out_ex(t2.data_ptr(), ops.ld(t2), A.data_ptr(), B.data_ptr(), sa.data_ptr(), r.data_ptr(), ops.ld(r), _ptr(ss), _ptr(hs),
                                  out.data_ptr(), ops.ld(out), _ptr(relu_bits), _ptr(pooled), ops.ld(pooled) if pooled is not None else 0,
                                  _ptr(pool_idx), n, h, w, c, st))
    if pool and pooled is None:
        pooled, pool_idx = maxpool_forward(out)
    if not save:
        return (out, None, pooled, pool_idx) if pool else (out, None)
    ctx = dict(x=x, r=r, t1=t1, a1=a1, t2=t2, out=out, mask=use_mask, p=p, training=training, sync=stats_hook if training else None, s1=s1, h1=h1, mean1=mean1, invstd1=invstd1, s2=s2, h2=h2,
               mean2=mean2, invstd2=invstd2, ss=ss, mean_s=mean_s, invstd_s=invstd_s, A=A, B=B, ca=ca, avg=avg, mx=mx, idx=idx,
               tval=tval, mean_nc=mean_nc, smap=smap, amax=amax, sa=sa, v1=kv1.get("V"), v2=kv2.get("V"), relu_bits=relu_bits, pool_idx=pool_idx)
    return (out, ctx, pooled, pool_idx) if pool else (out, ctx)


def rb_a1(ctx):
    """The activation between conv1 and conv2, relu(bn1(conv1 x)) * dropout mask: saved, or - where conv2's input transform produced it on the
    fly (rb_forward) - evaluated by the same expression (bn_apply_kernel and the fused transform share bn_pre: identical bits)."""
    if ctx["a1"] is not None:
        return ctx["a1"]
    return bn_apply(ctx["t1"], ctx["s1"], ctx["h1"], ctx["mask"], relu=True)


def rb_backward(ctx, dout, sink, pre="", need_dx=True, dpool=None, pool_idx=None, head_grad=None):
    """Parameter gradients go to `sink` (names prefixed with `pre`).  -> dx or None
    dpool, pool_idx: the gradient of the block's pooled output and the pool's winner bytes; the block's incoming gradient is then
    dout + maxpool_backward(dpool, pool_idx).  dout is left unmodified unless the edges are unfused (it is then accumulated into).
    head_grad: (dl [P], w [C]) of outc_backward_dl in place of dout (None): the incoming gradient is w[c] * dl[p], formed in rb_bwd1's load."""
    p: RBParams = ctx["p"]
    x, r, t1, a1, t2, out = ctx["x"], ctx["r"], ctx["t1"], ctx["a1"], ctx["t2"], ctx["out"]
    n, h, w, c = out.shape
    cr = p.w0p.shape[3]
    hw, P = h * w, n * h * w
    st = ops.stream()
    dev = x.device
    sm = Small(dev)
    A, B, sa, smap, amax = ctx["A"], ctx["B"], ctx["sa"], ctx["smap"], ctx["amax"]
    dv = ops.empty_nhwc(n, h, w, c, x)
    dq = torch.empty(P, device=dev, dtype=torch.float32)
    relu_bits = ctx.get("relu_bits") if _edge("bwd1") else None
    if dpool is not None and not _edge("bwd1"):
        dout, dpool = maxpool_backward(dpool, pool_idx, dx=dout), None
    if head_grad is not None:
        assert dout is None and dpool is None and relu_bits is not None
        check(lib.runet_rb_bwd1_rank1(head_grad[0].data_ptr(), head_grad[1].data_ptr(), relu_bits.data_ptr(), t2.data_ptr(), ops.ld(t2), A.data_ptr(),
                                      B.data_ptr(), sa.data_ptr(), dv.data_ptr(), ops.ld(dv), dq.data_ptr(), n, h, w, c, st))
    else:
        check(lib.runet_rb_bwd1_ex(dout.data_ptr(), ops.ld(dout), _ptr(dpool), ops.ld(dpool) if dpool is not None else 0,
                                   pool_idx.data_ptr() if dpool is not None else None, out.data_ptr(), ops.ld(out), _ptr(relu_bits), t2.data_ptr(),
                                   ops.ld(t2), A.data_ptr(), B.data_ptr(), sa.data_ptr(), dv.data_ptr(), ops.ld(dv), dq.data_ptr(), n, h, w, c, st))
    dsm = torch.empty((P, 2), device=dev, dtype=torch.float32)
    dwsa = sink.buf(pre, [("sa.conv1.weight", (7, 7, 2, 1))])
    ws = scratch(lib.runet_sa_conv7_bwd_workspace_floats(n, h, w), dev)
    check(lib.runet_sa_conv7_bwd(smap.data_ptr(), dq.data_ptr(), p.wsa.data_ptr(), dsm.data_ptr(), dwsa.data_ptr(), ws.data_ptr(), n, h, w, st))
    sdu, sdut = sm.f(n * c), sm.f(n * c)
    sync, tr = ctx["sync"], ctx["training"]
    # The shortcut BatchNorm's backward (blocks with a convolution shortcut: dv, final since rb_bwd1, is its incoming gradient and r its input)
    # is decided here, once:
    #   sc_sums  where its local sums come from - "bwd2": runet_rb_bwd2_bn takes them in its pass over dv (one read of r instead of a pass
    #            over dv and r); "early" / "late": bn_bwd_reduce(dv, r), in front of rb_bwd3 when something there waits for the sums (bn2's
    #            all-reduce, which they share under SyncBN, or rb_bwd3_sc), else behind conv1's gradients
    #   sc_bwd3  where dr is produced - inside runet_rb_bwd3_sc, written over dv (training mode), or by bn_bwd_apply behind conv1's gradients
    has_sc = p.ws is not None
    synced = sync is not None and tr
    sc_bwd3 = has_sc and tr and _edge("bwd3")
    sc_sums = None if not has_sc else "bwd2" if (FUSED_SHORTCUT_BN_SUMS and not synced) else "early" if (synced or sc_bwd3) else "late"
    sums_s = sink.buf(pre, [("shortcut.1.weight", (c,)), ("shortcut.1.bias", (c,))]) if has_sc else None

    def sc_reduce():
        bn_bwd_reduce(dv, r, ctx["mean_s"], ctx["invstd_s"], ctx["ss"], sums_s)

    if sc_sums == "bwd2":
        ws = scratch(lib.runet_rb_bwd2_bn_workspace_floats(n, hw, c), dev)
        check(lib.runet_rb_bwd2_bn(dv.data_ptr(), ops.ld(dv), t2.data_ptr(), ops.ld(t2), sa.data_ptr(), dsm.data_ptr(), amax.data_ptr(), r.data_ptr(),
                                   ops.ld(r), ctx["mean_s"].data_ptr(), ctx["invstd_s"].data_ptr(), n, hw, c, ws.data_ptr(), ws.numel(),
                                   sdu.data_ptr(), sdut.data_ptr(), sums_s.data_ptr(), st))
    else:
        ws = _ws(n, hw, c, dev)
        check(lib.runet_rb_bwd2(dv.data_ptr(), ops.ld(dv), t2.data_ptr(), ops.ld(t2), sa.data_ptr(), dsm.data_ptr(), amax.data_ptr(), n, hw, c,
                                ws.data_ptr(), sdu.data_ptr(), sdut.data_ptr(), st))
    davg, dmx = sm.f(n * c), sm.f(n * c)
    sums2 = sink.buf(pre, [("bn2.weight", (c,)), ("bn2.bias", (c,))])
    dw0p = sink.buf(pre, [("ca.fc.0.weight", (1, 1, c, cr))])
    dw2p = sink.buf(pre, [("ca.fc.2.weight", (1, 1, cr, c))])
    ws = scratch(lib.runet_ca_bwd_workspace_floats(n, c, cr), dev)
    check(lib.runet_ca_bwd(sdu.data_ptr(), sdut.data_ptr(), ctx["s2"].data_ptr(), ctx["h2"].data_ptr(), ctx["ca"].data_ptr(),
                           ctx["avg"].data_ptr(), ctx["mx"].data_ptr(), p.w0p.data_ptr(), p.w2p.data_ptr(), ctx["mean_nc"].data_ptr(),
                           ctx["tval"].data_ptr(), ctx["mean2"].data_ptr(), ctx["invstd2"].data_ptr(), n, c, cr, ws.data_ptr(),
                           davg.data_ptr(), dmx.data_ptr(), sums2.data_ptr(), dw0p.data_ptr(), dw2p.data_ptr(), st))
    dt2 = ops.empty_nhwc(n, h, w, c, x)
    if sc_sums == "early":
        sc_reduce()
    if has_sc and synced:                    # SyncBN: the shortcut BatchNorm's sums share bn2's all-reduce
        (use2, m_total), (use_s, m_s) = sync.reduce_sums_many([sums2, sums_s], [P, P])
    else:
        use2, m_total = dx_sums(sums2, tr, sync, P)
        # use_s is chosen here and read later: in training mode it IS sums_s, which a "late" reduce fills only behind conv1's gradients
        use_s, m_s = dx_sums(sums_s, tr) if has_sc else (None, 0)
    if sc_bwd3:
        check(lib.runet_rb_bwd3_sc(dv.data_ptr(), ops.ld(dv), t2.data_ptr(), ops.ld(t2), sa.data_ptr(), dsm.data_ptr(), amax.data_ptr(),
                                   ctx["ca"].data_ptr(), davg.data_ptr(), dmx.data_ptr(), ctx["idx"].data_ptr(), ctx["mean2"].data_ptr(),
                                   ctx["invstd2"].data_ptr(), ctx["s2"].data_ptr(), use2.data_ptr(), dt2.data_ptr(), ops.ld(dt2), r.data_ptr(),
                                   ops.ld(r), ctx["mean_s"].data_ptr(), ctx["invstd_s"].data_ptr(), ctx["ss"].data_ptr(), use_s.data_ptr(), m_s,
                                   P, hw, c, m_total, st))
    else:
        check(lib.runet_rb_bwd3(dv.data_ptr(), ops.ld(dv), t2.data_ptr(), ops.ld(t2), sa.data_ptr(), dsm.data_ptr(), amax.data_ptr(),
                                ctx["ca"].data_ptr(), davg.data_ptr(), dmx.data_ptr(), ctx["idx"].data_ptr(), ctx["mean2"].data_ptr(),
                                ctx["invstd2"].data_ptr(), ctx["s2"].data_ptr(), use2.data_ptr(), dt2.data_ptr(), ops.ld(dt2), P, hw, c, m_total, st))
    # the data gradient first: on the adjoint F(4x4) path it leaves Z = A dy A^T behind, which the weight gradient (side stream) reuses
    kz = {}
    da1 = ops.conv_dgrad(dt2, p.w2, keep_z=kz)
    if a1 is None:
        assert ctx.get("v2") is not None, "conv2 took its activation on the fly: its weight gradient needs the kept V"
        a1 = t1                                        # shape only: the weight gradient reads V
    ops.conv_wgrad(a1, dt2, 3, 3, out=sink.buf(pre, [("conv2.weight", (3, 3, c, c))]), v=ctx.get("v2"), z=kz.get("Z"))
    ctx["v2"] = None
    del dt2, kz
    sums1 = sink.buf(pre, [("bn1.weight", (c,)), ("bn1.bias", (c,))])
    kz1, dx1 = {}, None
    fused_dt1 = need_dx and p.cin_w == x.shape[3] and ops.fuses_bn_bwd_input(da1, p.w1)
    if fused_dt1:
        # conv1 on the adjoint F(4x4) path: the BatchNorm-backward dx rides in the loads of Z = A dt1 A^T, which both of conv1's gradients read
        # - dt1 itself is never written (two passes over the tensor and one launch less)
        bn_bwd_reduce(da1, t1, ctx["mean1"], ctx["invstd1"], ctx["s1"], sums1, None, ctx["mask"], ctx["h1"])
        use1, m1 = dx_sums(sums1, tr, sync, P)
        bn1 = dict(x=t1, mean=ctx["mean1"], invstd=ctx["invstd1"], scale=ctx["s1"], shift=ctx["h1"], sums=use1, m_total=m1, mask=ctx["mask"])
        if p.ws is not None:
            dx1 = ops.conv_dgrad(da1, p.w1, keep_z=kz1, bn=bn1)
        else:
            dx1 = ops.conv_dgrad(da1, p.w1, out=dv, accumulate=True, keep_z=kz1, bn=bn1)
        dt1 = da1                                      # shape only: the weight gradient reads Z
    else:
        dt1 = bn_backward(da1, t1, ctx["mean1"], ctx["invstd1"], ctx["s1"], sums1, mask=ctx["mask"], out=da1, sync=sync, relu_shift=ctx["h1"], training=tr)
        # the first block of the network (need_dx False) ends the backward chain: nothing is left on the main stream to overlap with, so its
        # last weight gradient runs there, next to the conv2 weight gradient still on the side stream
        if need_dx and p.ws is not None:
            dx1 = ops.conv_dgrad(dt1, p.w1, keep_z=kz1)
    ops.conv_wgrad(x, dt1, 3, 3, cin_w=p.cin_w, out=sink.buf(pre, [("conv1.weight", (3, 3, p.cin_w, c))]), v=ctx.get("v1"), on_side=need_dx,
                   z=kz1.get("Z"))
    ctx["v1"] = None
    dx = None
    if has_sc:
        if sc_sums == "late":
            sc_reduce()
        dr = dv if sc_bwd3 else bn_bwd_apply(dv, r, ctx["mean_s"], ctx["invstd_s"], ctx["ss"], use_s, m_s, out=dv)
        ops.conv_wgrad(x, dr, 1, 1, cin_w=p.cin_w, out=sink.buf(pre, [("shortcut.0.weight", (1, 1, p.cin_w, c))]))
        if need_dx:
            dx = dx1
            ops.conv_dgrad(dr, p.ws, out=dx, accumulate=True)
    elif need_dx:
        dx = dv
        if not fused_dt1:
            ops.conv_dgrad(dt1, p.w1, out=dx, accumulate=True)
    return dx


# =============================================================================== standalone attention modules
# ChannelAttention (Main_Final.py:82-101) and SpatialAttention (:104-117) called on their own.  Inside ResidualBlock both are fused into
# the block's tail (rb_forward); on their own they are the same kernels with an identity BatchNorm in front (scale 1, shift 0) and
# neutral stand-ins for the other attention (per-pixel factor 1 / per-channel factor 1), so nothing new is computed differently.
def _consts(n, c, P, dev):
    one_c, zero_c = torch.ones(max(2 * c, n * c), device=dev), zeros(max(2 * c, n * c), dev)
    return one_c, zero_c


def ca_forward(x, w0p, w2p, save=True):
    """y = x * sigmoid(mlp(avgpool x) + mlp(maxpool x)).  x NHWC.  -> (y, ctx)"""
    n, h, w, c = x.shape
    cr = w0p.shape[3]
    dev, st = x.device, ops.stream()
    sm = Small(dev)
    mean_nc, m2_nc, max_nc, min_nc = sm.f(n * c), sm.f(n * c), sm.f(n * c), sm.f(n * c)
    imax, imin, idx = sm.i(n * c), sm.i(n * c), sm.i(n * c)
    check(lib.runet_chan_stats(x.data_ptr(), ops.ld(x), n, h * w, c, _ws(n, h * w, c, dev).data_ptr(), mean_nc.data_ptr(), m2_nc.data_ptr(),
                               max_nc.data_ptr(), min_nc.data_ptr(), imax.data_ptr(), imin.data_ptr(), 1, st))
    one, zero = _consts(n, c, 0, dev)
    A, B, ca, avg, mx, tval = (sm.f(n * c) for _ in range(6))
    check(lib.runet_ca_coeff(mean_nc.data_ptr(), max_nc.data_ptr(), min_nc.data_ptr(), imax.data_ptr(), imin.data_ptr(), one.data_ptr(),
                             zero.data_ptr(), w0p.data_ptr(), w2p.data_ptr(), n, c, cr, A.data_ptr(), B.data_ptr(), ca.data_ptr(), avg.data_ptr(),
                             mx.data_ptr(), idx.data_ptr(), tval.data_ptr(), st))
    y = bn_apply(x, one, zero, ca, relu=False)          # (x * 1 + 0) * ca[n, c]
    return y, (dict(x=x, w0p=w0p, w2p=w2p, ca=ca, avg=avg, mx=mx, idx=idx, tval=tval, mean_nc=mean_nc) if save else None)


def ca_backward(ctx, dy, sink, pre=""):
    x, w0p, w2p = ctx["x"], ctx["w0p"], ctx["w2p"]
    n, h, w, c = x.shape
    cr = w0p.shape[3]
    hw, P = h * w, n * h * w
    dev, st = x.device, ops.stream()
    sm = Small(dev)
    one, zero = _consts(n, c, P, dev)
    ones_p = torch.ones(P, device=dev)
    zeros_p2 = torch.zeros((P, 2), device=dev)
    none_p = torch.full((P,), -1, device=dev, dtype=torch.int32)
    sdu, sdut, davg, dmx = sm.f(n * c), sm.f(n * c), sm.f(n * c), sm.f(n * c)
    check(lib.runet_rb_bwd2(dy.data_ptr(), ops.ld(dy), x.data_ptr(), ops.ld(x), ones_p.data_ptr(), zeros_p2.data_ptr(), none_p.data_ptr(), n, hw, c,
                            _ws(n, hw, c, dev).data_ptr(), sdu.data_ptr(), sdut.data_ptr(), st))
    dw0p = sink.buf(pre, [("fc.0.weight", (1, 1, c, cr))])
    dw2p = sink.buf(pre, [("fc.2.weight", (1, 1, cr, c))])
    sums = sm.f(2 * c)
    ws = scratch(lib.runet_ca_bwd_workspace_floats(n, c, cr), dev)
    check(lib.runet_ca_bwd(sdu.data_ptr(), sdut.data_ptr(), one.data_ptr(), zero.data_ptr(), ctx["ca"].data_ptr(), ctx["avg"].data_ptr(),
                           ctx["mx"].data_ptr(), w0p.data_ptr(), w2p.data_ptr(), ctx["mean_nc"].data_ptr(), ctx["tval"].data_ptr(), zero.data_ptr(),
                           one.data_ptr(), n, c, cr, ws.data_ptr(), davg.data_ptr(), dmx.data_ptr(), sums.data_ptr(), dw0p.data_ptr(), dw2p.data_ptr(), st))
    dx = ops.empty_nhwc(n, h, w, c, x)
    check(lib.runet_rb_bwd3(dy.data_ptr(), ops.ld(dy), x.data_ptr(), ops.ld(x), ones_p.data_ptr(), zeros_p2.data_ptr(), none_p.data_ptr(),
                            ctx["ca"].data_ptr(), davg.data_ptr(), dmx.data_ptr(), ctx["idx"].data_ptr(), zero.data_ptr(), one.data_ptr(), one.data_ptr(),
                            zero.data_ptr(), dx.data_ptr(), ops.ld(dx), P, hw, c, 0, st))
    return dx


def sa_forward(x, wsa, save=True):
    """y = x * sigmoid(conv7x7([mean_c x, max_c x])).  x NHWC.  -> (y, ctx)"""
    n, h, w, c = x.shape
    P = n * h * w
    dev, st = x.device, ops.stream()
    one, zero = _consts(n, c, P, dev)
    smap = torch.empty((P, 2), device=dev, dtype=torch.float32)
    amax = torch.empty(P, device=dev, dtype=torch.int32)
    check(lib.runet_sa_reduce(x.data_ptr(), ops.ld(x), one.data_ptr(), zero.data_ptr(), P, h * w, c, smap.data_ptr(), amax.data_ptr(), st))
    sa = torch.empty(P, device=dev, dtype=torch.float32)
    check(lib.runet_sa_conv7(smap.data_ptr(), wsa.data_ptr(), sa.data_ptr(), n, h, w, st))
    y = ops.empty_nhwc(n, h, w, c, x)
    check(lib.runet_mul_pixel(x.data_ptr(), ops.ld(x), sa.data_ptr(), y.data_ptr(), ops.ld(y), P, c, st))
    return y, (dict(x=x, wsa=wsa, smap=smap, amax=amax, sa=sa) if save else None)


def sa_backward(ctx, dy, sink, pre=""):
    x, wsa, smap, amax, sa = ctx["x"], ctx["wsa"], ctx["smap"], ctx["amax"], ctx["sa"]
    n, h, w, c = x.shape
    hw, P = h * w, n * h * w
    dev, st = x.device, ops.stream()
    sm = Small(dev)
    one, zero = _consts(n, c, P, dev)
    dv = ops.empty_nhwc(n, h, w, c, x)
    dq = torch.empty(P, device=dev, dtype=torch.float32)
    check(lib.runet_rb_bwd1(dy.data_ptr(), ops.ld(dy), None, 0, x.data_ptr(), ops.ld(x), one.data_ptr(), zero.data_ptr(), sa.data_ptr(),
                            dv.data_ptr(), ops.ld(dv), dq.data_ptr(), P, hw, c, st))
    dsm = torch.empty((P, 2), device=dev, dtype=torch.float32)
    dwsa = sink.buf(pre, [("conv1.weight", (7, 7, 2, 1))])
    ws = scratch(lib.runet_sa_conv7_bwd_workspace_floats(n, h, w), dev)
    check(lib.runet_sa_conv7_bwd(smap.data_ptr(), dq.data_ptr(), wsa.data_ptr(), dsm.data_ptr(), dwsa.data_ptr(), ws.data_ptr(), n, h, w, st))
    none_nc = torch.full((n * c,), -1, device=dev, dtype=torch.int32)
    dx = ops.empty_nhwc(n, h, w, c, x)
    check(lib.runet_rb_bwd3(dv.data_ptr(), ops.ld(dv), x.data_ptr(), ops.ld(x), sa.data_ptr(), dsm.data_ptr(), amax.data_ptr(), one.data_ptr(),
                            zero.data_ptr(), zero.data_ptr(), none_nc.data_ptr(), zero.data_ptr(), one.data_ptr(), one.data_ptr(), zero.data_ptr(),
                            dx.data_ptr(), ops.ld(dx), P, hw, c, 0, st))
    return dx


# =============================================================================== DilatedBlock
class DilParams:
    __slots__ = ("w", "b", "bn")

    def __init__(self, ws, bs, bn):
        self.w, self.b, self.bn = ws, bs, bn


DIL = (1, 1, 2, 4)


def dilated_forward(x, p: DilParams, training, save=True, stats_hook=None):
    n, h, w, _ = x.shape
    q = p.w[0].shape[3]
    sm = Small(x.device)
    cat = ops.empty_nhwc(n, h, w, 4 * q, x)
    for i in range(4):
        ops.conv_fwd(x, p.w[i], p.b[i], out=cat[..., i * q:(i + 1) * q], dil=DIL[i])
    s, hsh, mean, invstd, _ = bn_coeff(cat, p.bn, training, sm, stats_hook=stats_hook)
    out = bn_apply(cat, s, hsh, None, relu=True)
    if not save:
        return out, None
    return out, dict(x=x, cat=cat, out=out, p=p, s=s, h=hsh, mean=mean, invstd=invstd, training=training, sync=stats_hook if training else None)


def dilated_backward(ctx, dout, sink, pre="", need_dx=True):
    p: DilParams = ctx["p"]
    x, cat, out = ctx["x"], ctx["cat"], ctx["out"]
    q = p.w[0].shape[3]
    cin = x.shape[3]
    c = 4 * q
    # parameter order: conv1.weight, conv1.bias, ..., conv4.bias, bn.weight, bn.bias
    wb = [sink.buf(pre, [(f"conv{i + 1}.weight", (1 if i == 0 else 3, 1 if i == 0 else 3, cin, q)), (f"conv{i + 1}.bias", (q,))])
          for i in range(4)]
    sums = sink.buf(pre, [("bn.weight", (c,)), ("bn.bias", (c,))])
    dcat = bn_backward(dout, cat, ctx["mean"], ctx["invstd"], ctx["s"], sums, mask=None, sync=ctx["sync"], relu_shift=ctx["h"], training=ctx["training"])
    dx = None
    for i in range(4):
        sl = dcat[..., i * q:(i + 1) * q]
        k = 1 if i == 0 else 3
        nw = k * k * cin * q
        kz = {}
        if need_dx:
            dx = ops.conv_dgrad(sl, p.w[i], out=dx, dil=DIL[i], accumulate=i > 0, keep_z=kz)
        ops.conv_wgrad(x, sl, k, k, dil=DIL[i], out=wb[i][:nw], z=kz.get("Z"))
        chan_sum(sl, wb[i][nw:])
    return dx


# =============================================================================== up-conv + attention gate + concat
class UpGateParams:
    __slots__ = ("wup", "bup", "wg", "bg", "bng", "wx", "bx", "bnx", "wpsi", "bpsi", "bnp")

    def __init__(self, wup, bup, wg, bg, bng, wx, bx, bnx, wpsi, bpsi, bnp):
        (self.wup, self.bup, self.wg, self.bg, self.bng, self.wx, self.bx, self.bnx, self.wpsi, self.bpsi, self.bnp) = (
            wup, bup, wg, bg, bng, wx, bx, bnx, wpsi, bpsi, bnp)


def gate_x_branch(skip, p: UpGateParams, training, sm, stats_hook=None):
    """W_x(skip) + its BatchNorm statistics on the side stream: independent of the gate signal, so upgate_forward starts it in front of
    the transposed convolution.  -> (branch handle, x1, (scale, shift, mean, invstd))"""
    sm.f(4)
    n, h, w, _ = skip.shape
    x1 = ops.main_pool(ops.empty_nhwc(n, h, w, p.wx.shape[3], skip))      # allocated on the main stream (side_branch.join)
    br = ops.side_branch(stats_hook is None)
    with br:
        fx = {} if (training and stats_hook is None) else None
        ops.conv_fwd(skip, p.wx, p.bx, out=x1, stats=fx)
        # SyncBN: the statistics wait for gate_forward, where they share W_g's message
        cx = bn_coeff(x1, p.bnx, training, sm, fused=fx)[:4] if stats_hook is None else None
    return br, x1, cx


def gate_forward(up, skip, p: UpGateParams, training, att_out, sm, stats_hook=None, xb=None):
    """AttentionGate(g=up, x=skip) -> writes skip*psi into att_out; returns ctx pieces.  xb: gate_x_branch() started earlier."""
    n, h, w, c = skip.shape
    f = p.wg.shape[3]
    P = n * h * w
    st = ops.stream()
    if xb is None:
        xb = gate_x_branch(skip, p, training, sm, stats_hook)
    fg = {} if (training and stats_hook is None) else None
    g1 = ops.conv_fwd(up, p.wg, p.bg, stats=fg)
    br, x1, cx = xb
    if cx is None:
        br.join(x1)
        (sg, hg, mean_g, invstd_g), cx = bn_coeff_pair(g1, p.bng, x1, p.bnx, training, sm, stats_hook)
    else:
        sg, hg, mean_g, invstd_g, _ = bn_coeff(g1, p.bng, training, sm, fused=fg)
        br.join(x1)
    sx, hx, mean_x, invstd_x = cx
    s = torch.empty((n, h, w, 1), device=skip.device, dtype=torch.float32)
    check(lib.runet_ag_psi(g1.data_ptr(), ops.ld(g1), x1.data_ptr(), ops.ld(x1), sg.data_ptr(), hg.data_ptr(), sx.data_ptr(), hx.data_ptr(),
                           p.wpsi.data_ptr(), p.bpsi.data_ptr(), s.data_ptr(), P, f, st))
    sp, hp, mean_p, invstd_p, _ = bn_coeff(s, p.bnp, training, sm, stats_hook=stats_hook)
    check(lib.runet_ag_out(skip.data_ptr(), ops.ld(skip), s.data_ptr(), sp.data_ptr(), hp.data_ptr(), att_out.data_ptr(), ops.ld(att_out), P, c, st))
    return dict(training=training, sync=stats_hook if training else None, g1=g1, x1=x1, s=s, sg=sg, hg=hg, mean_g=mean_g, invstd_g=invstd_g, sx=sx, hx=hx, mean_x=mean_x, invstd_x=invstd_x,
                sp=sp, hp=hp, mean_p=mean_p, invstd_p=invstd_p)


def gate_backward(gc, up, skip, p: UpGateParams, datt, dup, sink, pre=""):
    """datt: grad of the gated skip (view); dup: grad buffer of `up`, accumulated into.  -> dskip"""
    n, h, w, c = skip.shape
    f = p.wg.shape[3]
    cg = up.shape[3]
    P = n * h * w
    st = ops.stream()
    dev = skip.device
    # parameter order: W_g.0.weight, W_g.0.bias, W_g.1.weight, W_g.1.bias, W_x.0.*, W_x.1.*, psi.0.weight, psi.0.bias, psi.1.*
    wg_b = sink.buf(pre, [("W_g.0.weight", (1, 1, cg, f)), ("W_g.0.bias", (f,))])
    sums_g = sink.buf(pre, [("W_g.1.weight", (f,)), ("W_g.1.bias", (f,))])
    wx_b = sink.buf(pre, [("W_x.0.weight", (1, 1, c, f)), ("W_x.0.bias", (f,))])
    sums_x = sink.buf(pre, [("W_x.1.weight", (f,)), ("W_x.1.bias", (f,))])
    dwpsi_db = sink.buf(pre, [("psi.0.weight", (1, 1, f, 1)), ("psi.0.bias", (1,))])
    sums_p = sink.buf(pre, [("psi.1.weight", (1,)), ("psi.1.bias", (1,))])
    dskip = ops.empty_nhwc(n, h, w, c, skip)
    dsbn = torch.empty((n, h, w, 1), device=dev, dtype=torch.float32)
    check(lib.runet_ag_bwd1(datt.data_ptr(), ops.ld(datt), skip.data_ptr(), ops.ld(skip), gc["s"].data_ptr(), gc["sp"].data_ptr(),
                            gc["hp"].data_ptr(), dskip.data_ptr(), ops.ld(dskip), dsbn.data_ptr(), P, c, st))
    sync, tr = gc["sync"], gc["training"]
    ds = bn_backward(dsbn, gc["s"], gc["mean_p"], gc["invstd_p"], gc["sp"], sums_p, out=dsbn, sync=sync, training=tr)
    dpre = ops.empty_nhwc(n, h, w, f, skip)
    g1, x1 = gc["g1"], gc["x1"]
    bn_g, bn_x = (gc["mean_g"], gc["invstd_g"], gc["sg"]), (gc["mean_x"], gc["invstd_x"], gc["sx"])
    synced = sync is not None and tr
    # where the two branches' BatchNorm-backward sums come from, and which sums enter dx (dx_sums): taken in the kernel that produces their
    # incoming gradient (runet_ag_bwd2_bn); SyncBN - two reductions, ready together, one all-reduce; or plain - each branch's own bn_backward
    if FUSED_GATE_BN_SUMS and not synced:
        ws = scratch(lib.runet_ag_bwd2_bn_workspace_floats(P, f), dev)
        check(lib.runet_ag_bwd2_bn(ds.data_ptr(), g1.data_ptr(), ops.ld(g1), x1.data_ptr(), ops.ld(x1), gc["sg"].data_ptr(), gc["hg"].data_ptr(),
                                   gc["sx"].data_ptr(), gc["hx"].data_ptr(), p.wpsi.data_ptr(), gc["mean_g"].data_ptr(), gc["invstd_g"].data_ptr(),
                                   gc["mean_x"].data_ptr(), gc["invstd_x"].data_ptr(), dpre.data_ptr(), ops.ld(dpre), ws.data_ptr(), ws.numel(),
                                   dwpsi_db.data_ptr(), sums_g.data_ptr(), sums_x.data_ptr(), P, f, st))
        use_g, use_x = dx_sums(sums_g, tr), dx_sums(sums_x, tr)
    else:
        ws = _ws(n, h * w, f, dev)
        check(lib.runet_ag_bwd2(ds.data_ptr(), g1.data_ptr(), ops.ld(g1), x1.data_ptr(), ops.ld(x1), gc["sg"].data_ptr(), gc["hg"].data_ptr(),
                                gc["sx"].data_ptr(), gc["hx"].data_ptr(), p.wpsi.data_ptr(), dpre.data_ptr(), ops.ld(dpre), ws.data_ptr(),
                                dwpsi_db.data_ptr(), P, f, st))
        use_g = use_x = None
        if synced:
            bn_bwd_reduce(dpre, g1, *bn_g, sums_g)
            bn_bwd_reduce(dpre, x1, *bn_x, sums_x)
            use_g, use_x = sync.reduce_sums_many([sums_g, sums_x], [P, P])

    def branch(t, bn, sums, use, src, wt, wb, dsrc, out=None):
        """One 1x1 branch: the gradient of its convolution's output t (dpre through its BatchNorm), its weight and bias gradients, and its
        data gradient accumulated into dsrc.  use: (sums, m_total) that enter dx, None: the branch reduces its own (plain mode)"""
        if use is None:
            d = bn_backward(dpre, t, *bn, sums, out=out, training=tr)
        else:
            d = bn_bwd_apply(dpre, t, *bn, *use, out=out)
        nw = src.shape[3] * f
        ops.conv_wgrad(src, d, 1, 1, out=wb[:nw])
        chan_sum(d, wb[nw:])
        ops.conv_dgrad(d, wt, out=dsrc, accumulate=True)

    branch(g1, bn_g, sums_g, use_g, up, p.wg, wg_b, dup)
    branch(x1, bn_x, sums_x, use_x, skip, p.wx, wx_b, dskip, out=dpre)
    return dskip


def upgate_forward(y, skip, p: UpGateParams, training, save=True, stats_hook=None):
    """cat([AttentionGate(up, skip), up]) with up = ConvTranspose2d(y), written into one buffer."""
    n, h, w, c = skip.shape
    sm = Small(skip.device)
    cat = ops.empty_nhwc(n, h, w, 2 * c, skip)
    up = cat[..., c:]
    xb = gate_x_branch(skip, p, training, sm, stats_hook)
    ops.convt_fwd(y, p.wup, p.bup, out=up)
    gc = gate_forward(up, skip, p, training, cat[..., :c], sm, stats_hook, xb=xb)
    if not save:
        return cat, None
    gc.update(y=y, skip=skip, cat=cat, p=p)
    return cat, gc


def upgate_backward(ctx, dcat, sink, pre_att, pre_up):
    """dcat [N,H,W,2C] is consumed (its right half accumulates the gate's gradient).  -> (dy, dskip)"""
    p: UpGateParams = ctx["p"]
    y, skip, cat = ctx["y"], ctx["skip"], ctx["cat"]
    c = skip.shape[3]
    cin = y.shape[3]
    up, dup, datt = cat[..., c:], dcat[..., c:], dcat[..., :c]
    dskip = gate_backward(ctx, up, skip, p, datt, dup, sink, pre=pre_att)
    up_b = sink.buf(pre_up, [("weight", (2, 2, cin, c)), ("bias", (c,))])
    ops.convt_wgrad(y, dup, out=up_b[:4 * cin * c])
    chan_sum(dup, up_b[4 * cin * c:])
    dy = ops.convt_dgrad(dup, p.wup)
    return dy, dskip


# =============================================================================== pool / stem / head
def maxpool_forward(x):
    n, h, w, c = x.shape
    y = ops.empty_nhwc(n, h // 2, w // 2, c, x)
    idx = torch.empty((n, h // 2, w // 2, c), device=x.device, dtype=torch.uint8)
    check(lib.runet_maxpool2_fwd(x.data_ptr(), ops.ld(x), y.data_ptr(), ops.ld(y), idx.data_ptr(), n, h, w, c, ops.stream()))
    return y, idx


def maxpool_backward(dy, idx, dx=None):
    """dx given: accumulate into it (skip-connection gradient already there)."""
    n, ho, wo, c = dy.shape
    acc = dx is not None
    if dx is None:
        dx = ops.empty_nhwc(n, 2 * ho, 2 * wo, c, dy)
    check(lib.runet_maxpool2_bwd(dy.data_ptr(), ops.ld(dy), idx.data_ptr(), dx.data_ptr(), ops.ld(dx), n, 2 * ho, 2 * wo, c, int(acc), ops.stream()))
    return dx


def bn_relu_maxpool_forward(t, scale, shift):
    """maxpool2(relu(t * scale + shift)) in one pass: -> (pooled, idx); the full-resolution activation is not written (SegNet's encoder ends)."""
    n, h, w, c = t.shape
    y = ops.empty_nhwc(n, h // 2, w // 2, c, t)
    idx = torch.empty((n, h // 2, w // 2, c), device=t.device, dtype=torch.uint8)
    check(lib.runet_bn_relu_maxpool2_fwd(t.data_ptr(), ops.ld(t), scale.data_ptr(), shift.data_ptr(), y.data_ptr(), ops.ld(y), idx.data_ptr(), n, h, w,
                                         c, ops.stream()))
    return y, idx


def bn_backward_pooled(dpool, idx, x, mean, invstd, scale, sums, relu_shift, training=True):
    """bn_backward(maxpool_backward(dpool, idx), x, ..., relu_shift=...) without the full-resolution gradient: the two pooled-gradient kernels
    scatter it in registers.  -> dx (full resolution)"""
    n, h, w, c = x.shape
    st = ops.stream()
    check(lib.runet_bn_bwd_reduce_pooled(dpool.data_ptr(), ops.ld(dpool), idx.data_ptr(), x.data_ptr(), ops.ld(x), n, h, w, c, mean.data_ptr(),
                                         invstd.data_ptr(), _ws(n, h * w, c, x.device).data_ptr(), sums.data_ptr(), scale.data_ptr(),
                                         relu_shift.data_ptr(), st))
    use = dx_sums(sums, training)[0]
    dx = ops.empty_nhwc(n, h, w, c, x)
    check(lib.runet_bn_bwd_apply_pooled(dpool.data_ptr(), ops.ld(dpool), idx.data_ptr(), x.data_ptr(), ops.ld(x), dx.data_ptr(), ops.ld(dx), n, h, w, c,
                                        mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(), use.data_ptr(), 0, relu_shift.data_ptr(), st))
    return dx


# ---- LeakyReLU forms (YOLOSeg, Main_Final.py:436-510: every BatchNorm2d is followed by nn.LeakyReLU(0.1))
# RUNET_NO_FUSED_LEAKY_POOL=1: a stage end runs runet_bn_apply_leaky + runet_maxpool2_fwd (and the full-resolution backward) instead of the
# fused pool kernels - the A/B partner; both give the same bits.
FUSED_LEAKY_POOL = os.environ.get("RUNET_NO_FUSED_LEAKY_POOL", "0") != "1"


def bn_apply_leaky(x, scale, shift, slope, out=None):
    """leaky_relu(x * scale + shift, slope) in one pass."""
    n, h, w, c = x.shape
    if out is None:
        out = ops.empty_nhwc(n, h, w, c, x)
    check(lib.runet_bn_apply_leaky(x.data_ptr(), ops.ld(x), out.data_ptr(), ops.ld(out), n * h * w, h * w, c, scale.data_ptr(), shift.data_ptr(),
                                   float(slope), ops.stream()))
    return out


def bn_backward_leaky(dy, x, mean, invstd, scale, sums, shift, slope, training=True, out=None):
    """bn_backward(relu_shift=shift) with the LeakyReLU factor (dy * slope where x * scale + shift <= 0).  sums: [2c] (dgamma | dbeta). -> dx"""
    n, h, w, c = x.shape
    hw = h * w
    st = ops.stream()
    check(lib.runet_bn_bwd_reduce_leaky(dy.data_ptr(), ops.ld(dy), x.data_ptr(), ops.ld(x), n, hw, c, mean.data_ptr(), invstd.data_ptr(),
                                        _ws(n, hw, c, x.device).data_ptr(), sums.data_ptr(), scale.data_ptr(), shift.data_ptr(), float(slope), st))
    use = dx_sums(sums, training)[0]
    if out is None:
        out = ops.empty_nhwc(n, h, w, c, x)
    check(lib.runet_bn_bwd_apply_leaky(dy.data_ptr(), ops.ld(dy), x.data_ptr(), ops.ld(x), out.data_ptr(), ops.ld(out), n * hw, hw, c,
                                       mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(), use.data_ptr(), 0, shift.data_ptr(), float(slope), st))
    return out


def bn_leaky_maxpool_forward(t, scale, shift, slope):
    """maxpool2(leaky_relu(t * scale + shift, slope)) -> (pooled, idx).  Fused: one pass, the full-resolution activation is not written."""
    n, h, w, c = t.shape
    if not FUSED_LEAKY_POOL:
        return maxpool_forward(bn_apply_leaky(t, scale, shift, slope))
    y = ops.empty_nhwc(n, h // 2, w // 2, c, t)
    idx = torch.empty((n, h // 2, w // 2, c), device=t.device, dtype=torch.uint8)
    check(lib.runet_bn_leaky_maxpool2_fwd(t.data_ptr(), ops.ld(t), scale.data_ptr(), shift.data_ptr(), float(slope), y.data_ptr(), ops.ld(y),
                                          idx.data_ptr(), n, h, w, c, ops.stream()))
    return y, idx


def bn_backward_pooled_leaky(dpool, idx, x, mean, invstd, scale, sums, shift, slope, training=True):
    """bn_backward_leaky(maxpool_backward(dpool, idx), x, ...) without the full-resolution gradient (fused), or with it
    (RUNET_NO_FUSED_LEAKY_POOL=1).  -> dx (full resolution)"""
    if not FUSED_LEAKY_POOL:
        return bn_backward_leaky(maxpool_backward(dpool, idx), x, mean, invstd, scale, sums, shift, slope, training=training)
    n, h, w, c = x.shape
    st = ops.stream()
    check(lib.runet_bn_bwd_reduce_pooled_leaky(dpool.data_ptr(), ops.ld(dpool), idx.data_ptr(), x.data_ptr(), ops.ld(x), n, h, w, c, mean.data_ptr(),
                                               invstd.data_ptr(), _ws(n, h * w, c, x.device).data_ptr(), sums.data_ptr(), scale.data_ptr(),
                                               shift.data_ptr(), float(slope), st))
    use = dx_sums(sums, training)[0]
    dx = ops.empty_nhwc(n, h, w, c, x)
    check(lib.runet_bn_bwd_apply_pooled_leaky(dpool.data_ptr(), ops.ld(dpool), idx.data_ptr(), x.data_ptr(), ops.ld(x), dx.data_ptr(), ops.ld(dx), n,
                                              h, w, c, mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(), use.data_ptr(), 0, shift.data_ptr(),
                                              float(slope), st))
    return dx


def maxunpool_forward(x, idx):
    """nn.MaxUnpool2d(2, 2) by a 2x2 pool's winner bytes: zeros, each value at its index (= runet_maxpool2_bwd without accumulation)."""
    return maxpool_backward(x, idx)


def maxunpool_backward(du, idx):
    """Gradient of maxunpool_forward: the gather du[2ho + k/2, 2wo + k%2] at each pooled position."""
    n, h, w, c = du.shape
    dp = ops.empty_nhwc(n, h // 2, w // 2, c, du)
    check(lib.runet_maxunpool2_bwd(du.data_ptr(), ops.ld(du), idx.data_ptr(), dp.data_ptr(), ops.ld(dp), n, h, w, c, ops.stream()))
    return dp


def to_nhwc_pad(x_nchw, c_pad):
    n, c, h, w = x_nchw.shape
    y = torch.empty((n, h, w, c_pad), device=x_nchw.device, dtype=torch.float32)
    sn, sc, sh, sw = x_nchw.stride()
    check(lib.runet_to_nhwc_pad(x_nchw.data_ptr(), sn, sc, sh, sw, y.data_ptr(), n, c, h, w, c_pad, ops.stream()))
    return y


def outc_forward(x, w, b, want_logit=False):
    n, h, wd, c = x.shape
    prob = torch.empty((n, 1, h, wd), device=x.device, dtype=torch.float32)
    logit = torch.empty((n, 1, h, wd), device=x.device, dtype=torch.float32) if want_logit else None
    check(lib.runet_outc_fwd(x.data_ptr(), ops.ld(x), w.data_ptr(), b.data_ptr(), logit.data_ptr() if want_logit else None, prob.data_ptr(),
                             n * h * wd, c, ops.stream()))
    return prob, logit


def outc_backward(dprob, prob, x, w, sink, pre=""):
    n, h, wd, c = x.shape
    dx = ops.empty_nhwc(n, h, wd, c, x)
    dw_db = sink.buf(pre, [("weight", (1, 1, c, 1)), ("bias", (1,))])
    ws = _ws(n, h * wd, c, x.device)
    check(lib.runet_outc_bwd(dprob.data_ptr(), prob.data_ptr(), x.data_ptr(), ops.ld(x), w.data_ptr(), dx.data_ptr(), ops.ld(dx), ws.data_ptr(),
                             dw_db.data_ptr(), n * h * wd, c, ops.stream()))
    return dx


def outc_backward_dl(dprob, prob, x, sink, pre=""):
    """outc_backward without the data gradient: the parameter gradients, and -> dl [P], the logit's gradient, for rb_backward(head_grad=(dl, w))"""
    n, h, wd, c = x.shape
    dl = torch.empty(n * h * wd, device=x.device, dtype=torch.float32)
    dw_db = sink.buf(pre, [("weight", (1, 1, c, 1)), ("bias", (1,))])
    ws = _ws(n, h * wd, c, x.device)
    check(lib.runet_outc_bwd_dl(dprob.data_ptr(), prob.data_ptr(), x.data_ptr(), ops.ld(x), dl.data_ptr(), ws.data_ptr(), dw_db.data_ptr(), n * h * wd, c,
                                ops.stream()))
    return dl


# =============================================================================== HRNet-Water head and fusion branches (csrc/hrnet.hip)
# The head's 1x1 convolution and the fusion branches' BatchNorm affine commute with the bilinear interpolation (its weights sum to 1), so they
# run on the small side of it.  RUNET_NO_FUSED_HR_HEAD=1 / RUNET_NO_FUSED_BN_UPSAMPLE=1: the reference's order on the shared kernels
# (runet_bn_apply, runet_bilinear_nhwc_*, runet_outc_*) - the A/B partners the fusions are timed against.
FUSED_HR_HEAD = os.environ.get("RUNET_NO_FUSED_HR_HEAD", "0") != "1"
FUSED_BN_UPSAMPLE = os.environ.get("RUNET_NO_FUSED_BN_UPSAMPLE", "0") != "1"


def _bilinear_nhwc(x, out):
    n, h, w, c = x.shape
    check(lib.runet_bilinear_nhwc_fwd(x.data_ptr(), ops.ld(x), out.data_ptr(), ops.ld(out), n, h, w, out.shape[1], out.shape[2], c, ops.stream()))
    return out


def _bilinear_nhwc_backward(dy, h, w):
    n, ho, wo, c = dy.shape
    dx = ops.empty_nhwc(n, h, w, c, dy)
    check(lib.runet_bilinear_nhwc_bwd(dy.data_ptr(), ops.ld(dy), dx.data_ptr(), ops.ld(dx), n, h, w, ho, wo, c, ops.stream()))
    return dx


def hr_head_forward(t, scale, shift, w, b, fused=None):
    """sigmoid(conv1x1(upsample2(relu(t * scale + shift)))) -> (prob [n, 1, 2h, 2w], saved).  t [n, h, w, c]: the head's raw 3x3 convolution
    output, w [c] / b [1]: the 1x1 convolution.  Fused: the 1x1 at t's resolution, then the one-channel plane upsampled (saved = None: the
    backward needs only t and prob).  Unfused: saved = (activation [n, h, w, c], its upsampling [n, 2h, 2w, c])."""
    n, h, wd, c = t.shape
    st = ops.stream()
    if FUSED_HR_HEAD if fused is None else fused:
        z = torch.empty((n, h, wd), device=t.device, dtype=torch.float32)
        prob = torch.empty((n, 1, 2 * h, 2 * wd), device=t.device, dtype=torch.float32)
        check(lib.runet_hr_head_fwd(t.data_ptr(), ops.ld(t), scale.data_ptr(), shift.data_ptr(), w.data_ptr(), b.data_ptr(), z.data_ptr(), n, h, wd, c, st))
        check(lib.runet_up2_sigmoid_fwd(z.data_ptr(), prob.data_ptr(), n, h, wd, st))
        return prob, None
    a = bn_apply(t, scale, shift, None, relu=True)
    up = _bilinear_nhwc(a, ops.empty_nhwc(n, 2 * h, 2 * wd, c, t))
    prob, _ = outc_forward(up, w, b)
    return prob, (a, up)


def hr_head_backward(dprob, prob, t, scale, shift, w, mean, invstd, saved=None, training=True):
    """-> (dt [n, h, w, c], out [3c + 1] = (dgamma | dbeta | dw | db)); saved: what hr_head_forward returned (None = the fused path)"""
    n, h, wd, c = t.shape
    dev = t.device
    st = ops.stream()
    out = torch.empty(3 * c + 1, device=dev, dtype=torch.float32)
    if saved is None:
        dz = torch.empty((n, h, wd), device=dev, dtype=torch.float32)
        check(lib.runet_up2_sigmoid_bwd(dprob.data_ptr(), prob.data_ptr(), dz.data_ptr(), n, h, wd, st))
        ws = scratch(lib.runet_hr_head_bwd_workspace_floats(n, h, wd, c), dev)
        check(lib.runet_hr_head_bwd_reduce(dz.data_ptr(), t.data_ptr(), ops.ld(t), scale.data_ptr(), shift.data_ptr(), w.data_ptr(), mean.data_ptr(),
                                           invstd.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(), n, h, wd, c, st))
        use = dx_sums(out, training)[0]
        dt = ops.empty_nhwc(n, h, wd, c, t)
        check(lib.runet_hr_head_bwd_apply(dz.data_ptr(), t.data_ptr(), ops.ld(t), w.data_ptr(), dt.data_ptr(), ops.ld(dt), n, h, wd, c, mean.data_ptr(),
                                          invstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), use.data_ptr(), 0, st))
        return dt, out
    a, up = saved
    dup = ops.empty_nhwc(n, 2 * h, 2 * wd, c, t)
    check(lib.runet_outc_bwd(dprob.data_ptr(), prob.data_ptr(), up.data_ptr(), ops.ld(up), w.data_ptr(), dup.data_ptr(), ops.ld(dup),
                             _ws(n, 4 * h * wd, c, dev).data_ptr(), out[2 * c:].data_ptr(), n * 4 * h * wd, c, st))
    da = _bilinear_nhwc_backward(dup, h, wd)
    dt = bn_backward(da, t, mean, invstd, scale, out[:2 * c], relu_shift=shift, out=da, training=training)
    return dt, out


def bn_bilinear_forward(x, scale, shift, out, s, fused=None):
    """out [n, s h, s w, 0:c] (an NHWC view, normally a channel slice of the concat buffer) := upsample_s(x * scale + shift), s = 2 or 4"""
    n, h, w, c = x.shape
    if tuple(out.shape) != (n, s * h, s * w, c):
        raise ValueError(f"bn_bilinear_forward: out {tuple(out.shape)} is not {s} x {tuple(x.shape)}")
    if FUSED_BN_UPSAMPLE if fused is None else fused:
        check(lib.runet_bn_bilinear_nhwc_fwd(x.data_ptr(), ops.ld(x), out.data_ptr(), ops.ld(out), scale.data_ptr(), shift.data_ptr(), n, h, w, s, c,
                                             ops.stream()))
        return out
    return _bilinear_nhwc(bn_apply(x, scale, shift), out)


def bn_bilinear_backward(dy, x, mean, invstd, scale, sums, s, training=True, fused=None):
    """dy [n, s h, s w, 0:c]: the gradient of bn_bilinear_forward's out; sums [2c] receives (dgamma | dbeta).  -> dx [n, h, w, c]"""
    n, h, w, c = x.shape
    if not (FUSED_BN_UPSAMPLE if fused is None else fused):
        g = _bilinear_nhwc_backward(dy, h, w)
        return bn_backward(g, x, mean, invstd, scale, sums, out=g, training=training)
    g = ops.empty_nhwc(n, h, w, c, x)
    ws = scratch(lib.runet_bilinear_nhwc_bwd_sums_workspace_floats(n, h, w, c), x.device)
    check(lib.runet_bilinear_nhwc_bwd_sums(dy.data_ptr(), ops.ld(dy), x.data_ptr(), ops.ld(x), mean.data_ptr(), invstd.data_ptr(), g.data_ptr(), ops.ld(g),
                                           ws.data_ptr(), ws.numel(), sums.data_ptr(), n, h, w, s, c, ops.stream()))
    use = dx_sums(sums, training)[0]
    return bn_bwd_apply(g, x, mean, invstd, scale, use, 0, out=g)



# =============================================================================== WaterNet front end (csrc/water_index.hip)
# WaterIndexModule + torch.cat (Extended_Baseline_Comparison.py:378-393, :458): Conv2d(3, 16, 1) -> BatchNorm2d -> ReLU -> Conv2d(16, 4, 1) ->
# Sigmoid, cat([x, idx]) as the 8-channel NHWC buffer [R, G, B, s0..s3, 0] that enc1's first convolution reads with cin_w = 7.  Fused: every
# 16-channel tensor is recomputed per pixel in registers (four launches + the shared finalize).  RUNET_NO_FUSED_WATER_INDEX=1: the reference's
# order on the shared kernels (runet_to_nhwc_pad, the implicit-GEMM 1x1 convolutions, bn_coeff / bn_apply / bn_backward, conv_wgrad, chan_sum,
# with runet_sigmoid_nhwc_* and runet_copy_nhwc for the sigmoid and the cat) - the A/B partner the fusion is timed against.
FUSED_WATER_INDEX = os.environ.get("RUNET_NO_FUSED_WATER_INDEX", "0") != "1"
WI_MID, WI_OUT = 16, 4


class WaterIndexParams:
    """w1 [1, 1, 3, 16] / w2 [1, 1, 16, 4]: the two 1x1 convolutions' weights in their physical (HWIO) layout; bn: BNState"""
    __slots__ = ("w1", "b1", "bn", "w2", "b2")

    def __init__(self, w1, b1, bn, w2, b2):
        self.w1, self.b1, self.bn, self.w2, self.b2 = w1, b1, bn, w2, b2


def _wi_src(x):
    n, c, h, w = x.shape
    if c != 3 or x.dtype != torch.float32:
        raise ValueError("water_index: expected a float32 image [N, 3, H, W]")
    return (x.data_ptr(),) + tuple(x.stride()) + (n, h, w)


def _wi_coef(p: WaterIndexParams):
    return (p.w1.data_ptr(), p.b1.data_ptr()), (p.w2.data_ptr(), p.b2.data_ptr())


def water_index_forward(x_nchw, p: WaterIndexParams, training, sm: Small, fused=None):
    """-> (buf [n, h, w, 8] = [R, G, B, s0..s3, 0], ctx for water_index_backward)"""
    n, _, h, w = x_nchw.shape
    dev, st = x_nchw.device, ops.stream()
    src = _wi_src(x_nchw)
    bn = p.bn
    buf = torch.empty((n, h, w, 8), device=dev, dtype=torch.float32)
    if FUSED_WATER_INDEX if fused is None else fused:
        c1, c2 = _wi_coef(p)
        scale, shift, mean, invstd = sm.f(WI_MID), sm.f(WI_MID), sm.f(WI_MID), sm.f(WI_MID)
        if training:
            nparts = lib.runet_water_index_parts(n, h, w)
            part = scratch(nparts * WI_MID * 3, dev)
            check(lib.runet_water_index_stats(*src, *c1, part.data_ptr(), part.numel(), st))
            check(lib.runet_bn_stats_finalize(part.data_ptr(), nparts, WI_MID, bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(),
                                              bn.running_var.data_ptr(), bn.nbt.data_ptr(), BN_MOMENTUM, BN_EPS, scale.data_ptr(), shift.data_ptr(),
                                              mean.data_ptr(), invstd.data_ptr(), st))
        else:
            check(lib.runet_bn_finalize(None, None, n, WI_MID, h * w, bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(),
                                        bn.running_var.data_ptr(), None, BN_MOMENTUM, BN_EPS, 0, scale.data_ptr(), shift.data_ptr(),
                                        mean.data_ptr(), invstd.data_ptr(), st))
        check(lib.runet_water_index_fwd(*src, *c1, scale.data_ptr(), shift.data_ptr(), *c2, buf.data_ptr(), 8, st))
        return buf, dict(x=x_nchw, p=p, scale=scale, shift=shift, mean=mean, invstd=invstd, training=training, fused=True)
    P = n * h * w
    x4 = to_nhwc_pad(x_nchw, 4)
    z = ops.conv_fwd(x4, p.w1, p.b1)
    scale, shift, mean, invstd, _ = bn_coeff(z, bn, training, sm)
    a = bn_apply(z, scale, shift, None, relu=True)
    u = ops.conv_fwd(a, p.w2, p.b2)
    check(lib.runet_copy_nhwc(x4.data_ptr(), 4, buf.data_ptr(), 8, P, 3, st))
    check(lib.runet_sigmoid_nhwc_fwd(u.data_ptr(), WI_OUT, buf[..., 3:].data_ptr(), 8, P, WI_OUT, st))
    check(lib.runet_copy_nhwc(x4[..., 3:].data_ptr(), 4, buf[..., 7:].data_ptr(), 8, P, 1, st))      # the padding channel: zero
    return buf, dict(x4=x4, z=z, a=a, buf=buf, p=p, scale=scale, shift=shift, mean=mean, invstd=invstd, training=training, fused=False)


def water_index_backward(ctx, g):
    """g [n, h, w, 4]: an NHWC view (any pixel stride, any first channel) of the gradient of channels 3..6 of the forward's buffer.
    -> out_red [100] = (dgamma [16] | dbeta [16] | dW2 [16][4] | db2 [4]), out_app [64] = (dW1 [3][16] | db1 [16]), physical layouts"""
    p: WaterIndexParams = ctx["p"]
    n, h, w, c = g.shape
    if c != WI_OUT:
        raise ValueError("water_index_backward: g must have 4 channels")
    dev, st = g.device, ops.stream()
    ldg = ops.ld(g)
    training = ctx["training"]
    out_red = torch.empty(2 * WI_MID + WI_MID * WI_OUT + WI_OUT, device=dev, dtype=torch.float32)
    out_app = torch.empty(4 * WI_MID, device=dev, dtype=torch.float32)
    scale, shift, mean, invstd = ctx["scale"], ctx["shift"], ctx["mean"], ctx["invstd"]
    if ctx["fused"]:
        src = _wi_src(ctx["x"])
        c1, c2 = _wi_coef(p)
        ws = scratch(lib.runet_water_index_workspace_floats(n, h, w), dev)
        check(lib.runet_water_index_bwd_reduce(*src, g.data_ptr(), ldg, *c1, scale.data_ptr(), shift.data_ptr(), *c2, mean.data_ptr(), invstd.data_ptr(),
                                               ws.data_ptr(), ws.numel(), out_red.data_ptr(), st))
        use = dx_sums(out_red, training)[0]
        check(lib.runet_water_index_bwd_apply(*src, g.data_ptr(), ldg, *c1, scale.data_ptr(), shift.data_ptr(), *c2, mean.data_ptr(), invstd.data_ptr(),
                                              use.data_ptr(), 0, ws.data_ptr(), ws.numel(), out_app.data_ptr(), st))
        return out_red, out_app
    P = n * h * w
    buf, a, z, x4 = ctx["buf"], ctx["a"], ctx["z"], ctx["x4"]
    du = torch.empty((n, h, w, WI_OUT), device=dev, dtype=torch.float32)
    check(lib.runet_sigmoid_nhwc_bwd(g.data_ptr(), ldg, buf[..., 3:].data_ptr(), 8, du.data_ptr(), WI_OUT, P, WI_OUT, st))
    k = 2 * WI_MID
    ops.conv_wgrad(a, du, 1, 1, out=out_red[k:k + WI_MID * WI_OUT].view(1, 1, WI_MID, WI_OUT))
    chan_sum(du, out_red[k + WI_MID * WI_OUT:])
    da = ops.conv_dgrad(du, p.w2)
    dz = bn_backward(da, z, mean, invstd, scale, out_red[:k], relu_shift=shift, out=da, training=training)
    ops.conv_wgrad(x4, dz, 1, 1, cin_w=3, out=out_app[:3 * WI_MID].view(1, 1, 3, WI_MID))
    chan_sum(dz, out_app[3 * WI_MID:])
    return out_red, out_app


# =============================================================================== MSWNet's MultiScaleBlock (csrc/multiscale.hip)
# MultiScaleBlock (Extended_Baseline_Comparison.py:479-494): cat(1x1, 3x3, 5x5, maxpool3 -> 1x1), each Conv2d -> BatchNorm2d -> ReLU at a quarter of
# the output channels.  ms_block_*: the four convolutions write channel slices of one buffer t, the four BatchNorms' vectors sit back to back in
# one vector each, so BatchNorm + ReLU and its backward run once over all channels.  ms_stem_*: the first level, MultiScaleBlock(3, 64), fused
# over the NCHW image (t is recomputed per pixel and never written).  RUNET_NO_FUSED_MS_STEM=1: the first level through ms_block_* on a
# 4-channel NHWC copy of the image - the A/B partner the fusion is timed against (tools/mswnet_step.py; the A/B run that decides this default
# is not measured yet: DESIGN.md section 3.12).
FUSED_MS_STEM = os.environ.get("RUNET_NO_FUSED_MS_STEM", "0") != "1"
MS_STEM_C, MS_STEM_Q = 64, 16


class MSBlockParams:
    """w, b: the four convolutions' weights (HWIO: [1,1,ci,q], [3,3,ci,q], [5,5,ci,q], [1,1,ci,q]) and biases in branch order; bn: four BNState"""
    __slots__ = ("w", "b", "bn")

    def __init__(self, w, b, bn):
        self.w, self.b, self.bn = w, b, bn


def maxpool3s1_forward(x, want_idx=True, out=None):
    """MaxPool2d(3, stride 1, padding 1) of an NHWC view -> (y, winner bytes [n, h, w, c] or None)"""
    n, h, w, c = x.shape
    y = ops.empty_nhwc(n, h, w, c, x) if out is None else out
    idx = torch.empty((n, h, w, c), device=x.device, dtype=torch.uint8) if want_idx else None
    check(lib.runet_maxpool3s1_fwd(x.data_ptr(), ops.ld(x), y.data_ptr(), ops.ld(y), idx.data_ptr() if want_idx else None, n, h, w, c, ops.stream()))
    return y, idx


def maxpool3s1_backward(dy, idx, dx=None):
    """dx given: accumulate into it (the block's other three data gradients are already there)."""
    n, h, w, c = dy.shape
    acc = dx is not None
    if dx is None:
        dx = ops.empty_nhwc(n, h, w, c, dy)
    check(lib.runet_maxpool3s1_bwd(dy.data_ptr(), ops.ld(dy), idx.data_ptr(), dx.data_ptr(), ops.ld(dx), n, h, w, c, int(acc), ops.stream()))
    return dx


def _bn_coeff_into(x, bn: BNState, training, fused, scale, shift, mean, invstd):
    """bn_coeff's two-launch routes for ONE BatchNorm whose input is a channel slice x, the coefficients written into the given slices of the
    block's concatenated vectors"""
    n, h, w, c = x.shape
    st = ops.stream()
    out = (scale.data_ptr(), shift.data_ptr(), mean.data_ptr(), invstd.data_ptr(), st)
    if not training:
        check(lib.runet_bn_finalize(None, None, n, c, h * w, bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(),
                                    bn.running_var.data_ptr(), None, BN_MOMENTUM, BN_EPS, 0, *out))
    elif FUSED_BN_STATS and fused and "part" in fused:
        check(lib.runet_bn_stats_finalize(fused["part"].data_ptr(), fused["nparts"], c, bn.weight.data_ptr(), bn.bias.data_ptr(),
                                          bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.nbt.data_ptr(), BN_MOMENTUM, BN_EPS, *out))
    else:
        check(lib.runet_bn_stats(x.data_ptr(), ops.ld(x), n, h * w, c, _ws(n, h * w, c, x.device).data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(),
                                 bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.nbt.data_ptr(), BN_MOMENTUM, BN_EPS, *out))


def ms_block_forward(x, p: MSBlockParams, training, sm: Small, out=None, save=True):
    """x [n, h, w, cx] NHWC (cx >= the weights' input channels: the RGB image zero-padded to 4) -> (relu(bn(cat)) written to `out`, ctx or None)"""
    n, h, w, _ = x.shape
    q = p.w[0].shape[3]
    c = 4 * q
    t = ops.empty_nhwc(n, h, w, c, x)
    xp, idx = maxpool3s1_forward(x, want_idx=save)
    vecs = [sm.f(c) for _ in range(4)]              # scale, shift, mean, invstd of the four BatchNorms back to back
    for b in range(4):
        sl = t[..., b * q:(b + 1) * q]
        fs = {} if training else None
        if b == 2:
            ops.conv_general_fwd(x, p.w[b], p.b[b], 1, 2, out=sl)
        else:
            ops.conv_fwd(xp if b == 3 else x, p.w[b], p.b[b], out=sl, stats=fs)
        _bn_coeff_into(sl, p.bn[b], training, fs, *(v[b * q:(b + 1) * q] for v in vecs))
    scale, shift, mean, invstd = vecs
    e = bn_apply(t, scale, shift, None, relu=True, out=out)
    if not save:
        return e, None
    return e, dict(x=x, xp=xp, idx=idx, t=t, p=p, scale=scale, shift=shift, mean=mean, invstd=invstd, training=training, fused=False)


def _ms_param_grads(x, xp, dt, p: MSBlockParams, G, pre):
    """the four convolutions' weight and bias gradients from dt's channel slices -> G[pre + "branch{b}.{i}.weight" / ".bias"]"""
    q = p.w[0].shape[3]
    cin_w = p.w[0].shape[2]
    for b in range(4):
        sl = dt[..., b * q:(b + 1) * q]
        name = f"{pre}branch{b + 1}.{1 if b == 3 else 0}"
        if b == 2:
            G[name + ".weight"] = ops.conv_general_wgrad(x, sl, 5, 5, 1, 2, cin_w=cin_w)
        else:
            k = 3 if b == 1 else 1
            G[name + ".weight"] = ops.conv_wgrad(xp if b == 3 else x, sl, k, k, cin_w=cin_w)
        G[name + ".bias"] = chan_sum(sl, torch.empty(q, device=dt.device, dtype=torch.float32))


def _ms_bn_grads(sums, q, G, pre):
    c = 4 * q
    for b in range(4):
        name = f"{pre}branch{b + 1}.{2 if b == 3 else 1}"
        G[name + ".weight"], G[name + ".bias"] = sums[b * q:(b + 1) * q], sums[c + b * q:c + (b + 1) * q]


def ms_block_backward(ctx, de, G, pre="", need_dx=True, keep=None):
    """de: the gradient of ms_block_forward's output (an NHWC view).  Parameter gradients into G (physical layouts).  -> dx or None; the input
    gradient is accumulated in a fixed order: 1x1, 3x3, 5x5, then the gather through the 3x3 pool of branch4's 1x1 data gradient.
    keep: a dict that receives "dt", the gradient of the four convolutions' outputs."""
    p: MSBlockParams = ctx["p"]
    x, xp, t = ctx["x"], ctx["xp"], ctx["t"]
    n, h, w, c = t.shape
    q = c // 4
    sums = torch.empty(2 * c, device=t.device, dtype=torch.float32)
    dt = bn_backward(de, t, ctx["mean"], ctx["invstd"], ctx["scale"], sums, relu_shift=ctx["shift"], training=ctx["training"])
    _ms_bn_grads(sums, q, G, pre)
    if keep is not None:
        keep["dt"] = dt
    dx = None
    if need_dx:
        dx = ops.conv_dgrad(dt[..., :q], p.w[0])
        ops.conv_dgrad(dt[..., q:2 * q], p.w[1], out=dx, accumulate=True)
        ops.conv_general_dgrad(dt[..., 2 * q:3 * q], p.w[2], h, w, 1, 2, out=dx, accumulate=True)
        d4 = ops.conv_dgrad(dt[..., 3 * q:], p.w[3])
        maxpool3s1_backward(d4, ctx["idx"], dx=dx)
    _ms_param_grads(x, xp, dt, p, G, pre)
    return dx


def _ms_src(x):
    n, c, h, w = x.shape
    if c != 3 or x.dtype != torch.float32:
        raise ValueError("ms_stem: expected a float32 image [N, 3, H, W]")
    return (x.data_ptr(),) + tuple(x.stride()) + (n, h, w)


def _ms_wts(p: MSBlockParams):
    if tuple(p.w[2].shape) != (5, 5, 3, MS_STEM_Q):
        raise ValueError("ms_stem: the fused stem is MultiScaleBlock(3, 64)")
    return tuple(t.data_ptr() for t in p.w) + tuple(t.data_ptr() for t in p.b)


def ms_stem_forward(x_nchw, p: MSBlockParams, training, sm: Small, out=None, save=True, fused=None):
    """MultiScaleBlock(3, 64) on the NCHW image -> (e [n, h, w, 64] written to `out`, ctx for ms_stem_backward or None)"""
    n, _, h, w = x_nchw.shape
    dev, st = x_nchw.device, ops.stream()
    if not (FUSED_MS_STEM if fused is None else fused):
        return ms_block_forward(to_nhwc_pad(x_nchw, 4), p, training, sm, out=out, save=save)
    src, wts = _ms_src(x_nchw), _ms_wts(p)
    c, q = MS_STEM_C, MS_STEM_Q
    if out is None:
        out = torch.empty((n, h, w, c), device=dev, dtype=torch.float32)
    scale, shift, mean, invstd = sm.f(c), sm.f(c), sm.f(c), sm.f(c)
    if training:
        nparts = lib.runet_ms_stem_parts(n, h, w)
        part = scratch(4 * nparts * q * 3, dev)
        check(lib.runet_ms_stem_stats(*src, *wts, part.data_ptr(), part.numel(), st))
    for b in range(4):
        bn, sl = p.bn[b], slice(b * q, (b + 1) * q)
        o = (scale[sl].data_ptr(), shift[sl].data_ptr(), mean[sl].data_ptr(), invstd[sl].data_ptr(), st)
        if training:
            check(lib.runet_bn_stats_finalize(part[b * nparts * q * 3:].data_ptr(), nparts, q, bn.weight.data_ptr(), bn.bias.data_ptr(),
                                              bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.nbt.data_ptr(), BN_MOMENTUM, BN_EPS, *o))
        else:
            check(lib.runet_bn_finalize(None, None, n, q, h * w, bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(),
                                        bn.running_var.data_ptr(), None, BN_MOMENTUM, BN_EPS, 0, *o))
    check(lib.runet_ms_stem_fwd(*src, *wts, scale.data_ptr(), shift.data_ptr(), out.data_ptr(), ops.ld(out), st))
    if not save:
        return out, None
    return out, dict(x=x_nchw, p=p, scale=scale, shift=shift, mean=mean, invstd=invstd, training=training, fused=True)


def ms_stem_backward(ctx, de, G, pre="", want_dt=False):
    """de [n, h, w, 64]: the gradient of the stem's output (an NHWC view).  Parameter gradients into G.  There is no input gradient (the input
    is the image).  want_dt: also return dt, the gradient of the four convolutions' outputs."""
    if not ctx["fused"]:
        keep = {}
        ms_block_backward(ctx, de, G, pre, need_dx=False, keep=keep)
        return keep["dt"] if want_dt else None
    p: MSBlockParams = ctx["p"]
    x = ctx["x"]
    n, _, h, w = x.shape
    dev, st = de.device, ops.stream()
    src, wts = _ms_src(x), _ms_wts(p)
    c, q = MS_STEM_C, MS_STEM_Q
    vec = (ctx["scale"].data_ptr(), ctx["shift"].data_ptr(), de.data_ptr(), ops.ld(de), ctx["mean"].data_ptr(), ctx["invstd"].data_ptr())
    sums = torch.empty(2 * c, device=dev, dtype=torch.float32)
    ws = scratch(lib.runet_ms_stem_workspace_floats(n, h, w), dev)
    check(lib.runet_ms_stem_bwd_reduce(*src, *wts, *vec, ws.data_ptr(), ws.numel(), sums.data_ptr(), st))
    use = dx_sums(sums, ctx["training"])[0]
    dt = torch.empty((n, h, w, c), device=dev, dtype=torch.float32)
    check(lib.runet_ms_stem_bwd_apply(*src, *wts, *vec, use.data_ptr(), 0, dt.data_ptr(), c, st))
    _ms_bn_grads(sums, q, G, pre)
    x4 = to_nhwc_pad(x, 4)
    xp, _ = maxpool3s1_forward(x4, want_idx=False)
    _ms_param_grads(x4, xp, dt, p, G, pre)
    return dt if want_dt else None


# =============================================================================== Fast-SCNN (csrc/fastscnn.hip, csrc/dwsep.hip)
# DepthwiseSeparableConv (comne.py:305-320): depthwise 3x3 (stride 1 | 2, no bias) -> pointwise 1x1 (no bias) -> BatchNorm2d -> ReLU.  Default:
# runet_dw3_fwd, then the shared 1x1 convolution and its weight gradient on the kept depthwise tensor.  RUNET_FUSED_DWSEP=1 (opt-in):
# runet_dwsep_fwd / runet_dwsep_wgrad_pw, the depthwise tensor exists in neither pass - measured SLOWER kernel by kernel at the 16 x 256^2 step's
# shapes (forward 29 / 16 / 30 us against 21 / 16 / 20, weight gradient 102 / 37 / 36 against 32 / 17 / 19; two step A/B runs disagree: the
# layers are so small that the fused kernels run 64 - 1024 blocks of one 64-pixel tile each behind a 6 - 64 KB weight load, DESIGN.md
# section 3.14), so it is the opt-in and the partner the default; RUNET_NO_FUSED_DWSEP=1 forces the partner whatever else is set.  Both share the
# rest of the backward: the pointwise data gradient through the shared 1x1 dgrad, runet_dw3_wgrad / runet_dw3_dgrad behind it.
# FeatureFusionModule (:403-427): RUNET_NO_FUSED_FFM=1 builds relu(bn(low) + upsample(bn(high))) from runet_bn_apply, runet_bn_bilinear_nhwc_fwd
# / runet_bilinear_nhwc_fwd and runet_add_inplace instead of runet_ffm_fwd.  Read like FUSED_MS_STEM.
FUSED_DWSEP = os.environ.get("RUNET_FUSED_DWSEP", "0") == "1" and os.environ.get("RUNET_NO_FUSED_DWSEP", "0") != "1"
FUSED_FFM = os.environ.get("RUNET_NO_FUSED_FFM", "0") != "1"
PYR_BINS = (1, 2, 3, 6)
PYR_OFF = (0, 1, 5, 14)      # cells of the branches in front of branch j, per image
PYR_ROWS = 50


def _out_hw(h, w, stride):
    return (h + stride - 1) // stride, (w + stride - 1) // stride


def dw3_forward(x, wd, stride, out=None):
    """x [n, h, w, c], wd [3, 3, 1, c] (HWIO) -> dwconv3x3(x), padding 1, [n, ceil(h / stride), ceil(w / stride), c]"""
    n, h, w, c = x.shape
    ho, wo = _out_hw(h, w, stride)
    if out is None:
        out = ops.empty_nhwc(n, ho, wo, c, x)
    check(lib.runet_dw3_fwd(x.data_ptr(), ops.ld(x), wd.data_ptr(), out.data_ptr(), ops.ld(out), n, h, w, c, stride, ops.stream()))
    return out


def dw3_wgrad(x, dy, stride):
    """-> the depthwise weight's gradient [3, 3, 1, c]"""
    n, h, w, c = x.shape
    ws = scratch(lib.runet_dw3_wgrad_workspace_floats(n, h, w, c, stride), x.device)
    dw = torch.empty((3, 3, 1, c), device=x.device, dtype=torch.float32)
    check(lib.runet_dw3_wgrad(x.data_ptr(), ops.ld(x), dy.data_ptr(), ops.ld(dy), ws.data_ptr(), ws.numel(), dw.data_ptr(), n, h, w, c, stride,
                              ops.stream()))
    return dw


def dw3_dgrad(dy, wd, h, w, stride, out=None):
    """dy [n, ceil(h / stride), ceil(w / stride), c] -> dx [n, h, w, c]"""
    n, _, _, c = dy.shape
    if out is None:
        out = ops.empty_nhwc(n, h, w, c, dy)
    check(lib.runet_dw3_dgrad(dy.data_ptr(), ops.ld(dy), wd.data_ptr(), out.data_ptr(), ops.ld(out), n, h, w, c, stride, ops.stream()))
    return out


class DWSepParams:
    """wd [3, 3, 1, cin] / wp [1, 1, cin, cout]: the depthwise and pointwise weights in their physical (HWIO) layout; bn: BNState"""
    __slots__ = ("wd", "wp", "bn", "stride")

    def __init__(self, wd, wp, bn, stride):
        self.wd, self.wp, self.bn, self.stride = wd, wp, bn, stride


def dwsep_fusable(cin, cout):
    return cin % 16 == 0 and cout % 16 == 0 and 16 <= cin <= 128 and 16 <= cout <= 128


def dwsep_conv(x, p: DWSepParams, want_stats, fused=None):
    """-> (t = pointwise(depthwise(x)), the depthwise tensor or None where it was never written, the BatchNorm statistics partials or None)"""
    n, h, w, cin = x.shape
    cout = p.wp.shape[3]
    if (FUSED_DWSEP if fused is None else fused) and dwsep_fusable(cin, cout):
        ho, wo = _out_hw(h, w, p.stride)
        t = ops.empty_nhwc(n, ho, wo, cout, x)
        nparts = lib.runet_dwsep_parts(n, h, w, p.stride)
        part = torch.empty(nparts * cout * 3, device=x.device, dtype=torch.float32)
        check(lib.runet_dwsep_fwd(x.data_ptr(), ops.ld(x), p.wd.data_ptr(), p.wp.data_ptr(), t.data_ptr(), ops.ld(t), part.data_ptr(), n, h, w, cin,
                                  cout, p.stride, ops.stream()))
        return t, None, dict(part=part, nparts=nparts)
    d = dw3_forward(x, p.wd, p.stride)
    fs = {} if want_stats else None
    return ops.conv_fwd(d, p.wp, None, stats=fs), d, fs


def dwsep_forward(x, p: DWSepParams, training, sm: Small, out=None, save=True, fused=None):
    """-> (relu(bn(pointwise(depthwise(x)))), written to `out` - a concat slice - when given; context or None)"""
    t, d, fs = dwsep_conv(x, p, training, fused)
    s, h, mean, invstd, _ = bn_coeff(t, p.bn, training, sm, fused=fs if training else None)
    a = bn_apply(t, s, h, None, relu=True, out=out)
    return a, (dict(x=x, d=d, t=t, s=s, h=h, mean=mean, invstd=invstd, p=p) if save else None)


def dwsep_wgrad_pw(x, wd, dt, stride):
    """the pointwise weight's gradient [1, 1, cin, cout] = d^T dt with d = dwconv(x) recomputed"""
    n, h, w, cin = x.shape
    cout = dt.shape[3]
    ws = scratch(lib.runet_dwsep_wgrad_pw_workspace_floats(n, h, w, cin, cout, stride), x.device)
    dwp = torch.empty((1, 1, cin, cout), device=x.device, dtype=torch.float32)
    check(lib.runet_dwsep_wgrad_pw(x.data_ptr(), ops.ld(x), wd.data_ptr(), dt.data_ptr(), ops.ld(dt), ws.data_ptr(), ws.numel(), dwp.data_ptr(), n, h,
                                   w, cin, cout, stride, ops.stream()))
    return dwp


def dwsep_backward(cx, da, G, pre, training, need_dx=True):
    """da: gradient of the activation.  G receives {pre}depthwise.weight, {pre}pointwise.weight, {pre}bn.weight / .bias (physical layouts).
    -> the gradient of the layer's input (None unless need_dx)"""
    p, x = cx["p"], cx["x"]
    n, h, w, cin = x.shape
    cout = p.wp.shape[3]
    sums = vec(2 * cout, da.device)
    dt = bn_backward(da, cx["t"], cx["mean"], cx["invstd"], cx["s"], sums, relu_shift=cx["h"], training=training)
    G[pre + "bn.weight"], G[pre + "bn.bias"] = sums[:cout], sums[cout:]
    if cx["d"] is None:
        G[pre + "pointwise.weight"] = dwsep_wgrad_pw(x, p.wd, dt, p.stride)
    else:
        G[pre + "pointwise.weight"] = ops.conv_wgrad(cx["d"], dt, 1, 1)
    dd = ops.conv_dgrad(dt, p.wp)
    G[pre + "depthwise.weight"] = dw3_wgrad(x, dd, p.stride)
    return dw3_dgrad(dd, p.wd, h, w, p.stride) if need_dx else None


class PPMParams:
    """ws [4] x [1, 1, c, c // 4] (HWIO), bs [4] x [c // 4], bns [4] x BNState: the four branches' Conv2d 1x1 and BatchNorm2d, bins 1 / 2 / 3 / 6"""
    __slots__ = ("ws", "bs", "bns")

    def __init__(self, ws, bs, bns):
        self.ws, self.bs, self.bns = ws, bs, bns


def _pyr_view(buf, j, n):
    b = PYR_BINS[j]
    return buf[n * PYR_OFF[j]:n * (PYR_OFF[j] + b * b)].view(n, b, b, buf.shape[1])


def ppm_forward(cat, p: PPMParams, training, sm: Small, save=True):
    """PyramidPoolingFastSCNN (comne.py:343-371).  cat [n, h, w, 2c]: channels [0, c) hold the module's input (written there by its producer),
    channels [c, 2c) receive the four resized branches - the reference's torch.cat without a copy.  -> context or None"""
    c = cat.shape[3] // 2
    cx = ppm_cells_forward(cat[..., :c], p, training, sm)
    n, h, w, _ = cx["shape"]
    up = cat[..., c:]
    check(lib.runet_pyramid_upsample_fwd(cx["acts"].data_ptr(), c // 4, up.data_ptr(), ops.ld(up), n, h, w, c // 4, ops.stream()))
    return cx if save else None


def ppm_cells_forward(x, p: PPMParams, training, sm: Small):
    """ppm_forward up to the activated branch cells, without the resize: x [n, h, w, c] (may be a channel slice).
    -> context with acts [50 n, c // 4], branch-major (_pyr_view)"""
    n, h, w, c = x.shape
    cq = c // 4
    st = ops.stream()
    pooled = torch.empty((PYR_ROWS * n, c), device=x.device, dtype=torch.float32)
    check(lib.runet_pyramid_pool_fwd(x.data_ptr(), ops.ld(x), pooled.data_ptr(), c, n, h, w, c, st))
    acts = torch.empty((PYR_ROWS * n, cq), device=x.device, dtype=torch.float32)
    br = []
    for j in range(4):
        pj = _pyr_view(pooled, j, n)
        fs = {} if training else None
        t = ops.conv_fwd(pj, p.ws[j], p.bs[j], stats=fs)
        s, hh, mean, invstd, _ = bn_coeff(t, p.bns[j], training, sm, fused=fs)
        bn_apply(t, s, hh, None, relu=True, out=_pyr_view(acts, j, n))
        br.append(dict(x=pj, w=p.ws[j], t=t, s=s, h=hh, mean=mean, invstd=invstd))
    return dict(br=br, acts=acts, shape=(n, h, w, c))


def ppm_backward(cx, dcat, G, pre, training):
    """dcat [n, h, w, 2c]: the gradient of the concat.  G receives {pre}convs.{j}.1.weight / .bias (the 1x1 convolutions) and
    {pre}convs.{j}.2.weight / .bias (the BatchNorms).  -> the gradient of the module's input [n, h, w, c]"""
    n, h, w, c = cx["shape"]
    cq = c // 4
    dup = dcat[..., c:]
    dacts = torch.empty((PYR_ROWS * n, cq), device=dcat.device, dtype=torch.float32)
    check(lib.runet_pyramid_upsample_bwd(dup.data_ptr(), ops.ld(dup), dacts.data_ptr(), cq, n, h, w, cq, ops.stream()))
    return ppm_cells_backward(cx, dacts, dcat[..., :c], G, pre, training)


def ppm_cells_backward(cx, dacts, direct, G, pre, training):
    """ppm_backward behind the resize's adjoint: dacts [50 n, c // 4] the gradient of the activated branch cells, direct [n, h, w, c] (may be
    a channel slice) the gradient that reaches the module's input beside the pyramid.  -> the gradient of the module's input"""
    n, h, w, c = cx["shape"]
    cq = c // 4
    dev = dacts.device
    st = ops.stream()
    dpooled = torch.empty((PYR_ROWS * n, c), device=dev, dtype=torch.float32)
    for j, b in enumerate(cx["br"]):
        sums = vec(2 * cq, dev)
        dt = bn_backward(_pyr_view(dacts, j, n), b["t"], b["mean"], b["invstd"], b["s"], sums, relu_shift=b["h"], training=training)
        G[f"{pre}convs.{j}.2.weight"], G[f"{pre}convs.{j}.2.bias"] = sums[:cq], sums[cq:]
        G[f"{pre}convs.{j}.1.weight"] = ops.conv_wgrad(b["x"], dt, 1, 1)
        G[f"{pre}convs.{j}.1.bias"] = chan_sum(dt, vec(cq, dev))
        ops.conv_dgrad(dt, b["w"], out=_pyr_view(dpooled, j, n))
    dx = ops.empty_nhwc(n, h, w, c, direct)
    check(lib.runet_pyramid_pool_bwd(dpooled.data_ptr(), c, direct.data_ptr(), ops.ld(direct), dx.data_ptr(), ops.ld(dx), n, h, w, c, st))
    return dx


_ones_vec = {}


def _ones(n, device):
    buf = _ones_vec.get(device.index)
    if buf is None or buf.numel() < n:
        buf = torch.ones(max(int(n), 4096), device=device, dtype=torch.float32)
        _ones_vec[device.index] = buf
    return buf


def ffm_forward(t_low, coef_low, t_high, coef_high, s, fused=None):
    """FeatureFusionModule.forward (comne.py:421-427) behind its two 1x1 convolutions: t_low [n, s h, s w, c] and t_high [n, h, w, c] are their
    raw outputs, coef_* = (scale, shift) of the BatchNorms.  -> y = relu(bn(t_low) + upsample_s(bn(t_high)))"""
    n, h, w, c = t_high.shape
    if tuple(t_low.shape) != (n, s * h, s * w, c):
        raise ValueError(f"ffm_forward: t_low {tuple(t_low.shape)} is not {s} x {tuple(t_high.shape)}")
    (sl, hl), (sh, hh) = coef_low, coef_high
    if FUSED_FFM if fused is None else fused:
        y = ops.empty_nhwc(n, s * h, s * w, c, t_low)
        check(lib.runet_ffm_fwd(t_low.data_ptr(), ops.ld(t_low), t_high.data_ptr(), ops.ld(t_high), sl.data_ptr(), hl.data_ptr(), sh.data_ptr(),
                                hh.data_ptr(), y.data_ptr(), ops.ld(y), n, h, w, s, c, ops.stream()))
        return y
    y = bn_apply(t_low, sl, hl)
    up = ops.empty_nhwc(n, s * h, s * w, c, t_low)
    if s in (2, 4):
        bn_bilinear_forward(t_high, sh, hh, up, s, fused=True)
    else:
        _bilinear_nhwc(bn_apply(t_high, sh, hh), up)
    check(lib.runet_add_inplace(y.data_ptr(), up.data_ptr(), y.numel(), ops.stream()))
    return bn_apply(y, _ones(c, y.device), zeros(c, y.device), None, relu=True, out=y)


def ffm_backward(dy, y, t_low, st_low, t_high, st_high, s, sums_low, sums_high, training=True):
    """st_* = (mean, invstd, scale) of the two BatchNorms, sums_* [2c] receive their (dgamma | dbeta).
    -> (dt_low [n, s h, s w, c], dt_high [n, h, w, c]): the gradients of the two 1x1 convolutions' outputs"""
    n, ho, wo, c = y.shape
    g = ops.empty_nhwc(n, ho, wo, c, y)
    check(lib.runet_relu_mask_nhwc(dy.data_ptr(), ops.ld(dy), y.data_ptr(), ops.ld(y), g.data_ptr(), ops.ld(g), n * ho * wo, c, ops.stream()))
    ml, il, sl = st_low
    mh, ih, sh = st_high
    dt_high = bn_bilinear_backward(g, t_high, mh, ih, sh, sums_high, s, training=training, fused=s in (2, 4))
    dt_low = bn_backward(g, t_low, ml, il, sl, sums_low, out=g, training=training)
    return dt_low, dt_high


def up_sigmoid_forward(z, s):
    """z [n, h, w] (the logit plane) -> sigmoid(upsample_s(z)) [n, 1, s h, s w]"""
    n, h, w = z.shape
    prob = torch.empty((n, 1, s * h, s * w), device=z.device, dtype=torch.float32)
    check(lib.runet_up_sigmoid_fwd(z.data_ptr(), prob.data_ptr(), n, h, w, s, ops.stream()))
    return prob


def up_sigmoid_backward(dprob, prob, s):
    n, _, ho, wo = prob.shape
    dz = torch.empty((n, ho // s, wo // s), device=prob.device, dtype=torch.float32)
    check(lib.runet_up_sigmoid_bwd(dprob.data_ptr(), prob.data_ptr(), dz.data_ptr(), n, ho // s, wo // s, s, ops.stream()))
    return dz


# =============================================================================== ENet baseline (comne.py:482-608; csrc/enet.hip)
# RUNET_NO_FUSED_ENET_INITIAL=1: the initial block from the shared kernels (runet_to_nhwc_pad, runet_conv2d_general with the weight zero-padded
# to 16 columns, runet_maxpool2_fwd, runet_copy_nhwc, bn_coeff's own statistics pass, runet_conv_wgrad_general) - the A/B partner of
# runet_enet_initial_*.  RUNET_NO_FUSED_ENET_TAIL=1: the bottleneck's tail from the shared kernels (runet_bn_apply, runet_add_inplace,
# runet_relu_mask_nhwc and bn_backward per BatchNorm) - the A/B partner of runet_enet_tail_*.  Read at import.
FUSED_ENET_INITIAL = os.environ.get("RUNET_NO_FUSED_ENET_INITIAL", "0") != "1"
FUSED_ENET_TAIL = os.environ.get("RUNET_NO_FUSED_ENET_TAIL", "0") != "1"


class BottleneckParams:
    """Physical handles of one BottleneckBlock.  w1 / w3 / wd: HWIO 1x1 weights (wd, bnd: conv_down, None for a plain block); conv2:
    [(HWIO weight, BNState, (pad_h, pad_w), (dil_h, dil_w))], one entry, or two for the asymmetric block; drop: the Dropout2d holder."""
    __slots__ = ("w1", "bn1", "conv2", "w3", "bn3", "wd", "bnd", "drop", "cout")

    def __init__(self, w1, bn1, conv2, w3, bn3, wd, bnd, drop, cout):
        self.w1, self.bn1, self.conv2, self.w3, self.bn3, self.wd, self.bnd, self.drop, self.cout = w1, bn1, conv2, w3, bn3, wd, bnd, drop, cout


def enet_initial_forward(x_nchw, w13, bn: BNState, training, sm: Small, save=True, fused=None):
    """InitialBlock.forward (comne.py:492-497): relu(bn(cat([conv3x3 s2 p1 (x), maxpool2(x)]))).  w13: HWIO [3, 3, 3, 13].
    Fused (runet_enet_initial_fwd): one pass over the NCHW image writes the 16-wide t and its BatchNorm partials.  Partner (shared kernels):
    the convolution runs with the weight zero-padded to 16 output columns into the 16-wide buffer t, the pool's three channels are copied
    over columns 13..15, bn_coeff takes its own statistics pass.  -> (a [n, H/2, W/2, 16], context)"""
    n, _, H, W = x_nchw.shape
    if FUSED_ENET_INITIAL if fused is None else fused:
        t = ops.empty_nhwc(n, H // 2, W // 2, 16, x_nchw)
        fs = {}
        sp = ops._stats_buf(fs, lib.runet_enet_initial_parts(n, H, W), 16, x_nchw.device)
        sn, sc, sh, sw = x_nchw.stride()
        check(lib.runet_enet_initial_fwd(x_nchw.data_ptr(), sn, sc, sh, sw, w13.data_ptr(), t.data_ptr(), 16, sp, n, H, W, ops.stream()))
        s, h, mean, invstd, _ = bn_coeff(t, bn, training, sm, fused=fs)
        a = bn_apply(t, s, h, None, relu=True)
        return a, (dict(x=x_nchw, t=t, s=s, h=h, mean=mean, invstd=invstd) if save else None)
    xp = to_nhwc_pad(x_nchw, 4)
    w16 = torch.zeros((3, 3, 3, 16), device=xp.device, dtype=torch.float32)
    w16[..., :13].copy_(w13)
    t = ops.empty_nhwc(n, H // 2, W // 2, 16, xp)
    ops.conv_general_fwd(xp, w16, None, 2, 1, out=t)
    pooled, _ = maxpool_forward(xp)
    check(lib.runet_copy_nhwc(pooled.data_ptr(), ops.ld(pooled), t[..., 13:].data_ptr(), 16, n * (H // 2) * (W // 2), 3, ops.stream()))
    s, h, mean, invstd, _ = bn_coeff(t, bn, training, sm)
    a = bn_apply(t, s, h, None, relu=True)
    return a, (dict(xp=xp, t=t, s=s, h=h, mean=mean, invstd=invstd) if save else None)


def enet_initial_backward(cx, da, G, pre, training):
    """da: gradient of the block's output (overwritten).  G[pre + "conv.weight"] (HWIO [3, 3, 3, 13]), G[pre + "bn.weight" / "bn.bias"]."""
    sums = vec(32, da.device)
    dt = bn_backward(da, cx["t"], cx["mean"], cx["invstd"], cx["s"], sums, relu_shift=cx["h"], out=da, training=training)
    G[pre + "bn.weight"], G[pre + "bn.bias"] = sums[:16], sums[16:]
    if "x" in cx:          # the fused forward kept the image itself
        x = cx["x"]
        n, _, H, W = x.shape
        dw = torch.empty((3, 3, 3, 13), device=da.device, dtype=torch.float32)
        sn, sc, sh, sw = x.stride()

        def run():
            ws = scratch(lib.runet_enet_initial_wgrad_workspace_floats(n, H, W), da.device)
            check(lib.runet_enet_initial_wgrad(x.data_ptr(), sn, sc, sh, sw, dt.data_ptr(), ops.ld(dt), ws.data_ptr(), ws.numel(), dw.data_ptr(), n, H, W,
                                               ops.stream()))
            return dw
        G[pre + "conv.weight"] = ops._on_side(run, (x, dt, dw)) if ops.side_stream() is not None else run()
        return
    dw16 = ops.conv_general_wgrad(cx["xp"], dt, 3, 3, 2, 1, cin_w=3)
    G[pre + "conv.weight"] = dw16[..., :13].contiguous()


def enet_tail_forward(t3, coef3, idn, coef_d=None, mask=None, fused=None):
    """out = relu(mask * (t3 * scale3 + shift3) + id); id = idn (plain) or idn * scale_d + shift_d (coef_d given: the downsample block)."""
    n, h, w, c = t3.shape
    if tuple(idn.shape) != tuple(t3.shape):
        raise ValueError(f"enet_tail_forward: identity {tuple(idn.shape)} against main branch {tuple(t3.shape)}")
    s3, h3 = coef3
    if FUSED_ENET_TAIL if fused is None else fused:
        out = ops.empty_nhwc(n, h, w, c, t3)
        sd, hd = coef_d if coef_d is not None else (None, None)
        check(lib.runet_enet_tail_fwd(t3.data_ptr(), ops.ld(t3), idn.data_ptr(), ops.ld(idn), s3.data_ptr(), h3.data_ptr(),
                                      sd.data_ptr() if sd is not None else None, hd.data_ptr() if hd is not None else None,
                                      mask.data_ptr() if mask is not None else None, out.data_ptr(), ops.ld(out), n, h, w, c, ops.stream()))
        return out
    y = bn_apply(t3, s3, h3, mask, relu=False)
    idb = bn_apply(idn, coef_d[0], coef_d[1]) if coef_d is not None else idn
    check(lib.runet_add_inplace(y.data_ptr(), idb.data_ptr(), y.numel(), ops.stream()))
    return bn_apply(y, _ones(c, y.device), zeros(c, y.device), None, relu=True, out=y)


def enet_tail_backward(dout, out, t3, st3, idn=None, st_d=None, mask=None, training=True, fused=None):
    """st3 / st_d = (mean, invstd, scale) of conv3's / conv_down's BatchNorm (st_d and idn: the downsample block).
    -> (dt3, did, sums3 [2c], sums_d [2c] or None): did is dt_d, the gradient of conv_down's raw output, or for the plain block g = dout
    where out > 0, the identity's gradient onto which the caller accumulates conv1's data gradient."""
    n, h, w, c = t3.shape
    dev = t3.device
    m3, i3, s3 = st3
    down = st_d is not None
    if FUSED_ENET_TAIL if fused is None else fused:
        sums = vec((4 if down else 2) * c, dev)
        md, idv, sd = st_d if down else (None, None, None)
        p = lambda t: t.data_ptr() if t is not None else None
        ldi = ops.ld(idn) if idn is not None else 0
        ws = scratch(lib.runet_enet_tail_bwd_workspace_floats(n, h, w, c, int(down)), dev)
        check(lib.runet_enet_tail_bwd_reduce(dout.data_ptr(), ops.ld(dout), out.data_ptr(), ops.ld(out), t3.data_ptr(), ops.ld(t3), p(idn), ldi,
                                             m3.data_ptr(), i3.data_ptr(), p(md), p(idv), p(mask), ws.data_ptr(), ws.numel(), sums.data_ptr(), n, h, w,
                                             c, ops.stream()))
        use = dx_sums(sums, training)[0]
        dt3, did = ops.empty_nhwc(n, h, w, c, t3), ops.empty_nhwc(n, h, w, c, t3)
        check(lib.runet_enet_tail_bwd_apply(dout.data_ptr(), ops.ld(dout), out.data_ptr(), ops.ld(out), t3.data_ptr(), ops.ld(t3), p(idn), ldi,
                                            m3.data_ptr(), i3.data_ptr(), s3.data_ptr(), p(md), p(idv), p(sd), p(mask), use.data_ptr(), 0,
                                            dt3.data_ptr(), ops.ld(dt3), did.data_ptr(), ops.ld(did), n, h, w, c, ops.stream()))
        return dt3, did, sums[:2 * c], (sums[2 * c:] if down else None)
    g = ops.empty_nhwc(n, h, w, c, t3)
    check(lib.runet_relu_mask_nhwc(dout.data_ptr(), ops.ld(dout), out.data_ptr(), ops.ld(out), g.data_ptr(), ops.ld(g), n * h * w, c, ops.stream()))
    # runet_bn_bwd_reduce reads mask_nc only together with a ReLU decision (act or relu_shift): the Dropout2d factor is applied in front
    gm = bn_apply(g, _ones(c, dev), zeros(c, dev), mask) if mask is not None else g
    sums3 = vec(2 * c, dev)
    dt3 = bn_backward(gm, t3, m3, i3, s3, sums3, training=training)
    if not down:
        return dt3, g, sums3, None
    sums_d = vec(2 * c, dev)
    md, idv, sd = st_d
    return dt3, bn_backward(g, idn, md, idv, sd, sums_d, out=g, training=training), sums3, sums_d


def enet_head_forward(x, w, b):
    """decoder.6 + sigmoid: ConvTranspose2d(c, 1, 2, stride 2); w: the parameter's physical [2, 2, c, 1].  x [n, h, w, c] -> prob [n, 1, 2h, 2w]"""
    n, h, wd, c = x.shape
    prob = torch.empty((n, 1, 2 * h, 2 * wd), device=x.device, dtype=torch.float32)
    check(lib.runet_enet_head_fwd(x.data_ptr(), ops.ld(x), w.data_ptr(), b.data_ptr(), prob.data_ptr(), n, h, wd, c, ops.stream()))
    return prob


def enet_head_backward(dprob, prob, x, w, sink, pre=""):
    """-> dx; the sink receives pre + "weight" ([2, 2, c, 1]) and pre + "bias" out of one fixed-order buffer"""
    n, h, wd, c = x.shape
    dx = ops.empty_nhwc(n, h, wd, c, x)
    dw_db = sink.buf(pre, [("weight", (2, 2, c, 1)), ("bias", (1,))])
    ws = scratch(lib.runet_enet_head_bwd_workspace_floats(n, h, wd, c), x.device)
    check(lib.runet_enet_head_bwd(dprob.data_ptr(), prob.data_ptr(), x.data_ptr(), ops.ld(x), w.data_ptr(), dx.data_ptr(), ops.ld(dx), ws.data_ptr(),
                                  ws.numel(), dw_db.data_ptr(), n, h, wd, c, ops.stream()))
    return dx


# =============================================================================== PSPNet baseline (comne.py:214-299; csrc/pspnet.hip)
# final_conv.0 convolves cat[x, up(P_1), up(P_2), up(P_3), up(P_6)].  Tap planes: the pyramid half of that convolution on the 50 cells per
# image (Z_j = P_j . Wtap_j through the shared 1x1 convolution, runet_psp_taps_fwd adds the shifted, resized planes onto the 3x3 convolution
# of x alone); no concat buffer, no upsampled channels, half the matrix work of the layer in all three passes.  Head: BatchNorm, ReLU,
# Dropout2d and the 1x1 convolution in one pass (runet_psp_head_*).  Both are OPT-IN (RUNET_FUSED_PSP_TAPS=1, RUNET_FUSED_PSP_HEAD=1): in
# the 16 x 256^2 step neither gain - the tap planes over the reference's order on the shared kernels (the concat buffer,
# runet_pyramid_upsample_*, one 3x3 convolution 2c -> cout), the head over runet_bn_apply + runet_outc_* - was larger than the
# round-to-round spread.  RUNET_NO_FUSED_PSP_TAPS=1 / RUNET_NO_FUSED_PSP_HEAD=1 force the default.  Read at import.
FUSED_PSP_TAPS = os.environ.get("RUNET_FUSED_PSP_TAPS", "0") == "1" and os.environ.get("RUNET_NO_FUSED_PSP_TAPS", "0") != "1"
FUSED_PSP_HEAD = os.environ.get("RUNET_FUSED_PSP_HEAD", "0") == "1" and os.environ.get("RUNET_NO_FUSED_PSP_HEAD", "0") != "1"
PSP_HEAD_SCALE = 16


def psp_split_weights(w_hwio, cache):
    """final_conv.0's weight [3, 3, 2c, cout] (the parameter's physical view) -> (wx [3, 3, c, cout]: the rows that meet x; wp [1, 1, c, 9 cout]:
    the rows that meet the pyramid, input channel outermost, so branch j's Wtap_j [c // 4, 9 cout] is the contiguous block wp[:, :, j c/4 : (j + 1) c/4]).
    Copies kept in `cache` (the model's dict) and rewritten in place, on the current stream, when the parameter has changed (its version
    counter or ops.WEIGHT_EPOCH): call it before ops.prefetch_derived(), whose refills of the derived forms of wx / wp then follow the copy
    in stream order.  The copies go through torch, so their own version counters move and ops._cached sees them as new."""
    base = w_hwio._base if w_hwio._base is not None else w_hwio
    kh, kw, c2, cout = w_hwio.shape
    c = c2 // 2
    tag = (base._version, ops.WEIGHT_EPOCH, w_hwio.data_ptr(), tuple(w_hwio.shape))
    if cache.get("tag") != tag:
        if "wx" not in cache or cache["wx"].device != w_hwio.device or tuple(cache["wx"].shape) != (kh, kw, c, cout):
            cache["wx"] = torch.empty((kh, kw, c, cout), device=w_hwio.device, dtype=torch.float32)
            cache["wp"] = torch.empty((1, 1, c, kh * kw * cout), device=w_hwio.device, dtype=torch.float32)
        with torch.no_grad():
            cache["wx"].copy_(w_hwio[:, :, :c, :])
            cache["wp"].view(c, kh, kw, cout).copy_(w_hwio[:, :, c:, :].permute(2, 0, 1, 3))
        cache["tag"] = tag
    return cache["wx"], cache["wp"]


def psp_join_wgrad(dwx, dwp):
    """the two halves' weight gradients -> one [3, 3, 2c, cout] tensor in the parameter's physical layout.  Inside the backward pass the
    halves are written on the weight-gradient stream, so the two copies go there too (torch-level switch: they are torch copies)."""
    kh, kw, c, cout = dwx.shape
    g = torch.empty((kh, kw, 2 * c, cout), device=dwx.device, dtype=torch.float32)

    def run():
        g[:, :, :c, :].copy_(dwx)
        g[:, :, c:, :].copy_(dwp.view(c, kh, kw, cout).permute(1, 2, 0, 3))
        return g
    if ops.side_stream() is None:
        return run()
    prev = ops._side.get("torch_switch")
    ops._side["torch_switch"] = True
    try:
        return ops._on_side(run, (dwx, dwp, g))
    finally:
        ops._side["torch_switch"] = prev


def psp_taps_forward(t, acts, wp):
    """t [n, h, w, cout] (may be a channel slice) += the pyramid half of the 3x3 convolution: acts [50 n, cq] the activated branch cells
    (ppm_cells_forward), wp [1, 1, 4 cq, 9 cout] (psp_split_weights).  -> t"""
    n, h, w, cout = t.shape
    cq = acts.shape[1]
    z = torch.empty((PYR_ROWS * n, 9 * cout), device=t.device, dtype=torch.float32)
    for j in range(4):
        ops.conv_fwd(_pyr_view(acts, j, n), wp[:, :, j * cq:(j + 1) * cq, :], None, out=_pyr_view(z, j, n))
    check(lib.runet_psp_taps_fwd(z.data_ptr(), 9 * cout, t.data_ptr(), ops.ld(t), n, h, w, cout, ops.stream()))
    return t


def psp_taps_backward(dt, acts, wp):
    """dt [n, h, w, cout]: the gradient of the 3x3 convolution's output.  -> (dacts [50 n, cq], dwp shaped like wp)"""
    n, h, w, cout = dt.shape
    cq = acts.shape[1]
    dev = dt.device
    dz = torch.empty((PYR_ROWS * n, 9 * cout), device=dev, dtype=torch.float32)
    ws = scratch(lib.runet_psp_taps_bwd_workspace_floats(n, h, w, cout), dev)
    check(lib.runet_psp_taps_bwd(dt.data_ptr(), ops.ld(dt), dz.data_ptr(), 9 * cout, ws.data_ptr(), ws.numel(), n, h, w, cout, ops.stream()))
    dacts = torch.empty((PYR_ROWS * n, cq), device=dev, dtype=torch.float32)
    dwp = torch.empty_like(wp)
    for j in range(4):
        ops.conv_wgrad(_pyr_view(acts, j, n), _pyr_view(dz, j, n), 1, 1, out=dwp[:, :, j * cq:(j + 1) * cq, :])
    # dP = dZ . Wtap^T is 100 K outputs behind a 9 cout deep contraction: a few tiles of the shared data gradient, each walking all of it
    # (572 us for the four branches at the 16 x 256^2 workload); runet_psp_taps_dp splits the contraction by tap
    ws = scratch(lib.runet_psp_taps_dp_workspace_floats(n, cq), dev)
    check(lib.runet_psp_taps_dp(dz.data_ptr(), 9 * cout, wp.data_ptr(), 9 * cout, ws.data_ptr(), ws.numel(), dacts.data_ptr(), cq, n, cq, cout,
                                ops.stream()))
    return dacts, dwp


def psp_head_forward(t, scale, shift, mask, w, b, fused=None):
    """sigmoid(upsample16(conv1x1(dropout(relu(t * scale + shift))))) -> (prob [n, 1, 16 h, 16 w], saved).  t [n, h, w, c]: final_conv.0's raw
    output, mask [n, c] or None, w: the 1x1 convolution's physical [1, 1, c, 1], b [1].  Fused: saved = None (the backward needs t and prob);
    partner: saved = the activation [n, h, w, c]."""
    n, h, wd, c = t.shape
    if FUSED_PSP_HEAD if fused is None else fused:
        z = torch.empty((n, h, wd), device=t.device, dtype=torch.float32)
        check(lib.runet_psp_head_fwd(t.data_ptr(), ops.ld(t), scale.data_ptr(), shift.data_ptr(), mask.data_ptr() if mask is not None else None,
                                     w.data_ptr(), b.data_ptr(), z.data_ptr(), n, h, wd, c, ops.stream()))
        return up_sigmoid_forward(z, PSP_HEAD_SCALE), None
    a = bn_apply(t, scale, shift, mask, relu=True)
    _, logit = outc_forward(a, w, b, want_logit=True)
    return up_sigmoid_forward(logit.view(n, h, wd), PSP_HEAD_SCALE), a


def psp_head_backward(dprob, prob, t, scale, shift, mask, w, mean, invstd, saved=None, training=True):
    """-> (dt [n, h, w, c], out [3c + 1] = (dgamma | dbeta | dw | db)); saved: what psp_head_forward returned (None = the fused path)"""
    n, h, wd, c = t.shape
    dev = t.device
    st = ops.stream()
    out = torch.empty(3 * c + 1, device=dev, dtype=torch.float32)
    dz = up_sigmoid_backward(dprob, prob, PSP_HEAD_SCALE)
    mp = mask.data_ptr() if mask is not None else None
    if saved is None:
        ws = scratch(lib.runet_psp_head_bwd_workspace_floats(n, h, wd, c), dev)
        check(lib.runet_psp_head_bwd_reduce(dz.data_ptr(), t.data_ptr(), ops.ld(t), scale.data_ptr(), shift.data_ptr(), mp, w.data_ptr(), mean.data_ptr(),
                                            invstd.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(), n, h, wd, c, st))
        use = dx_sums(out, training)[0]
        dt = ops.empty_nhwc(n, h, wd, c, t)
        check(lib.runet_psp_head_bwd_apply(dz.data_ptr(), t.data_ptr(), ops.ld(t), mp, w.data_ptr(), dt.data_ptr(), ops.ld(dt), n, h, wd, c, mean.data_ptr(),
                                           invstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), use.data_ptr(), 0, st))
        return dt, out
    da = ops.empty_nhwc(n, h, wd, c, t)
    check(lib.runet_outc_bwd(dz.data_ptr(), None, saved.data_ptr(), ops.ld(saved), w.data_ptr(), da.data_ptr(), ops.ld(da), _ws(n, h * wd, c, dev).data_ptr(),
                             out[2 * c:].data_ptr(), n * h * wd, c, st))
    dt = bn_backward(da, t, mean, invstd, scale, out[:2 * c], mask=mask, relu_shift=shift, out=da, training=training)
    return dt, out
