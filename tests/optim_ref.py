"""Float64 reference for FusedAdam past the first step, a float32 restatement with named mistakes, and the one comparison
(`check_adam`) that tests/test_gpu_optim.py uses.  CPU only; tests/test_optim_ref_cpu.py checks this file against torch.optim.Adam.

Why more than one step: at step 1 Adam's update is -lr * g / (|g| + eps) whatever the betas are, so swapped betas, a missing
bias correction, eps inside the square root, decoupled decay and moments that are never written back all pass a one-step test.

Inputs (`make_inputs`): SIZES = the chunk edges of the kernel (16384 elements per block, four floats per lane) plus 200 tensors of
1..64 elements; parameters N(0, 1); gradients redrawn every step with magnitudes log-uniform over 1e-10 .. 1e2 and random signs;
element 1 of every tensor with >= 4 elements has p = 0 and g = 0 at every step (0 / (0 + eps) must stay 0), element 2 has g = 0 at
every step, and about 1 % of the other gradient elements are exact zeros.

What "close" means (`check_adam`): for p, max |p - p_ref| as a multiple of the learning rate in force at that step; for exp_avg
and exp_avg_sq, per tensor, max |x - x_ref| / max |x_ref|, and the largest such ratio over the tensors (a reference tensor that is
all zero must be matched exactly).

LIMITS are NOT taken from what the kernels give.  They are 4 x the distance between the two CPU statements of the rule in this
file: the unmutated float32 restatement against the float64 reference, the largest value over every scenario of SCENARIOS at
every step (`measure()`).  The factor 4 is for what the GPU may do differently within float32: contraction to FMAs and its own
sqrtf / division sequences, a few ulps per step.  Measured on the CPU (tests/test_optim_ref_cpu.py repeats the measurement and
fails if it has moved by more than a factor 2 either way, or if 4 x the p figure passes 0.05 lr):

    p  3.77e-03 lr     (steps 7..12, where lr is 2.5e-4: 9.4e-7 absolute, two ulps of |p| ~ 4; 6e-4 lr while lr is 1e-3)
    m  1.72e-06        (per tensor, so a small tensor whose two terms nearly cancel counts in full)
    v  3.39e-07

so LIMITS = {p: 1.51e-2 lr, m: 6.88e-6, v: 1.36e-6}; the p limit is below the 0.05 lr this suite allows itself at most.
Each mistake of MUTANTS, put into the restatement, is rejected at these limits (weight_decay 1e-4, the checked steps 1, 2, 6, 7
and 12): in p the weakest is `swap_betas` with 4.1 lr at step 12 (0.057 lr at step 2), the others reach 19 .. 490 lr; at step 1
`swap_betas` and `moments_not_stored` are exact in p (1.2e-4 lr) and show in m and v only (0.99 and 1.0 of the tensor's maximum).
"""
import importlib
import math

import numpy as np
import torch

oracle = importlib.import_module("oracle.robust_unet_ref")

CHUNK = 16384
SIZES = (1, 3, 4, 5, 255, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7) + tuple(1 + (29 * i) % 64 for i in range(200))
LATE = 7                      # index of the parameter (16385 elements: two blocks) whose first gradient arrives at call 4 in "late"
CHECK_STEPS = (1, 2, 6, 7, 12)
MUTANTS = ("swap_betas", "no_bc1", "no_bc2", "eps_inside_sqrt", "decoupled_decay", "moments_not_stored")

MEASURED = {"p": 3.77e-3, "m": 1.72e-6, "v": 3.39e-7}
LIMITS = {k: 4 * x for k, x in MEASURED.items()}


def f32(x):
    """The double that a float argument of the C ABI holds."""
    return float(np.float32(x))


def hyper(weight_decay=1e-4, grad_scale=1.0, lr=1e-3, lr_schedule=None):
    """lr_schedule: {call number (1-based): learning rate from that call on}."""
    return dict(lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay, grad_scale=grad_scale, lr_schedule=dict(lr_schedule or {}))


# name -> hyper-parameters, number of calls, skipped calls, index of the parameter without a gradient in calls 1-3
SCENARIOS = {}
for _wd in (0.0, 1e-4):
    for _gs in (1.0, 1.0 / 1024):
        SCENARIOS[f"matrix-wd{_wd:g}-gs{_gs:g}"] = dict(hyper=hyper(_wd, _gs, lr_schedule={7: 2.5e-4}), steps=12, skip=(), late=None)
SCENARIOS["skip"] = dict(hyper=hyper(), steps=8, skip=(4,), late=None)
SCENARIOS["late"] = dict(hyper=hyper(), steps=8, skip=(), late=LATE)
SCENARIOS["resume"] = dict(hyper=hyper(), steps=6, skip=(), late=None)


_STARTS = np.cumsum((0,) + SIZES[:-1])
_ZERO_PG = torch.tensor([int(o) + 1 for o, n in zip(_STARTS, SIZES) if n >= 4])       # p = 0 and g = 0 at every step
_ZERO_G = _ZERO_PG + 1                                                                # g = 0 at every step
_INPUTS = {}


def make_inputs(steps=12, seed=11):
    """-> (params, grad_seq): float32 CPU tensors, grad_seq[k][i] the gradient of parameter i in call k + 1.  The first `steps` calls
    of a longer sequence are the same tensors.  Shared between callers: do not write into them."""
    if (steps, seed) not in _INPUTS:
        g = torch.Generator().manual_seed(seed)
        total = sum(SIZES)
        p = torch.randn(total, generator=g)
        p[_ZERO_PG] = 0.0
        grad_seq = []
        for _ in range(steps):
            mag = torch.pow(10.0, torch.rand(total, generator=g, dtype=torch.float64) * 12.0 - 10.0)
            sign = torch.where(torch.rand(total, generator=g) < 0.5, -1.0, 1.0).double()
            gr = (mag * sign).float()
            gr[torch.rand(total, generator=g) < 0.01] = 0.0
            gr[_ZERO_PG] = 0.0
            gr[_ZERO_G] = 0.0
            grad_seq.append(list(gr.split(SIZES)))
        _INPUTS[(steps, seed)] = (list(p.split(SIZES)), grad_seq)
    params, grad_seq = _INPUTS[(steps, seed)]
    return list(params), [list(gs) for gs in grad_seq]


def scenario_inputs(name):
    """-> (params, grad_seq) as the optimizer under test and both CPU statements are given them."""
    sc = SCENARIOS[name]
    params, grad_seq = make_inputs(sc["steps"])
    mult = 1.0 / sc["hyper"]["grad_scale"]
    if mult != 1.0:           # a loss scale: the gradients arrive multiplied by it (1024: exact) and grad_scale divides it out
        grad_seq = [[g * mult for g in grads] for grads in grad_seq]
    if sc["late"] is not None:
        for k in range(3):
            grad_seq[k][sc["late"]] = None
    return params, grad_seq


def _lr_at(hp, call):
    lr = hp["lr"]
    for c in sorted(hp["lr_schedule"]):
        if call >= c:
            lr = hp["lr_schedule"][c]
    return lr


def _run(params, grad_seq, hp, skip, count_skipped, dtype, update):
    """Parameters and moments live in one flat tensor each; consecutive parameters at the same step count are updated together."""
    sizes = [t.numel() for t in params]
    ends = np.cumsum(sizes).tolist()
    p = torch.cat([t.detach().reshape(-1) for t in params]).to(dtype)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    step = [0] * len(sizes)
    snaps = []
    for call, grads in enumerate(grad_seq, start=1):
        lr = _lr_at(hp, call)
        live = [g is not None for g in grads]
        if call in skip:
            step = [s + 1 if (count_skipped and l) else s for s, l in zip(step, live)]
        else:
            step = [s + 1 if l else s for s, l in zip(step, live)]
            g = torch.cat([torch.zeros(n) if gr is None else gr.reshape(-1) for gr, n in zip(grads, sizes)]).to(dtype)
            i = 0
            while i < len(sizes):
                j = i
                while j + 1 < len(sizes) and live[j + 1] == live[i] and step[j + 1] == step[i]:
                    j += 1
                lo, hi = ends[i] - sizes[i], ends[j]
                if live[i]:
                    update(p[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi], step[i], lr)
                i = j + 1
        snaps.append(dict(p=list(p.clone().split(sizes)), m=list(m.clone().split(sizes)), v=list(v.clone().split(sizes)),
                          step=list(step), lr=lr))
    return snaps


def adam_reference(params, grad_seq, hyper, skip=(), count_skipped=False):
    """torch.optim.Adam's rule in float64 (L2-coupled decay, both bias corrections, eps after the square root), per-parameter step
    counts (a parameter whose gradient is None is not updated and does not count).  lr, betas, eps, weight_decay and grad_scale are
    rounded to float32 first and then used as doubles: that is what the kernels are given.  Calls listed in `skip` (1-based) are not
    taken and do not advance the step count; count_skipped=True is the host-hyper form's documented behaviour under a skip flag
    (nothing is updated, the host counter advances).
    -> one snapshot per call: {"p", "m", "v": lists of float64 tensors, "step": list of int, "lr": the rate of that call}."""
    b1, b2 = f32(hyper["betas"][0]), f32(hyper["betas"][1])
    eps, wd, gs = f32(hyper["eps"]), f32(hyper["weight_decay"]), f32(hyper["grad_scale"])

    def update(p, g, m, v, step, lr):
        oracle.adam_step([p], [g * gs], [m], [v], step, lr=f32(lr), beta1=b1, beta2=b2, eps=eps, weight_decay=wd)

    return _run(params, grad_seq, hyper, tuple(skip), count_skipped, torch.float64, update)


def adam_fp32_restatement(params, grad_seq, hyper, skip=(), count_skipped=False, mutant=None):
    """The same rule with every tensor operation in float32 on the CPU (the bias corrections in double from the float32 betas, then
    rounded, as both kernel forms take them).  `mutant` names one mistake a kernel could make (MUTANTS)."""
    assert mutant is None or mutant in MUTANTS, mutant
    b1, b2 = f32(hyper["betas"][0]), f32(hyper["betas"][1])
    eps, wd, gs = f32(hyper["eps"]), f32(hyper["weight_decay"]), f32(hyper["grad_scale"])
    if mutant == "swap_betas":
        b1, b2 = b2, b1
    one_b1, one_b2 = f32(1.0 - b1), f32(1.0 - b2)         # exact in float32: the kernels' 1.f - beta

    def update(p, g, m, v, step, lr):
        lr = f32(lr)
        bc1 = 1.0 if mutant == "no_bc1" else f32(1.0 - b1 ** step)
        bc2_sqrt = 1.0 if mutant == "no_bc2" else f32(math.sqrt(1.0 - b2 ** step))
        if mutant == "decoupled_decay":
            g = g * gs
            p.mul_(f32(1.0 - lr * wd))
        else:
            g = g * gs + wd * p
        m_new = b1 * m + one_b1 * g
        v_new = b2 * v + one_b2 * g * g
        if mutant == "eps_inside_sqrt":
            denom = (v_new / f32(bc2_sqrt * bc2_sqrt) + eps).sqrt()
        else:
            denom = v_new.sqrt() / bc2_sqrt + eps
        p.sub_(f32(lr / bc1) * m_new / denom)
        if mutant != "moments_not_stored":
            m.copy_(m_new)
            v.copy_(v_new)

    return _run(params, grad_seq, hyper, tuple(skip), count_skipped, torch.float32, update)


def _flat(ts):
    return torch.cat([t.detach().reshape(-1) for t in ts]).cpu().double() if isinstance(ts, (list, tuple)) else ts.detach().reshape(-1).cpu().double()


def adam_errors(got_p, got_m, got_v, ref):
    """-> {"p": max |p - p_ref| / lr, "m", "v": the largest per-tensor max error / max |reference|}; `ref` is one snapshot, got_*
    are lists of tensors like the reference's or their concatenation."""
    sizes = [t.numel() for t in ref["p"]]
    seg = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    out = {}
    for key, got in (("p", got_p), ("m", got_m), ("v", got_v)):
        a, r = _flat(got), _flat(ref[key])
        assert a.shape == r.shape, (key, a.shape, r.shape)
        err = (a - r).abs()
        err[err != err] = float("inf")                   # NaN
        if key == "p":
            out[key] = float(err.max()) / ref["lr"]
            continue
        per_err = torch.zeros(len(sizes), dtype=torch.float64).scatter_reduce_(0, seg, err, "amax")
        per_ref = torch.zeros(len(sizes), dtype=torch.float64).scatter_reduce_(0, seg, r.abs(), "amax")
        empty = per_ref == 0                             # nothing may appear where the reference has nothing
        ratio = torch.where(empty, torch.where(per_err == 0, 0.0, float("inf")), per_err / torch.where(empty, 1.0, per_ref))
        out[key] = float(ratio.max())
    return out


def check_adam(got_p, got_m, got_v, ref, lim=None, what=""):
    """The one comparison of every GPU test: prints the figures, then asserts them against `lim` (default LIMITS)."""
    lim = LIMITS if lim is None else lim
    e = adam_errors(got_p, got_m, got_v, ref)
    print(f"adam {what}: p {e['p']:.3e} lr (limit {lim['p']:.2e})  m {e['m']:.3e} ({lim['m']:.2e})  v {e['v']:.3e} ({lim['v']:.2e})")
    bad = [k for k in ("p", "m", "v") if not e[k] <= lim[k]]
    assert not bad, f"{what}: " + ", ".join(f"{k} {e[k]:.3e} > {lim[k]:.2e}" for k in bad)
    return e


_CACHE = {}


def reference(name, count_skipped=False):
    """Float64 snapshots of a scenario, computed once and shared (do not modify)."""
    key = (name, count_skipped)
    if key not in _CACHE:
        sc = SCENARIOS[name]
        params, grad_seq = scenario_inputs(name)
        _CACHE[key] = adam_reference(params, grad_seq, sc["hyper"], sc["skip"], count_skipped)
    return _CACHE[key]


def restatement(name, count_skipped=False, mutant=None):
    sc = SCENARIOS[name]
    params, grad_seq = scenario_inputs(name)
    return adam_fp32_restatement(params, grad_seq, sc["hyper"], sc["skip"], count_skipped, mutant)


def measure():
    """Unmutated float32 restatement against the float64 reference: the largest figure over every scenario and every call."""
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for name, sc in SCENARIOS.items():
        for cs in ((False, True) if sc["skip"] else (False,)):
            for got, ref in zip(restatement(name, cs), reference(name, cs)):
                e = adam_errors(got["p"], got["m"], got["v"], ref)
                worst = {k: max(worst[k], e[k]) for k in worst}
    return worst
