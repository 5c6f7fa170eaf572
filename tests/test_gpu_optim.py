"""GPU: the optimizer, loss and overflow-flag kernels past the first step, against float64 on the CPU.

Adam (runet_adam_multi / runet_adam_multi_dev through FusedAdam): 12 steps of gradients the test supplies, compared with
tests/optim_ref.py's float64 reference by its `check_adam` at limits that were measured CPU against CPU (see that file; nothing
here is derived from what a kernel gave).  Parameters and gradients are views into flat buffers, so that one copy per step feeds
every gradient at a fixed address and so that the space between the tensors can be checked for stray writes.
BCE (runet_bce_fwd / runet_bce_bwd): float64 F.binary_cross_entropy on the CPU, including the saturated probabilities.
runet_nonfinite_flag: every length class of its vector loop and tail, Inf / NaN at each edge, +-FLT_MAX and denormals as clean values.
"""
import copy
import importlib
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_ref as R

pytestmark = pytest.mark.gpu

PKG = "eusipco-2026-robust-unet_amd"
DEV = "cuda:0"
GAP = 7.0          # fills the flat parameter buffer between the tensors


def _mod(name):
    return importlib.import_module(PKG + "." + name)


# ------------------------------------------------------------------------------------------------------------------------- Adam
def _offsets(misaligned):
    """Start of every tensor of R.SIZES in a flat buffer: multiples of 4 floats (16 bytes), or 1, 2, 3 floats past one."""
    offs, cur = [], 0
    for i, n in enumerate(R.SIZES):
        start = (cur + 3) // 4 * 4 + ((1 + i % 3) if misaligned else 0)
        offs.append(start)
        cur = start + n
    return offs, cur + 4


def _scatter(tensors, offs, total, fill=0.0):
    flat = torch.full((total,), fill, dtype=torch.float32)
    for t, o in zip(tensors, offs):
        if t is not None:
            flat[o:o + t.numel()] = t
    return flat


class Rig:
    """One FusedAdam over R.SIZES in a given memory layout, fed from the CPU and read back as lists of CPU tensors."""

    def __init__(self, params, layout, capturable, hp):
        assert layout in ("aligned", "param_views", "grad_views")
        optim = _mod("optim")
        self.p_off, p_total = _offsets(layout == "param_views")
        self.g_off, self.g_total = _offsets(layout == "grad_views")
        self.flat_p = _scatter(params, self.p_off, p_total, GAP).to(DEV)
        self.flat_g = torch.zeros(self.g_total, device=DEV)
        self.params = [torch.nn.Parameter(self.flat_p[o:o + n]) for o, n in zip(self.p_off, R.SIZES)]
        self.grad_views = [self.flat_g[o:o + n] for o, n in zip(self.g_off, R.SIZES)]
        assert all((p.data_ptr() % 16 == 0) == (layout != "param_views") for p in self.params)
        assert all((g.data_ptr() % 16 == 0) == (layout != "grad_views") for g in self.grad_views)
        self.gap = torch.ones(p_total, dtype=torch.bool)
        for o, n in zip(self.p_off, R.SIZES):
            self.gap[o:o + n] = False
        self.opt = optim.FusedAdam(self.params, lr=hp["lr"], betas=hp["betas"], eps=hp["eps"], weight_decay=hp["weight_decay"])
        self.opt.grad_scale = hp["grad_scale"]
        self.opt.capturable = capturable

    def feed(self, grads):
        """p.grad.copy_ for every parameter at once (fixed addresses); a None gradient leaves that parameter without one."""
        self.flat_g.copy_(_scatter(grads, self.g_off, self.g_total))
        for p, g, view in zip(self.params, grads, self.grad_views):
            p.grad = None if g is None else view

    def read(self):
        flat = self.flat_p.cpu()
        assert bool((flat[self.gap] == GAP).all()), "a write landed between the parameter tensors"
        p = [flat[o:o + n] for o, n in zip(self.p_off, R.SIZES)]
        m, v = [], []
        for q in self.params:
            st = self.opt.state.get(q, {})
            m.append(st["exp_avg"] if "exp_avg" in st else torch.zeros_like(q))
            v.append(st["exp_avg_sq"] if "exp_avg_sq" in st else torch.zeros_like(q))
        return p, list(torch.cat(m).cpu().split(R.SIZES)), list(torch.cat(v).cpu().split(R.SIZES))

    def host_steps(self):
        return [self.opt.state[q]["step"] if q in self.opt.state else 0 for q in self.params]

    def device_step(self):
        return int(self.opt._dev_state[0][1].item())

    def set_lr(self, lr):
        self.opt.param_groups[0]["lr"] = lr
        if self.opt.capturable:
            self.opt.sync_hyper()


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[0] + a[1] + a[2], b[0] + b[1] + b[2]))


@pytest.mark.parametrize("grad_scale", [1.0, 1.0 / 1024])
@pytest.mark.parametrize("weight_decay", [0.0, 1e-4])
@pytest.mark.parametrize("layout", ["aligned", "param_views", "grad_views"])
@pytest.mark.parametrize("capturable", [False, True], ids=["host_hyper", "device_hyper"])
def test_adam_twelve_steps_against_float64(capturable, layout, weight_decay, grad_scale):
    name = f"matrix-wd{weight_decay:g}-gs{grad_scale:g}"
    sc, ref = R.SCENARIOS[name], R.reference(name)
    params, grad_seq = R.scenario_inputs(name)
    rig = Rig(params, layout, capturable, sc["hyper"])      # grad_scale 1/1024: the scenario's gradients are multiplied by 1024
    for call, grads in enumerate(grad_seq, start=1):
        lr = R._lr_at(sc["hyper"], call)
        if lr != rig.opt.param_groups[0]["lr"]:
            rig.set_lr(lr)
        rig.feed(grads)
        rig.opt.step()
        if call in R.CHECK_STEPS:
            R.check_adam(*rig.read(), ref[call - 1], what=f"{name} {layout} step {call}")
            assert rig.host_steps() == ref[call - 1]["step"] == [call] * len(R.SIZES)
    if capturable:
        assert rig.device_step() == sc["steps"]


@pytest.mark.parametrize("layout", ["aligned", "grad_views"])
@pytest.mark.parametrize("capturable", [False, True], ids=["host_hyper", "device_hyper"])
def test_adam_skipped_step(capturable, layout):
    sc = R.SCENARIOS["skip"]
    # the device form does not count the skipped call (why TrainStep forces it under loss scaling); the host form's counter advances
    ref = R.reference("skip", count_skipped=not capturable)
    params, grad_seq = R.scenario_inputs("skip")
    rig = Rig(params, layout, capturable, sc["hyper"])
    flag = torch.zeros(2, dtype=torch.int32, device=DEV)
    rig.opt.skip_flag = flag
    for call, grads in enumerate(grad_seq, start=1):
        skipped = call in sc["skip"]
        flag[0] = 1 if skipped else 0
        before = rig.read() if skipped else None
        dev_before = rig.device_step() if skipped and capturable else None
        rig.feed(grads)
        rig.opt.step()
        after = rig.read()
        if skipped:
            assert _same(before, after), "a skipped step changed a parameter or a moment"
            if capturable:
                assert rig.device_step() == dev_before == call - 1
        R.check_adam(*after, ref[call - 1], what=f"skip {layout} step {call}")
        if not capturable:
            assert rig.host_steps() == ref[call - 1]["step"] == [call] * len(R.SIZES)
    if capturable:
        assert rig.device_step() == sc["steps"] - 1 == ref[-1]["step"][0]
    assert flag.tolist() == [0, 0]          # the optimizer reads the flag, it never writes it


def test_adam_late_gradient_host_form_counts_per_parameter():
    sc, ref = R.SCENARIOS["late"], R.reference("late")
    params, grad_seq = R.scenario_inputs("late")
    rig = Rig(params, "aligned", False, sc["hyper"])
    for call, grads in enumerate(grad_seq, start=1):
        rig.feed(grads)
        rig.opt.step()
        R.check_adam(*rig.read(), ref[call - 1], what=f"late step {call}")
        assert rig.host_steps() == ref[call - 1]["step"]
    assert rig.host_steps()[R.LATE] == sc["steps"] - 3 and rig.host_steps()[0] == sc["steps"]


def test_adam_late_gradient_device_form_raises():
    sc, ref = R.SCENARIOS["late"], R.reference("late")
    params, grad_seq = R.scenario_inputs("late")
    rig = Rig(params, "aligned", True, sc["hyper"])
    for call in (1, 2, 3):
        rig.feed(grad_seq[call - 1])
        rig.opt.step()
    R.check_adam(*rig.read(), ref[2], what="late (device form) step 3")
    before, steps = rig.read(), rig.host_steps()
    rig.feed(grad_seq[3])
    with pytest.raises(RuntimeError, match="step count"):      # one device counter cannot serve step 4 and step 1
        rig.opt.step()
    assert _same(before, rig.read()) and rig.device_step() == 3
    assert [s for i, s in enumerate(rig.host_steps()) if i != R.LATE] == [s for i, s in enumerate(steps) if i != R.LATE]


@pytest.mark.parametrize("same_object", [False, True], ids=["fresh_optimizer", "same_optimizer"])
def test_adam_resume_from_state_dict(same_object):
    sc, ref = R.SCENARIOS["resume"], R.reference("resume")
    params, grad_seq = R.scenario_inputs("resume")
    rig = Rig(params, "aligned", True, sc["hyper"])
    for call in (1, 2, 3):
        rig.feed(grad_seq[call - 1])
        rig.opt.step()
    saved = copy.deepcopy(rig.opt.state_dict())
    p3 = rig.read()[0]
    if same_object:
        for call in (4, 5):      # go on, then come back to the checkpoint: the device counter stands at 5
            rig.feed(grad_seq[call - 1])
            rig.opt.step()
        assert rig.device_step() == 5
        rig.flat_p.copy_(_scatter(p3, rig.p_off, rig.flat_p.numel(), GAP))
    else:
        rig = Rig(p3, "aligned", True, sc["hyper"])
    rig.opt.load_state_dict(saved)
    for call in (4, 5, 6):
        rig.feed(grad_seq[call - 1])
        rig.opt.step()
        R.check_adam(*rig.read(), ref[call - 1], what=f"resume ({'same' if same_object else 'fresh'} optimizer) step {call}")
        assert rig.host_steps() == [call] * len(R.SIZES)
    assert rig.device_step() == 6


# -------------------------------------------------------------------------------------------------------------------------- BCE
TINY = float(np.finfo(np.float32).tiny)            # smallest normal float
P_SPECIAL = (0.0, 1.0, TINY, 1.0 - 2.0 ** -24, 0.5)
Y_SPECIAL = (1.0, 0.0, 0.3)
BCE_SIZES = (1, 255, 2049, 1024 * 256 * 8 + 5)     # the last: past the forward's 1024-block cap and the backward's 4096 blocks
FLOOR = 1e-12                                      # ATen's (and the kernel's) floor of p (1 - p) in the backward
_BCE = {}


def _bce_case(n):
    """Probabilities, targets, float64 loss and float64 gradient for grad_out = 1 (computed once per size, not to be modified)."""
    if n not in _BCE:
        g = torch.Generator().manual_seed(100 + n % 97)
        prob = torch.rand(n, generator=g)          # multiples of 2^-24: no denormals
        tgt = torch.where(torch.rand(n, generator=g) < 0.5, (torch.rand(n, generator=g) < 0.5).float(), torch.rand(n, generator=g))
        special = [(p, y) for y in Y_SPECIAL for p in P_SPECIAL]      # (0, 1) first: the one element of n = 1
        k = min(n, len(special))
        prob[:k] = torch.tensor([p for p, _ in special[:k]])
        tgt[:k] = torch.tensor([y for _, y in special[:k]])
        if n >= 4 * len(special):                                    # and again at the very end (the grid-stride tail)
            prob[-k:] = prob[:k]
            tgt[-k:] = tgt[:k]
        pr = prob.double().requires_grad_(True)
        loss = F.binary_cross_entropy(pr, tgt.double())
        loss.backward()
        _BCE[n] = (prob, tgt, float(loss), pr.grad.detach())
    return _BCE[n]


@pytest.mark.parametrize("grad_out", [1.0, 1024.0, 1.0 / 3.0])
@pytest.mark.parametrize("n", BCE_SIZES)
@pytest.mark.parametrize("path", ["ops", "custom_op"])
def test_bce_against_float64(path, n, grad_out):
    prob, tgt, loss_ref, grad1 = _bce_case(n)
    gout = torch.tensor(grad_out, dtype=torch.float32)          # what the kernel reads; the reference uses the same rounded value
    grad_ref = grad1 * float(gout)
    pd = prob.to(DEV).requires_grad_(True)
    if path == "ops":
        loss = _mod("ops").bce_loss(pd, tgt.to(DEV))
    else:
        _mod("custom_ops")
        loss = torch.ops.runet.bce_loss(pd, tgt.to(DEV))
    loss.backward(gout.to(DEV))
    got_loss, got = float(loss), pd.grad.cpu().double()
    rel = abs(got_loss - loss_ref) / abs(loss_ref)
    # gradient: 4e-6 of each element's reference.  Where p (1 - p) is under the 1e-12 floor there is an absolute term as well, the
    # float32 format's and not the kernel's: an intermediate of the size grad_out (p - y) / n may fall below the smallest normal
    # 2^-126 there (p = that number, y = 0, a gradient of 1e-26 / n); what becomes of it is no part of the contract, and divided by
    # the floor it is 1.2e-26.
    p64, y64 = prob.double(), tgt.double()
    floored = p64 * (1 - p64) < FLOOR
    lim = 4e-6 * grad_ref.abs() + floored * (2.0 ** -126 / FLOOR)
    err = (got - grad_ref).abs()
    worst = int(torch.argmax(err - lim))
    ratio = err / grad_ref.abs().clamp_min(1e-300)
    print(f"bce {path} n={n} grad_out={grad_out:g}: loss {got_loss:.9g} ref {loss_ref:.9g} rel {rel:.2e}; grad max err/|ref| "
          f"{float(ratio[~floored].max()) if not bool(floored.all()) else 0.0:.2e} above the floor, {float(ratio[floored].max()):.2e} under it "
          f"(nearest the limit at {worst}: p {float(prob[worst])!r} y {float(tgt[worst])!r})")
    assert rel <= 2e-6
    assert bool((err <= lim).all()), (worst, float(got[worst]), float(grad_ref[worst]))
    # saturated probabilities in closed form
    sat = (p64 == 0) | (p64 == 1)
    assert bool((got[sat & (p64 == y64)] == 0).all())                           # exactly 0, not 0 / 0
    want = float(gout) * (p64 - y64) / (n * FLOOR)                              # +-grad_out / (n 1e-12) for the opposite hard target
    assert bool(((got - want).abs()[sat] <= 4e-6 * want.abs()[sat]).all())
    assert int((sat & ((p64 - y64).abs() == 1)).sum()) >= 1 and (n == 1 or int((sat & (p64 == y64)).sum()) >= 2)


# ------------------------------------------------------------------------------------------------------------- overflow flag
FLT_MAX = float(np.finfo(np.float32).max)
FLAG_SIZES = (1, 2, 3, 4, 5, 7, 4099, 2 * 4096 * 256 * 4 + 3)      # the last: two trips of the 4096-block grid-stride loop and a 3-element tail


@pytest.mark.parametrize("n", FLAG_SIZES)
def test_nonfinite_flag(n):
    lib, ops = _mod("_lib"), _mod("ops")
    g = torch.Generator().manual_seed(n % 1000)
    host = torch.randn(n + 4, generator=g)
    nvec = n // 4 * 4
    probes = sorted({0, max(nvec - 1, 0)} | set(range(nvec, n)))       # first element, last vectorised element, every tail element
    for i, pos in enumerate(probes):
        host[pos] = FLT_MAX if i % 2 == 0 else -FLT_MAX              # the largest finite values are clean
    if n > 16:
        host[8:12] = torch.tensor([1e-40, -1e-45, FLT_MAX, -FLT_MAX])      # denormals too
    host[n:] = float("nan")                                           # just past the end: must not be read
    store = host.to(DEV)
    buf = store[:n]
    flag = torch.zeros(2, dtype=torch.int32, device=DEV)
    assert buf.data_ptr() % 16 == 0

    def run():
        lib.check(lib.lib.runet_nonfinite_flag(buf.data_ptr(), n, flag.data_ptr(), ops.stream()))
        return flag.tolist()          # synchronizes: nothing above is freed before the kernels are done

    assert run() == [0, 0], "a finite buffer (+-FLT_MAX, denormals) was flagged"
    hits = 0
    for bad in (float("nan"), float("inf"), float("-inf")):
        for pos in probes:
            keep = float(host[pos])
            buf[pos] = bad
            hits += 1
            assert run() == [1, hits], (bad, pos)
            buf[pos] = keep
            assert run() == [0, hits], "a clean call resets flag[0] and leaves the count of flagged calls alone"
