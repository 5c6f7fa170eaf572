"""tests/optim_ref.py on the CPU: the float64 reference IS torch.optim.Adam, the limits in its docstring are what this machine
measures, and every named mistake is rejected at those limits while the unmutated float32 restatement is accepted - the proof that
tests/test_gpu_optim.py would notice these mistakes in a kernel."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_ref as R

MUTANT_SCENARIO = "matrix-wd0.0001-gs1"       # a decay of 0 would make `decoupled_decay` no mistake at all


@pytest.mark.parametrize("name", ["matrix-wd0.0001-gs1", "matrix-wd0-gs0.000976562", "skip", "late"])
def test_reference_is_torch_adam_in_float64(name):
    sc = R.SCENARIOS[name]
    hp = sc["hyper"]
    params, grad_seq = R.scenario_inputs(name)
    ref = R.reference(name)
    ps = [torch.nn.Parameter(p.double()) for p in params]
    opt = torch.optim.Adam(ps, lr=R.f32(hp["lr"]), betas=tuple(R.f32(b) for b in hp["betas"]), eps=R.f32(hp["eps"]),
                           weight_decay=R.f32(hp["weight_decay"]))
    gs = R.f32(hp["grad_scale"])
    taken = 0
    for call, grads in enumerate(grad_seq, start=1):
        opt.param_groups[0]["lr"] = R.f32(R._lr_at(hp, call))
        if call not in sc["skip"]:
            for p, g in zip(ps, grads):
                p.grad = None if g is None else g.double() * gs
            opt.step()
            taken += 1
        snap = ref[call - 1]
        for i, p in enumerate(ps):
            if p not in opt.state or "exp_avg" not in opt.state[p]:      # no gradient yet: untouched, no state
                assert snap["step"][i] == 0 and torch.equal(snap["p"][i], params[i].double())
                continue
            st = opt.state[p]
            assert int(st["step"]) == snap["step"][i]
            for got, want in ((p.detach(), snap["p"][i]), (st["exp_avg"], snap["m"][i]), (st["exp_avg_sq"], snap["v"][i])):
                err = float((got - want).abs().max())
                assert err <= 1e-12 * max(float(want.abs().max()), 1e-300), (name, call, i, err)
    assert ref[-1]["step"][0] == taken
    if sc["late"] is not None:
        assert ref[-1]["step"][sc["late"]] == taken - 3


def test_host_form_counts_a_skipped_call():
    a, b = R.reference("skip"), R.reference("skip", count_skipped=True)
    assert a[-1]["step"][0] == 7 and b[-1]["step"][0] == 8
    for k in (2, 3):      # calls 3 and 4: the skipped call changes nothing but the count
        assert all(torch.equal(x, y) for x, y in zip(a[k]["m"] + a[k]["v"] + a[k]["p"], b[k]["m"] + b[k]["v"] + b[k]["p"]))
    assert all(torch.equal(x, y) for x, y in zip(a[2]["p"] + a[2]["m"], a[3]["p"] + a[3]["m"]))
    assert not torch.equal(torch.cat(a[-1]["p"]), torch.cat(b[-1]["p"]))


def test_limits_are_the_measured_ones():
    got = R.measure()
    print("restatement against reference:", {k: f"{x:.3e}" for k, x in got.items()})
    for k, x in got.items():
        # the same arithmetic on another host may round a few elements the other way, no more
        assert R.MEASURED[k] / 2 <= x <= R.MEASURED[k] * 2, (k, x, R.MEASURED[k])
        assert R.LIMITS[k] == 4 * R.MEASURED[k]
    assert R.LIMITS["p"] <= 0.05 and 4 * got["p"] <= 0.05


def test_unmutated_restatement_is_accepted():
    for name in R.SCENARIOS:
        for step, (got, ref) in enumerate(zip(R.restatement(name), R.reference(name)), start=1):
            R.check_adam(got["p"], got["m"], got["v"], ref, what=f"{name} step {step}")


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutant_is_rejected(mutant):
    got, ref = R.restatement(MUTANT_SCENARIO, mutant=mutant), R.reference(MUTANT_SCENARIO)
    rejected = []
    for step in R.CHECK_STEPS:
        try:
            R.check_adam(got[step - 1]["p"], got[step - 1]["m"], got[step - 1]["v"], ref[step - 1], what=f"{mutant} step {step}")
        except AssertionError:
            rejected.append(step)
    # step 1 alone cannot tell the betas apart or see that the moments were dropped in p; from step 2 on every mistake shows
    assert set(rejected) >= {2, 6, 7, 12}, (mutant, rejected)


def test_check_adam_rejects_nan_and_values_where_the_reference_is_zero():
    ref = R.reference("resume")[0]
    p, m, v = ([t.clone() for t in ref[k]] for k in ("p", "m", "v"))
    R.check_adam(p, m, v, ref)
    bad = [t.clone() for t in p]
    bad[4][1] = float("nan")                    # 0 / 0: the element with p = 0 and g = 0
    with pytest.raises(AssertionError):
        R.check_adam(bad, m, v, ref)
    zero_ref = dict(ref, m=[torch.zeros_like(t) for t in ref["m"]])
    zm = [torch.zeros_like(t) for t in m]
    R.check_adam(p, zm, v, zero_ref)
    zm[0][0] = 1e-30
    with pytest.raises(AssertionError):
        R.check_adam(p, zm, v, zero_ref)
