"""tests/attention_ref.py on the CPU: the reference the GPU tests of csrc/attention.hip compare with is the oracle's arithmetic, and its
inputs (attention_ref.cases()) are such that a correct fp32 kernel must take the float64 reference's decisions.

  1. float64, composed with F.conv2d: tail() / gate() / channel_attention() / spatial_attention() equal oracle.robust_unet_ref's
     residual_block / attention_gate / channel_attention / spatial_attention on the same state to 1e-12, outputs and every gradient.
  2. every case: (a) arg-max margins >= 2e-5 of scale (twice the GPU tests' forward tolerance), (b) at most 0.02 % of the ReLU inputs
     within 2e-5 of scale of zero, (c) a quarter of each sigmoid's outputs in [0.1, 0.9], (d) 35-65 % of the ReLU inputs positive.
     A gate has no arg-max; its ReLU is the one over bn(g1) + bn(x1) and its sigmoid the one over psi.  The standalone attentions have
     no ReLU.  Planted ties are exact and left out of (a).
  3. the fp32 floor: the reference in float32 against float64, per tensor, printed (pytest -s) - the figure the GPU tests' tolerance rule
     refers to.  No kernel is involved.
"""
import importlib

import pytest
import torch

import attention_ref as R

CASES = R.cases()


def _oracle():
    return importlib.import_module("oracle.robust_unet_ref")


def _state(P, pre):
    return {f"{pre}.{k}": v.clone() for k, v in R.f64(P).items()}


def _grads(loss_of, leaves):
    for v in leaves:
        v.grad = None
    loss_of().backward()
    return [v.grad.clone() for v in leaves]


def _same(a, b, name):
    assert a.shape == b.shape, name
    err = float((a - b).abs().max())
    assert err <= 1e-12 * max(1.0, float(b.abs().max())), (name, err)


@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "tail" and c.shape[:3] in ((2, 8, 8), (3, 6, 10), (1, 2, 2))], ids=lambda c: c.id)
def test_tail_is_the_oracles_residual_block(case):
    O = _oracle()
    b = case.build()
    P = {k: (v.requires_grad_(True) if v.is_floating_point() and "running" not in k else v) for k, v in R.f64(b.P).items()}
    x = b.x.double().requires_grad_(True)
    dout = b.dout.double()
    leaves = [x] + [v for v in P.values() if v.requires_grad]

    def mine():
        t2, r = R.tail_inputs(x, P, case.training, b.mask)
        return (R.tail(t2, r, P, case.training).out * dout).sum()

    def theirs():
        st = {f"rb.{k}": (v.clone() if not v.requires_grad else v) for k, v in P.items()}
        return (O.residual_block(st, "rb", x, case.training, b.mask.double() if b.mask is not None else None) * dout).sum()
    with torch.no_grad():
        t2, r = R.tail_inputs(x, P, case.training, b.mask)
        _same(R.tail(t2, r, P, case.training).out,
              O.residual_block(_state(b.P, "rb"), "rb", x, case.training, b.mask.double() if b.mask is not None else None), "out")
    for k, a, c in zip(["x"] + [k for k, v in P.items() if v.requires_grad], _grads(mine, leaves), _grads(theirs, leaves)):
        _same(a, c, "grad " + k)


@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "gate" and c.shape[:3] in ((2, 8, 8), (3, 6, 10)) and c.switch is None],
                         ids=lambda c: c.id)
def test_gate_is_the_oracles_attention_gate(case):
    O = _oracle()
    b = case.build()
    c = case.shape[3]
    P = {k: (v.requires_grad_(True) if v.is_floating_point() and "running" not in k else v) for k, v in R.f64(b.P).items()}
    up, skip = b.up.double().requires_grad_(True), b.skip.double().requires_grad_(True)
    datt = b.dcat[:, :c].double()
    leaves = [up, skip] + [v for v in P.values() if v.requires_grad]

    def mine():
        g1, x1 = R.gate_inputs(up, skip, P)
        return (R.gate(g1, x1, skip, P, case.training).att * datt).sum()

    def theirs():
        st = {f"att.{k}": (v.clone() if not v.requires_grad else v) for k, v in P.items()}
        return (O.attention_gate(st, "att", up, skip, case.training) * datt).sum()
    with torch.no_grad():
        g1, x1 = R.gate_inputs(up, skip, P)
        _same(R.gate(g1, x1, skip, P, case.training).att, O.attention_gate(_state(b.P, "att"), "att", up, skip, case.training), "att")
    for k, a, c_ in zip(["up", "skip"] + [k for k, v in P.items() if v.requires_grad], _grads(mine, leaves), _grads(theirs, leaves)):
        _same(a, c_, "grad " + k)


@pytest.mark.parametrize("case", [c for c in CASES if c.kind in ("ca", "sa") and c.shape[1] <= 8], ids=lambda c: c.id)
def test_standalone_attentions_are_the_oracles(case):
    """ties included: the oracle's adaptive_max_pool2d / max(dim=1) and the reference's max(dim=...) send the gradient to the same element"""
    O = _oracle()
    b = case.build()
    if case.kind == "ca":
        (ref, g) = R.ca_run(b.x, b.P, b.dy)
        names = ("fc.0.weight", "fc.2.weight")
        fn = lambda st, x: O.channel_attention(st, "m", x)
    else:
        (ref, g) = R.sa_run(b.x, b.P, b.dy)
        names = ("conv1.weight",)
        fn = lambda st, x: O.spatial_attention(st, "m", x)
    st = {f"m.{k}": v.clone().requires_grad_(True) for k, v in R.f64(b.P).items()}
    x = b.x.double().requires_grad_(True)
    y = fn(st, x)
    (y * b.dy.double()).sum().backward()
    _same(ref.y.detach(), y.detach(), "y")
    _same(g["dx"], x.grad, "dx")
    for k in names:
        _same(g[k], st[f"m.{k}"].grad, k)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_input_conditions(case):
    fig = R.conditions(case)
    print(case.id, {k: (f"{v:.3g}" if isinstance(v, float) else v) for k, v in fig.items()})
    assert not R.conditions_hold(fig), R.conditions_hold(fig)
    b = case.build()
    for k, v in b.P.items():         # about 30 % negative gammas in every BatchNorm; from 16 channels on at least an eighth and at most 60 %
        if k.endswith(".weight") and v.dim() == 1:
            share = float((v < 0).float().mean())
            assert v.numel() < 16 or 0.125 <= share <= 0.6, (k, share)
            assert v.numel() < 2 or 0 < share < 1, (k, share)


def test_some_gate_has_a_negative_psi_gamma():
    signs = [float(c.build().P["psi.1.weight"]) < 0 for c in CASES if c.kind == "gate"]
    assert any(signs) and not all(signs)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_fp32_floor(case):
    """Prints the floor; asserts only that float32 stays a float32 (1e-4 of scale: a wrong formula in one dtype's path would not)."""
    floor = R.fp32_floor(case)
    print("fp32 floor", case.id, " ".join(f"{k}={v:.1e}" for k, v in floor.items()))
    assert all(v <= 1e-4 for v in floor.values()), floor
