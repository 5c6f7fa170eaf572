"""tests/x3_ref.py against itself and against torch, without a GPU: the restatement of the fixed split passes the checks that
tests/test_gpu_x3_edges.py applies to the kernels, the parent's split and three named mistakes are rejected by them, the table of
the representation error is where the file says it is, and torch's own fp32 ops class every edge output as the reference does."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import x3_ref as R      # noqa: E402

SIDES = ("a", "b")


def _run(es, **kw):
    return R.x3_matmul(es["a"], es["b"], **kw), R.x3_matmul(es["a_clean"], es["b_clean"], **kw)


def _tn_run(es, **kw):
    mm = lambda a, b: R.x3_matmul(a, b, **kw)      # noqa: E731
    return R.tn_split_ref(es["a"], es["b"], mm), R.tn_split_ref(es["a_clean"], es["b_clean"], mm)


@pytest.mark.parametrize("flush", [False, True])
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_fixed_restatement_keeps_the_contract_on_every_edge_set(kind, side, flush):
    es = R.gemm_edge_set(kind, side)
    got, clean = _run(es, variant="fixed", flush=flush)
    R.check_finite_contract(got, R.mm64(es["a"], es["b"]), es["touched"], clean, what=f"NN {kind} in {side}", rms_tol=R.RMS_TOL)
    es = R.tn_edge_set(kind, side)
    got, clean = _tn_run(es, variant="fixed", flush=flush)
    R.check_finite_contract(got, R.tn_split_ref(es["a"], es["b"]), es["touched"], clean, what=f"TN {kind} in {side}", rms_tol=R.RMS_TOL)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("kind", R.HUGE_KINDS)
def test_parent_split_fails_finite_stays_finite(kind, side):
    """h = bf16(x) without the clamp: every dot product that reads a finite |x| >= 0x7F7F8000 is NaN - six rows of 36 (A side) or six
    columns of 130 (B side) of batch 0; 0x7F7F7FFF still rounds to bf16-max and passes."""
    es = R.gemm_edge_set(kind, side)
    got, clean = _run(es, variant="parent")
    ref = R.mm64(es["a"], es["b"])
    assert bool(torch.isfinite(ref).all())
    bad = int((~torch.isfinite(got.float())).sum())
    if kind == "h_last":
        assert bad == 0
        R.check_finite_contract(got, ref, es["touched"], clean)
        return
    assert bad == (6 * 36 if side == "a" else 6 * 130), bad
    assert bool((~torch.isfinite(got.float()) == es["touched"]).all())
    with pytest.raises(AssertionError, match=f"C1, {bad} outputs non-finite"):
        R.check_finite_contract(got, ref, es["touched"], clean)


@pytest.mark.parametrize("kind", R.HUGE_KINDS)
def test_mixed_splits_fail_on_the_unprotected_side_only(kind):
    """a library whose packer clamps and whose kernel does not (or the reverse): C1 fails exactly where the overflowing element meets the
    unprotected split, whichever operand that is"""
    for side in SIDES:
        es = R.gemm_edge_set(kind, side)
        ref = R.mm64(es["a"], es["b"])
        for va, vb in (("parent", "fixed"), ("fixed", "parent")):
            got = R.x3_matmul(es["a"], es["b"], va, variant_b=vb)
            hit = kind != "h_last" and (va if side == "a" else vb) == "parent"
            assert bool((~torch.isfinite(got.float())).any()) == hit, (side, va, vb)
            if not hit:
                R.check_finite_contract(got, ref, es["touched"], R.x3_matmul(es["a_clean"], es["b_clean"], va, variant_b=vb), rms_tol=R.RMS_TOL)


def test_three_huge_elements_in_a_scaled_product():
    """the issue's count: three huge elements in A, B scaled by 2^-12 -> 3 rows x 36 columns non-finite in the parent, none fixed"""
    a, b = R.gaussian((130, 48), 1), R.gaussian((48, 36), 2) * R.PARTNER_SCALE
    for r, k, v in ((3, 0, R.FLT_MAX), (77, 20, -R.H_OVERFLOWS), (129, 47, R.H_OVERFLOWS)):
        a[r, k] = v
    ref = R.mm64(a, b)
    assert int((~torch.isfinite(R.x3_matmul(a, b, "parent").float())).sum()) == 108
    got = R.x3_matmul(a, b, "fixed")
    assert bool(torch.isfinite(got.float()).all())
    assert float((got - ref).abs().max() / ref.abs().max()) <= 5e-8


@pytest.mark.parametrize("side", SIDES)
def test_mistake_inf_to_finite_is_rejected(side):
    """h clamped AND the residual taken from the clamped x: Inf becomes 3.39e38 and the overflow never reaches the gradient"""
    for kind in ("pinf", "ninf", "pinf_ninf", "inf_x_one"):
        es = R.gemm_edge_set(kind, side)
        got, clean = _run(es, mistake="inf_to_finite")
        with pytest.raises(AssertionError, match="C2"):
            R.check_finite_contract(got, R.mm64(es["a"], es["b"]), es["touched"], clean)


@pytest.mark.parametrize("kind", ("nan", "flt_max"))
def test_mistake_poison_leaks_is_rejected(kind):
    es = R.gemm_edge_set(kind, "a")
    got, _ = _run(es, mistake="poison_leaks")                       # row 65 of both batches, which reads no edge element
    clean = R.x3_matmul(es["a_clean"], es["b_clean"])
    with pytest.raises(AssertionError, match="C3, 72 non-finite outputs outside"):
        R.check_finite_contract(got, R.mm64(es["a"], es["b"]), es["touched"], clean)


def test_mistake_drop_l_plane_is_rejected():
    """l = 0 leaves 16 of the 24 significant bits: 3.4e-6 rms and 3.5 - 4.0e-6 of scale at s = 1 - at the edge of the 4e-6 maximum-norm
    bound, seven times the rms bound that the k = 48 GEMM cases apply beside it"""
    a, b = R.gaussian((2, 130, 48), 5), R.gaussian((2, 48, 36), 6)
    got, ref = R.x3_matmul(a, b, mistake="drop_l_plane"), R.mm64(a, b)
    none = torch.zeros(2, 130, 36, dtype=torch.bool)
    with pytest.raises(AssertionError, match="C1, rms error 3.4"):
        R.check_finite_contract(got, ref, none, got, rms_tol=R.RMS_TOL)
    with pytest.raises(AssertionError, match="rms error 3.4"):
        R.check_tiny(got, ref, 1.0, rms_tol=R.RMS_TOL)
    R.check_tiny(R.x3_matmul(a, b), ref, 1.0, rms_tol=R.RMS_TOL)
    R.check_finite_contract(R.x3_matmul(a, b), ref, none, rms_tol=R.RMS_TOL)
    # the figure the rms limit rests on: torch's fp32 bmm against float64 on the same operands
    fp32 = R._rms_ratio(torch.bmm(a, b).double() - ref, ref)
    assert R.RMS_MEASURED / 2 <= fp32 <= R.RMS_MEASURED * 2, fp32


def test_measure_is_where_the_docstring_says():
    now = R.measure()
    for s, figs in R.MEASURED.items():
        for name, was, is_ in zip(("kept", "flushed"), figs, now[s]):
            assert was / 2 <= is_ <= was * 2, (s, name, was, is_)
            assert f"{was:.1e}" in R.__doc__, (s, name, was)
    assert R.tiny_limit(1e-20) == R.tiny_limit(1e-30) == R.BASE_TOL + 4 * R.MEASURED[1e-30][1]
    assert R.tiny_limit(1e-35) == R.BASE_TOL + 4 * R.MEASURED[1e-35][1] and R.tiny_limit(1e-37) == R.BASE_TOL + 4 * R.MEASURED[1e-37][1]
    assert all(R.tiny_limit(a) <= R.tiny_limit(b) for a, b in zip(R.TINY_SCALES, R.TINY_SCALES[1:]))


@pytest.mark.parametrize("flush", [False, True])
def test_fixed_restatement_is_within_the_tiny_limits(flush):
    a, b = R.gaussian((2, 130, 48), 31), R.gaussian((2, 48, 36), 32)
    for s in R.TINY_SCALES:
        a_s = (a * s).float()
        R.check_tiny(R.x3_matmul(a_s, b, flush=flush), R.mm64(a_s, b), s, rms_tol=R.RMS_TOL)
    a_d = a.clone()
    a_d.view(-1)[::100] = 1e-40                        # fp32 denormals among O(1) elements, as the GPU case plants them
    assert int(((a_d != 0) & (a_d.abs() < R.MIN_NORMAL)).sum()) == a_d.numel() // 100 + 1
    R.check_tiny(R.x3_matmul(a_d, b, flush=flush), R.mm64(a_d, b), None)
    a_d = torch.full((2, 130, 48), 1e-40) * torch.sign(a)      # nothing but denormals: the result is far below 1e-38, every plane denormal
    R.check_tiny(R.x3_matmul(a_d, b, flush=flush), R.mm64(a_d, b), None)


def _classes(t):
    t = t.float()
    return torch.isfinite(t).int() + 2 * torch.isposinf(t).int() + 4 * torch.isneginf(t).int() + 8 * torch.isnan(t).int()


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_torch_fp32_bmm_classes_every_output_as_the_reference_does(kind, side):
    """guards the reference's class rule (IEEE products, no BLAS) against a surprise in the CPU library behind torch.bmm"""
    es = R.gemm_edge_set(kind, side)
    assert torch.equal(_classes(torch.bmm(es["a"], es["b"])), _classes(R.mm64(es["a"], es["b"])))
    es = R.tn_edge_set(kind, side)
    assert torch.equal(_classes(torch.bmm(es["a"].transpose(1, 2), es["b"])), _classes(R.tn_split_ref(es["a"], es["b"]).sum(0)))


@pytest.mark.parametrize("kind", R.KINDS)
def test_torch_fp32_conv2d_classes_every_output_as_the_reference_does(kind):
    """the 3x3, dilated, 1x1 and transposed references against torch's fp32 convolutions on a poisoned activation, and the touched
    geometry of the Winograd tiles covers every non-finite output of the reference"""
    scale = R.PARTNER_SCALE if kind in R.HUGE_KINDS else 1.0
    for dil, (n, h, w, ci, co) in ((1, (2, 8, 8, 16, 32)), (2, (2, 16, 16, 16, 8))):
        x, wt = R.gaussian((n, h, w, ci), 40 + dil), R.gaussian((3, 3, ci, co), 50) * scale
        xe, _ = R.plant(x, kind, ((1, 3 * dil, 4 * dil, 5),), 3)
        got = F.conv2d(xe.permute(0, 3, 1, 2), wt.permute(3, 2, 0, 1), None, 1, dil, dil).permute(0, 2, 3, 1)
        ref = R.conv3_ref(xe, wt, dil)
        assert torch.equal(_classes(got), _classes(ref))
        for m in (2, 4):
            mask = R.wino_touched((n, h, w), m, dil, ((1, 3 * dil, 4 * dil),))
            assert not bool((~torch.isfinite(ref.float()) & ~mask[..., None]).any())
            assert int(mask.sum()) <= 4 * m * m
    x, w1, w2 = R.gaussian((1, 6, 10, 48), 60), R.gaussian((1, 1, 48, 36), 61) * scale, R.gaussian((2, 2, 48, 36), 62) * scale
    xe, _ = R.plant(x, kind, ((0, 5, 9, 47),), 3)
    got = F.conv2d(xe.permute(0, 3, 1, 2), w1.permute(3, 2, 0, 1)).permute(0, 2, 3, 1)
    assert torch.equal(_classes(got), _classes(R.mm64(xe.reshape(1, 60, 48), w1[0, 0][None]).reshape(1, 6, 10, 36)))
    got = F.conv_transpose2d(xe.permute(0, 3, 1, 2), w2.permute(2, 3, 0, 1), stride=2).permute(0, 2, 3, 1)
    assert torch.equal(_classes(got), _classes(R.convt_ref(xe, w2)))


def test_references_equal_torch_float64_on_gaussian_data():
    x, wt, dy = R.gaussian((2, 8, 8, 16), 1).double(), R.gaussian((3, 3, 16, 8), 2).double().requires_grad_(True), R.gaussian((2, 8, 8, 8), 3).double()
    for dil in (1, 2):
        xr = x.clone().requires_grad_(True)
        y = F.conv2d(xr.permute(0, 3, 1, 2), wt.permute(3, 2, 0, 1), None, 1, dil, dil).permute(0, 2, 3, 1)
        gx, gw = torch.autograd.grad(y, (xr, wt), dy)
        for got, ref in ((R.conv3_ref(x, wt.detach(), dil), y), (R.conv3_dgrad_ref(dy, wt.detach(), dil), gx), (R.conv3_wgrad_ref(x, dy, dil), gw)):
            assert float((got - ref.detach()).abs().max()) <= 1e-12
    w2 = R.gaussian((2, 2, 16, 8), 4).double().requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    y = F.conv_transpose2d(xr.permute(0, 3, 1, 2), w2.permute(2, 3, 0, 1), stride=2).permute(0, 2, 3, 1)
    dy2 = R.gaussian(tuple(y.shape), 5).double()
    gx, gw = torch.autograd.grad(y, (xr, w2), dy2)
    for got, ref in ((R.convt_ref(x, w2.detach()), y), (R.convt_dgrad_ref(dy2, w2.detach()), gx), (R.convt_wgrad_ref(x, dy2), gw)):
        assert float((got - ref.detach()).abs().max()) <= 1e-12
