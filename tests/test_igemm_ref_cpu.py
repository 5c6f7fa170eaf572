"""CPU: tests/igemm_ref.py is what tests/test_gpu_igemm_variants.py measures the implicit-GEMM and GEMM kernels with, so it is measured first.

  * every reference equals torch.nn.functional's float64 operation (autograd for the gradients) to 1e-12 at every shape of the GPU file;
  * SENSITIVITY of bound(nterms, magnitude) at every float32 shape of the GPU file, with bias and `+=` present (the largest bound): a result
    with one tap dropped, with the last channel chunk (the last 4 channels read; for a weight gradient the last 16 pixels, one k-step)
    dropped, computed from a source shifted by one pixel, or with one output row written one pixel off, violates the bound somewhere.  This
    is what keeps the bound meaningful; it fails when a shape is made so large that a dropped product hides inside the bound;
  * float32 on the CPU (torch's own kernels, and the reference's loops run in float32) stays inside the bound: a correct fp32
    implementation does not violate it.
"""
import pytest
import torch
import torch.nn.functional as F

import igemm_ref as R

OPS = R.igemm_cases() + R.general_cases()
ALL_OPS = OPS + R.lowp_cases() + R.lowp_c3_cases()
WG = R.wgrad_cases()
GEMMS = R.gemm_cases()


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def torch_op(c, x, w, bias, old):
    """the operation of an op case through torch.nn.functional, in the dtype of its arguments"""
    n, h, wd = c.n, c.h, c.w
    if c.kind in ("conv", "gconv"):
        y = nhwc(F.conv2d(nchw(x[..., :c.cin_w]), w.permute(3, 2, 0, 1), None, c.stride, c.pad, c.dil))
    elif c.kind in ("conv_dgrad", "gconv_dgrad"):
        z = torch.zeros(n, c.cout, h, wd, dtype=x.dtype, requires_grad=True)
        y = nhwc(torch.autograd.grad(F.conv2d(z, w.permute(3, 2, 0, 1), None, c.stride, c.pad, c.dil), z, nchw(x))[0])
    elif c.kind in ("convt2", "convt4"):
        y = nhwc(F.conv_transpose2d(nchw(x), w.permute(2, 3, 0, 1), None, 2, c.pad))
    else:
        z = torch.zeros(n, c.cout, h, wd, dtype=x.dtype, requires_grad=True)
        y = nhwc(torch.autograd.grad(F.conv_transpose2d(z, w.permute(2, 3, 0, 1), None, 2, c.pad), z, nchw(x))[0])
    if bias is not None:
        y = y + bias
    if old is not None:
        y = y + old
    return y


def torch_wgrad(c, x, dy):
    if c.tr:
        wz = torch.zeros(c.cin, c.cout, 2, 2, dtype=x.dtype, requires_grad=True)
        g, = torch.autograd.grad(F.conv_transpose2d(nchw(x), wz, None, 2), wz, nchw(dy))
        return g.permute(2, 3, 0, 1)
    wz = torch.zeros(c.cout, c.cin_w, c.k, c.k, dtype=x.dtype, requires_grad=True)
    g, = torch.autograd.grad(F.conv2d(nchw(x[..., :c.cin_w]), wz, None, 1, c.dil * (c.k // 2), c.dil), wz, nchw(dy))
    return g.permute(2, 3, 1, 0)


def relerr(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("c", ALL_OPS, ids=lambda c: c.id)
def test_op_references_are_torch_float64(c):
    p = R.op_problem(c)
    for bias, old in ((False, False), (True, True)):
        ref, mag = p.ref(bias, old)
        want = torch_op(c, p.x.double(), p.w.double(), p.bias.double() if bias else None, p.old.double() if old else None)
        assert ref.shape == want.shape == (c.n,) + p.dst_hw + (c.cout,)
        assert relerr(ref, want) <= 1e-12
        assert bool((mag >= ref.abs() * (1 - 1e-12)).all())
    wantm = torch_op(c, p.x.double().abs(), p.w.double().abs(), p.bias.double().abs(), p.old.double().abs())
    assert relerr(mag, wantm) <= 1e-12


@pytest.mark.parametrize("c", WG, ids=lambda c: c.id)
def test_wgrad_references_are_torch_float64(c):
    p = R.wgrad_problem(c)
    ref, mag = p.ref()
    assert relerr(ref, torch_wgrad(c, p.x.double(), p.dy.double())) <= 1e-12
    assert relerr(mag, torch_wgrad(c, p.x.double().abs(), p.dy.double().abs())) <= 1e-12


def test_gemm_references_are_torch_float64():
    for c in GEMMS:
        a, b = R.randn((c.batch, c.rows, c.k), 1).double(), R.randn((c.batch, c.k, c.n), 2).double()
        ref, mag = R.gemm(a, b)
        assert relerr(ref, torch.bmm(a, b)) <= 1e-12 and relerr(mag, torch.bmm(a.abs(), b.abs())) <= 1e-12
    for rows in R.TN_ROWS:
        a, b = R.randn((R.TN_BATCH, rows, 36), 3).double(), R.randn((R.TN_BATCH, rows, 68), 4).double()
        ref, mag = R.gemm_tn_split(a, b, R.TN_RPS)
        assert ref.shape == (3, R.TN_BATCH, 36, 68)
        assert relerr(ref.sum(0), torch.bmm(a.transpose(1, 2), b)) <= 1e-12
        assert relerr(ref[2], torch.bmm(a[:, 64:].transpose(1, 2), b[:, 64:])) <= 1e-12
        assert relerr(mag.sum(0), torch.bmm(a.abs().transpose(1, 2), b.abs())) <= 1e-12


def violates(got, ref, lim):
    return bool(((got - ref).abs() > lim).any())


def swap_rows(t, cols):
    """one row (pixel) of the result written one row off: rows r and r + 1 exchanged"""
    flat = t.reshape(-1, cols).clone()
    r = flat.shape[0] // 2
    flat[[r, r + 1]] = flat[[r + 1, r]]
    return flat.reshape(t.shape)


@pytest.mark.parametrize("c", OPS, ids=lambda c: c.id)
def test_bound_is_sensitive_at_every_forward_and_data_gradient_shape(c):
    p = R.op_problem(c)
    x, w, b, o = p.x.double(), p.w.double(), p.bias.double(), p.old.double()
    ref, mag = p.fn(x, w, b, o)
    lim = R.bound(p.nterms, mag)
    # the weight's contraction axis: rows (axis 2) of a forward weight, columns (axis 3) of the forward weight a data gradient reads
    kax = 2 if c.kind in ("conv", "gconv", "convt2", "convt4") else 3
    kw_ = w.shape[kax]
    for r in range(c.k):
        for s in range(c.k):
            w1 = w.clone()
            w1[r, s] = 0
            mid = c.k // 2
            if c.stride == 1 and c.k == 3 and ((r != mid and c.dil >= p.src_hw[0]) or (s != mid and c.dil >= p.src_hw[1])):
                assert not violates(p.fn(x, w1, b, o)[0], ref, lim)      # this tap never meets the image: nothing to drop
            else:
                assert violates(p.fn(x, w1, b, o)[0], ref, lim), f"tap ({r}, {s}) dropped"
    w2 = w.clone()
    w2.narrow(kax, 4 * ((kw_ - 1) // 4), kw_ - 4 * ((kw_ - 1) // 4)).zero_()
    assert violates(p.fn(x, w2, b, o)[0], ref, lim), "last channel chunk dropped"
    assert violates(p.fn(torch.roll(x, 1, 2), w, b, o)[0], ref, lim), "source shifted by one pixel"
    assert violates(swap_rows(ref, c.cout), ref, lim), "one output row written one pixel off"
    # float32 on the CPU stays inside
    got = torch_op(c, p.x, p.w, p.bias, p.old).double()
    assert not violates(got, ref, lim), float(((got - ref).abs() / lim).max())
    got = p.fn(p.x, p.w, p.bias, p.old)[0].double()
    assert not violates(got, ref, lim), float(((got - ref).abs() / lim).max())


@pytest.mark.parametrize("c", WG, ids=lambda c: c.id)
def test_bound_is_sensitive_at_every_weight_gradient_shape(c):
    p = R.wgrad_problem(c)
    x, dy = p.x.double(), p.dy.double()
    ref, mag = p.fn(x, dy)
    lim = R.bound(p.pixels + 64, mag)                 # 64: more slabs than any plan makes at these shapes
    for r in range(c.k):
        for s in range(c.k):
            got = ref.clone()
            got[r, s] = 0
            assert violates(got, ref, lim), f"tap ({r}, {s}) dropped"
    x2 = x.clone()
    x2.reshape(-1, c.cin)[-16:] = 0
    assert violates(p.fn(x2, dy)[0], ref, lim), "last 16 pixels dropped"
    assert violates(p.fn(torch.roll(x, 1, 2), dy)[0], ref, lim), "source shifted by one pixel"
    assert violates(swap_rows(ref, c.cout), ref, lim), "one output row written one row off"
    got = torch_wgrad(c, p.x, p.dy).double()
    assert not violates(got, ref, lim), float(((got - ref).abs() / lim).max())
    got = p.fn(p.x, p.dy)[0].double()
    assert not violates(got, ref, R.bound(p.pixels, mag)), float(((got - ref).abs() / lim).max())


def test_bound_is_sensitive_at_every_gemm_shape():
    for c in GEMMS:
        a32, b32 = R.randn((c.batch, c.rows, c.k), 1), R.randn((c.batch, c.k, c.n), 2)
        a, b = a32.double(), b32.double()
        ref, mag = R.gemm(a, b)
        lim = R.bound(R.ceil16(c.k), mag)
        b2 = b.clone()
        b2[:, -4:] = 0
        assert violates(R.gemm(a, b2)[0], ref, lim), "last channel chunk dropped"
        assert violates(R.gemm(torch.roll(a, 1, 1), b)[0], ref, lim), "source shifted by one row"
        assert violates(swap_rows(ref, c.n), ref, lim), "one output row written one row off"
        assert not violates(torch.bmm(a32, b32).double(), ref, lim)
    for rows in R.TN_ROWS:
        for k in R.TN_KN:
            for n in R.TN_KN:
                a32, b32 = R.randn((R.TN_BATCH, rows, k), 3), R.randn((R.TN_BATCH, rows, n), 4)
                a, b = a32.double(), b32.double()
                ref, mag = R.gemm_tn_split(a, b, R.TN_RPS)
                lim = R.bound(R.TN_RPS, mag)
                a2 = a.clone()
                a2[:, -4:] = 0
                assert violates(R.gemm_tn_split(a2, b, R.TN_RPS)[0], ref, lim), "last rows dropped"
                assert violates(R.gemm_tn_split(torch.roll(a, 1, 1), b, R.TN_RPS)[0], ref, lim), "source shifted by one row"
                assert violates(swap_rows(ref, n), ref, lim), "one output row written one row off"
                assert not violates(R.gemm_tn_split(a32, b32, R.TN_RPS)[0].double(), ref, lim)


def test_gamma():
    assert R.gamma(1) == pytest.approx(2.0 ** -24, rel=1e-6)
    assert R.bound(290, torch.tensor(2.0)).item() == pytest.approx(2 * 290 * R.U / (1 - 290 * R.U))
    assert R.ceil16(20) == 32 and R.ceil16(16) == 16 and R.ceil16(4) == 16
