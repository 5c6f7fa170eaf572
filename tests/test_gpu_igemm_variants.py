"""GPU: every tile variant, loader and route of csrc/conv_igemm.hip and csrc/gemm.hip against tests/igemm_ref.py in float64.

Both files choose their kernel by problem size and the rest of the suite uses small problems, so the large-problem instantiations are forced
here (runet_igemm_force_variant, runet_igemm_lowp_force_variant, RUNET_C3_PH) at shapes that are ragged against every
tile: P = 297 pixels, cin = 20 (K pads to 32), cout = 36 / 68 / 132 / 8 / 4.  tests/test_igemm_ref_cpu.py shows on the CPU that the references
are torch's float64 operations and that the bound used here notices a dropped tap, channel chunk, a shifted source or a misplaced row at
each of these shapes.

Criterion (float32 kernels): |got - ref64| <= gamma(nterms) * magnitude elementwise, igemm_ref.bound - derived, not tuned.  nterms = taps x
ceil16(K) + 2 for forward / data gradient, pixels + slabs for a weight gradient, the rows of a split for a split-K slab.  The 16-bit kernels
are held to the criterion of tests/test_gpu_bf16.py: 2e-4 of the output's scale against the float64 convolution of the rounded operands.

Every source is a channel slice of a wider buffer whose other channels are NaN (a read outside the slice that reaches a product shows),
every destination a slice whose neighbours must keep their bits; every case runs with and without bias, overwriting NaN and adding onto
random old content.

Each test keeps its worst err / bound; the module prints them at the end (pytest -s), DESIGN.md section 4 records one run.
"""
import importlib
import os
import subprocess
import sys

import pytest
import torch

import igemm_ref as R
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAN = float("nan")
TILES = ("<128, 32, 32, 32,", "<256, 64, 64, 64,", "<128, 64, 64, 32,", "<128, 128, 64, 64,", "<64, 64, 32, 32,")
TILE_BM = (128, 256, 128, 128, 64)
WORST = {}
_PROBLEMS = {}


def L():
    m = importlib.import_module(f"{PKG_NAME}._lib")
    return m.lib, m.check


def st():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture
def force():
    """force(variant) / force(variant, lowp=True): both hooks are back at -1 (automatic) when the test ends, however it ends"""
    lib, check = L()

    def f(variant, lowp=False):
        check((lib.runet_igemm_lowp_force_variant if lowp else lib.runet_igemm_force_variant)(variant))
    try:
        yield f
    finally:
        lib.runet_igemm_force_variant(-1)
        lib.runet_igemm_lowp_force_variant(-1)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for k in sorted(WORST):
        print(f"\nigemm-variants worst {k}: {WORST[k]:.4g}", end="")
    print()


@pytest.fixture(autouse=True)
def stop_at_a_device_error():
    """a failed launch or a device fault ends the session: nothing more is started on a device that reported an error"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error after a test of {__name__}: {e}", returncode=3)


def note(entry, value):
    WORST[entry] = max(WORST.get(entry, 0.0), float(value))


def within(entry, got, ref, lim, what):
    """|got - ref| <= lim elementwise (a NaN fails); keeps the worst err / bound of the entry point"""
    err = (got.double() - ref).abs()
    ratio = err / lim
    worst = float(ratio.nan_to_num(nan=float("inf")).max())
    note(entry + " err/bound", worst)
    assert bool((err <= lim).all()), f"{entry} {what}: worst err / bound {worst:.3g}, NaN {int(torch.isnan(got).sum())}"


def guard(shape, seed):
    return R.randn(shape, 9000 + seed).to(DEV)


def src_slice(t, ld=None, off=4):
    """t [..., c] as the channel slice [off, off + c) of a buffer [..., ld] of NaN -> (buffer, pointer of the slice, ld)"""
    c = t.shape[-1]
    ld = c + 8 if ld is None else ld
    buf = torch.full(tuple(t.shape[:-1]) + (ld,), NAN, device=DEV)
    buf[..., off:off + c] = t.to(DEV)
    return buf, buf.data_ptr() + 4 * off, ld


class Dst:
    """destination slice [off, off + c) of a buffer [..., ld] of random guard values; the slice starts as `old` or as NaN"""

    def __init__(self, shape, c, old=None, ld=None, off=4):
        self.c, self.off = c, off
        self.ld = c + 8 if ld is None else ld
        self.buf = guard(tuple(shape) + (self.ld,), c + len(shape))
        self.buf[..., off:off + c] = old.to(DEV) if old is not None else NAN
        self.snap = self.buf.clone()
        self.ptr = self.buf.data_ptr() + 4 * off

    def result(self):
        b, s, o, c = self.buf, self.snap, self.off, self.c
        assert torch.equal(b[..., :o], s[..., :o]) and torch.equal(b[..., o + c:], s[..., o + c:]), "the channels beside the destination slice changed"
        return b[..., o:o + c].clone()


def strided3(t, ld, off, stride, fill=NAN):
    """t [batch, rows, cols] laid out with row stride ld and batch stride `stride` in a flat buffer, first element at `off`"""
    batch, rows, cols = t.shape
    flat = torch.full((off + batch * stride + ld,), fill, device=DEV)
    view = torch.as_strided(flat, (batch, rows, cols), (stride, ld, 1), off)
    view.copy_(t.to(DEV))
    return flat, view, flat.data_ptr() + 4 * off


def problem(c):
    """the case's inputs and its four float64 references (bias x accumulate), computed once"""
    if c.id not in _PROBLEMS:
        p = R.op_problem(c)
        p.refs = {}
        for bias in (False, True):
            for acc in (0, 1):
                ref, mag = p.ref(bias, bool(acc))
                p.refs[bias, acc] = (ref.to(DEV), R.bound(p.nterms, mag).to(DEV))
        p.w_dev, p.bias_dev = p.w.to(DEV), p.bias.to(DEV)
        _PROBLEMS[c.id] = p
    return _PROBLEMS[c.id]


MODE = {"conv": R.FWD, "conv_dgrad": R.DGRAD, "convt2": R.CONVT_FWD, "convt2_dgrad": R.CONVT_DGRAD, "gconv": R.FWD, "gconv_dgrad": R.DGRAD,
        "convt4": R.CONVT_FWD, "convt4_dgrad": R.CONVT_DGRAD}
ENTRY = {"conv": "runet_conv_igemm", "conv_dgrad": "runet_conv_igemm", "convt2": "runet_conv_igemm", "convt2_dgrad": "runet_conv_igemm",
         "gconv": "runet_conv2d_general", "gconv_dgrad": "runet_conv2d_general", "convt4": "runet_convt4_igemm", "convt4_dgrad": "runet_convt4_igemm"}


def call_op(c, p, bias, acc, mode=None, w=None, stats=None):
    """one launch of the case through the C ABI -> the destination slice (the guard channels are checked on the way)"""
    lib, check = L()
    mode = MODE[c.kind] if mode is None else mode
    w = p.w_dev if w is None else w
    # the k2-s2 transposed forward writes the right half of a concat buffer, its data gradient reads one
    xbuf, xptr, ldx = src_slice(p.x, 2 * c.cin, c.cin) if c.kind == "convt2_dgrad" else src_slice(p.x)
    d = Dst((c.n,) + p.dst_hw, c.cout, p.old if acc else None, *((2 * c.cout, c.cout) if c.kind == "convt2" else ()))
    bptr = p.bias_dev.data_ptr() if bias else None
    if stats is not None:
        check(lib.runet_convt4_igemm_stats(xptr, ldx, w.data_ptr(), bptr, d.ptr, d.ld, c.n, c.h, c.w, c.cin, c.cout, stats.data_ptr(), st()))
    elif ENTRY[c.kind] == "runet_conv_igemm":
        check(lib.runet_conv_igemm(xptr, ldx, w.data_ptr(), bptr, d.ptr, d.ld, c.n, c.h, c.w, c.cin, c.cin_w, c.cout, c.k, c.k, c.dil, mode, acc, st()))
    elif ENTRY[c.kind] == "runet_conv2d_general":
        check(lib.runet_conv2d_general(xptr, ldx, w.data_ptr(), bptr, d.ptr, d.ld, c.n, c.h, c.w, c.cin, c.cin_w, c.cout, c.k, c.k, c.stride, c.pad,
                                       c.dil, mode, acc, st()))
    else:
        check(lib.runet_convt4_igemm(xptr, ldx, w.data_ptr(), bptr, d.ptr, d.ld, c.n, c.h, c.w, c.cin, c.cout, mode, acc, st()))
    return d.result()


def transposed_taps(c, p):
    """runet_transpose_taps of the forward weight [taps][cout][cin] (this call's naming) -> [taps][cin][cout] for the _T modes"""
    lib, check = L()
    wt = torch.empty(c.k * c.k, c.cin, c.cout, device=DEV)
    check(lib.runet_transpose_taps(p.w_dev.data_ptr(), wt.data_ptr(), c.k * c.k, c.cout, c.cin, st()))
    assert torch.equal(wt, p.w_dev.reshape(c.k * c.k, c.cout, c.cin).transpose(1, 2))
    return wt


def run_forced(c, variant, force):
    lib, _ = L()
    p = problem(c)
    force(variant)
    if ENTRY[c.kind] == "runet_conv_igemm":
        name = lib.runet_conv_igemm_kernel_name(c.n, c.h, c.w, c.cin, c.cout, c.k, MODE[c.kind]).decode()
        assert TILES[variant] in name, name
        kcontig = "true" if c.kind.endswith("dgrad") else "false"          # k-contiguous weights: the data gradients on the forward weight
        simple = "true" if c.k in (1, 2) and c.cin % 16 == 0 else "false"      # the loader without predicates: 1 x 1 and k2-s2, whole k-steps
        assert name.endswith(f", {kcontig}, {simple}>"), name
        print(f"\n{c.id} variant {variant}: {name}", end="")
    wt = transposed_taps(c, p) if c.kind in ("conv_dgrad", "convt2_dgrad") else None
    for bias in (False, True):
        for acc in (0, 1):
            got = call_op(c, p, bias, acc)
            within(ENTRY[c.kind], got, *p.refs[bias, acc], f"{c.id} variant {variant} bias {bias} accumulate {acc}")
            if wt is not None:
                got_t = call_op(c, p, bias, acc, mode=R.DGRAD_T if c.kind == "conv_dgrad" else R.CONVT_DGRAD_T, w=wt)
                assert torch.equal(got_t, got), "pre-transposed weights: not the bits of the untransposed mode under the same variant"


# ------------------------------------------------------------------------------------------------ a. runet_conv_igemm
@pytest.mark.parametrize("variant", range(5))
@pytest.mark.parametrize("c", R.igemm_cases(), ids=lambda c: c.id)
def test_conv_igemm_every_tile_variant_against_float64(c, variant, force):
    run_forced(c, variant, force)


INVARIANT = [c for c in R.igemm_cases() if (c.kind, c.cin, c.cout, c.k) in (("conv", 20, 36, 3), ("conv_dgrad", 20, 36, 3), ("conv", 48, 132, 1),
                                                                            ("conv_dgrad", 48, 132, 1), ("convt2", 32, 36, 2), ("convt2_dgrad", 20, 36, 2))]


@pytest.mark.parametrize("c", INVARIANT, ids=lambda c: c.id)
def test_conv_igemm_tile_variants_agree_bitwise(c, force):
    """an output element sees the same sequence of v_mfma_f32_32x32x2_f32 steps whatever the tile shape (k order: channel chunk, tap, 16
    channels in steps of two), so the five variants give the same bits - in every mode, the pre-transposed ones included"""
    p = problem(c)
    assert len(INVARIANT) == 6
    modes = {"conv": (R.FWD,), "conv_dgrad": (R.DGRAD, R.DGRAD_T), "convt2": (R.CONVT_FWD,), "convt2_dgrad": (R.CONVT_DGRAD, R.CONVT_DGRAD_T)}[c.kind]
    wt = transposed_taps(c, p) if len(modes) == 2 else None
    for mode in modes:
        outs = []
        for variant in range(5):
            force(variant)
            outs.append(call_op(c, p, True, 1, mode=mode, w=wt if mode in (R.DGRAD_T, R.CONVT_DGRAD_T) else None))
        for variant in range(1, 5):
            assert torch.equal(outs[variant], outs[0]), f"mode {mode}: variant {variant} differs from variant 0 by {float((outs[variant] - outs[0]).abs().max()):.3g}"


# ------------------------------------------------------------------------------------------------ b. the other geometries
@pytest.mark.parametrize("variant", range(5))
@pytest.mark.parametrize("c", R.general_cases(), ids=lambda c: c.id)
def test_general_and_k4_transposed_convolutions_every_tile_variant(c, variant, force):
    run_forced(c, variant, force)


@pytest.mark.parametrize("variant", range(5))
@pytest.mark.parametrize("c", [c for c in R.general_cases() if c.kind == "convt4"], ids=lambda c: c.id)
def test_k4_transposed_statistics_epilogue_every_tile_variant(c, variant, force):
    """runet_convt4_igemm_stats under a forced variant: y has the plain call's bits, the parts are the ones runet_convt4_igemm_stats_parts
    counts (one per tile and parity class), the counts add up to the pixels, and the finalized statistics equal the separate pass to 2e-6"""
    lib, _ = L()
    blocks = importlib.import_module(f"{PKG_NAME}.blocks")
    p = problem(c)
    force(variant)
    parts = lib.runet_convt4_igemm_stats_parts(c.n, c.h, c.w, c.cout)
    assert parts == 4 * -(-c.n * c.h * c.w // TILE_BM[variant])
    sent = -7777.25
    stats = torch.full((parts + 1, c.cout, 3), sent, device=DEV)
    y0 = call_op(c, p, True, 0)
    y1 = call_op(c, p, True, 0, stats=stats)
    assert torch.equal(y1, y0)
    assert bool((stats[:parts] != sent).all()) and bool((stats[parts] == sent).all())
    assert torch.equal(stats[:parts, :, 0].double().sum(0), torch.full((c.cout,), float(c.n * 4 * c.h * c.w), device=DEV, dtype=torch.float64))

    def bn_state():
        return blocks.BNState(torch.full((c.cout,), 1.5, device=DEV), torch.full((c.cout,), -0.25, device=DEV), torch.zeros(c.cout, device=DEV),
                              torch.ones(c.cout, device=DEV), torch.zeros((), device=DEV, dtype=torch.int64))
    bn_a, bn_b = bn_state(), bn_state()
    got = blocks.bn_coeff(y1, bn_a, True, blocks.Small(DEV), fused={"part": stats[:parts].reshape(-1), "nparts": parts})[:4]
    ref = blocks.bn_coeff(y1, bn_b, True, blocks.Small(DEV))[:4]
    for a, r, name in zip(got, ref, ("scale", "shift", "mean", "invstd")):
        err = float((a - r).abs().max() / r.abs().max())
        note("runet_convt4_igemm_stats " + name, err)
        assert err <= 2e-6, (name, err)
    assert float((bn_a.running_mean - bn_b.running_mean).abs().max()) <= 2e-6 * float(bn_b.running_mean.abs().max() + 1e-3)
    assert float((bn_a.running_var - bn_b.running_var).abs().max() / bn_b.running_var.abs().max()) <= 2e-6


# ------------------------------------------------------------------------------------------------ c. runet_gemm_batched
@pytest.mark.parametrize("c", R.gemm_cases(), ids=lambda c: c.id)
def test_gemm_batched_every_branch_against_float64(c):
    lib, check = L()
    assert lib.runet_gemm_batched_kernel_name(c.batch, c.rows, c.k, c.n).decode() == c.name
    a, b = R.randn((c.batch, c.rows, c.k), 1), R.randn((c.batch, c.k, c.n), 2)
    ref, mag = R.gemm(a.double(), b.double())
    lda, ldc = c.k + 8, c.n + 8
    sa, sb, sc = c.rows * lda + 16, c.k * c.n + 8, c.rows * ldc + 16          # batch strides larger than the matrices
    abuf, _, aptr = strided3(a, lda, 4, sa)
    bbuf, _, bptr = strided3(b, c.n, 4, sb)
    cbuf = guard((4 + c.batch * sc + ldc,), c.n)
    cview = torch.as_strided(cbuf, (c.batch, c.rows, c.n), (sc, ldc, 1), 4)
    cview.fill_(NAN)
    snap = cbuf.clone()
    check(lib.runet_gemm_batched(aptr, lda, sa, bptr, sb, cbuf.data_ptr() + 16, ldc, sc, c.batch, c.rows, c.k, c.n, st()))
    got = cview.clone()
    within("runet_gemm_batched", got, ref.to(DEV), R.bound(R.ceil16(c.k), mag).to(DEV), c.id)
    cview.fill_(NAN)
    assert torch.equal(torch.isnan(cbuf), torch.isnan(snap)) and torch.equal(cbuf.nan_to_num(), snap.nan_to_num()), "C changed outside rows x n"


# ------------------------------------------------------------------------------------------------ d. runet_gemm_tn_batched
@pytest.mark.parametrize("rows", R.TN_ROWS)
@pytest.mark.parametrize("k", R.TN_KN)
def test_gemm_tn_batched_against_float64(k, rows):
    """split-K slabs of A^T B: three splits, the last one short; rows = 80 takes the loaders without predicates, 77 the general ones.  k and n
    both > 64: gemm_tn_kernel, otherwise wgrad_kernel<64, 64, 32, 32>."""
    lib, check = L()
    batch, rps = R.TN_BATCH, R.TN_RPS
    splits = -(-rows // rps)
    assert splits == 3 and rows - 2 * rps < rps
    for n in R.TN_KN:
        a, b = R.randn((batch, rows, k), k + n), R.randn((batch, rows, n), k + n + 1)
        ref, mag = R.gemm_tn_split(a.double(), b.double(), rps)
        lda, ldb = k + 8, n + 8
        sa, sb = rows * lda + 16, rows * ldb + 16
        abuf, _, aptr = strided3(a, lda, 4, sa)
        bbuf, _, bptr = strided3(b, ldb, 4, sb)
        numel = splits * batch * k * n
        cbuf = guard((numel + 64,), k + n)
        cbuf[:numel] = NAN
        tail = cbuf[numel:].clone()
        check(lib.runet_gemm_tn_batched(aptr, lda, sa, bptr, ldb, sb, cbuf.data_ptr(), batch, rows, k, n, rps, st()))
        got = cbuf[:numel].reshape(splits, batch, k, n)
        assert torch.equal(cbuf[numel:], tail)
        ref, mag = ref.to(DEV), mag.to(DEV)
        for s in range(splits):          # each slab against the bound of its own rows
            within("runet_gemm_tn_batched", got[s], ref[s], R.bound(min(rps, rows - s * rps), mag[s]), f"k {k} n {n} rows {rows} slab {s}")
        within("runet_gemm_tn_batched", got.double().sum(0), ref.sum(0), R.bound(rows + splits, mag.sum(0)), f"k {k} n {n} rows {rows} slabs summed")


def wgrad_run(c, p, ws_floats):
    """runet_conv_wgrad with a workspace of ws_floats floats (0: none) -> dw [k, k, cin_w, cout]"""
    lib, check = L()
    xbuf, xptr, ldx = src_slice(p.x)
    ybuf, yptr, ldy = src_slice(p.dy)
    numel = c.k * c.k * c.cin_w * c.cout
    dw = guard((numel + 64,), c.cin + c.cout)
    dw[:numel] = NAN
    tail = dw[numel:].clone()
    ws = guard((ws_floats + 64,), 5) if ws_floats else None
    wtail = ws[ws_floats:].clone() if ws_floats else None
    check(lib.runet_conv_wgrad(xptr, ldx, yptr, ldy, dw.data_ptr(), ws.data_ptr() if ws_floats else None, ws_floats, c.n, c.h, c.w, c.cin, c.cin_w,
                               c.cout, c.k, c.k, c.dil, c.tr, st()))
    assert torch.equal(dw[numel:], tail), "dw written past its end"
    assert ws is None or torch.equal(ws[ws_floats:], wtail), "workspace written past the size given"
    return dw[:numel].reshape(c.k, c.k, c.cin_w, c.cout).clone()


NINE = [R.NS(route="nine", slabs=5, n=3, h=9, w=11, cin=ci, cin_w=ci, cout=co, k=1, dil=1, tr=0, id=f"1x1-{ci}-{co}") for ci in (20, 36, 68) for co in (20, 36, 68)]


@pytest.mark.parametrize("c", NINE, ids=lambda c: c.id)
def test_one_by_one_wgrad_nine_channel_classes_against_float64(c):
    """1 x 1 weight gradients with cin, cout each <= 32, <= 64, > 64 (all below the 128 channels of the TN GEMM route): the four
    wgrad_tile_kernel<1, TM, TN> instances, one or two 64-channel chunks per side, ragged against every one of them"""
    lib, _ = L()
    p = R.wgrad_problem(c)
    ref, mag = p.ref()
    ws = lib.runet_conv_wgrad_workspace_floats(c.n, c.h, c.w, c.cin_w, c.cout, 1, 1)
    assert ws >= c.slabs * c.cin * c.cout
    got = wgrad_run(c, p, ws)
    within("runet_conv_wgrad", got, ref.to(DEV), R.bound(p.pixels + c.slabs, mag).to(DEV), c.id)      # 5 tiles of 64 pixels


# ------------------------------------------------------------------------------------------------ e. runet_conv_wgrad
@pytest.mark.parametrize("c", R.wgrad_cases(), ids=lambda c: c.id)
def test_conv_wgrad_every_route_against_float64(c):
    """each route with the workspace runet_conv_wgrad_workspace_floats asks for, with one slab and with none (the routes of these cases re-plan
    their splits instead of refusing); a repeated call gives the same bits"""
    lib, _ = L()
    p = R.wgrad_problem(c)
    ref, mag = p.ref()
    ref, mag = ref.to(DEV), mag.to(DEV)
    ws = lib.runet_conv_wgrad_workspace_floats(c.n, c.h, c.w, c.cin_w, c.cout, c.k, c.k)
    wsize = c.k * c.k * c.cin_w * c.cout
    assert ws >= c.slabs * wsize
    for floats, slabs in ((ws, c.slabs), (wsize, 1), (0, 1)):
        got = wgrad_run(c, p, floats)
        within("runet_conv_wgrad", got, ref, R.bound(p.pixels + slabs, mag), f"{c.id} workspace {floats}")
        assert torch.equal(wgrad_run(c, p, floats), got), "not bitwise reproducible"


def test_conv_wgrad_direct_route_refuses_a_missing_workspace():
    """the 1 x 1 direct route does not re-plan: 513 pixels make two splits, and without the slabs' workspace the call returns an error"""
    lib, _ = L()
    x = torch.zeros(3, 9, 19, 132, device=DEV)
    dw = torch.zeros(132, 132, device=DEV)
    assert lib.runet_conv_wgrad_workspace_floats(3, 9, 19, 132, 132, 1, 1) >= 2 * 132 * 132
    rc = lib.runet_conv_wgrad(x.data_ptr(), 132, x.data_ptr(), 132, dw.data_ptr(), None, 0, 3, 9, 19, 132, 132, 132, 1, 1, 1, 0, st())
    assert rc != 0 and b"workspace too small" in lib.runet_last_error()


# ------------------------------------------------------------------------------------------------ f. reduced precision
def rounded(t, prec):
    return (t.bfloat16() if prec == "bf16" else t.half()).double()


def lowp_close(entry, got, ref, what, tol=2e-4):
    """tests/test_gpu_bf16.py's _close: within 2e-4 of the output's scale"""
    scale = float(ref.abs().max()) + 1e-30
    err = float((got.double() - ref).abs().nan_to_num(nan=float("inf")).max())
    note(entry + " err/scale", err / scale)
    assert err <= tol * scale, f"{entry} {what}: max err {err:.3e} vs scale {scale:.3e}"


def lowp_run(c, prec, variants, force):
    lib, check = L()
    p = R.op_problem(c)
    taps = c.k * c.k
    dgrad = c.kind.endswith("dgrad")
    wp = torch.zeros(getattr(lib, f"runet_{prec}_pack_elems")(taps, c.cin, c.cout), device=DEV, dtype=torch.bfloat16 if prec == "bf16" else torch.float16)
    w_dev, bias_dev = p.w.to(DEV), p.bias.to(DEV)
    # the forward weight is [taps][cin][cout] for a forward and [taps][cout][cin] (this call's naming) for a data gradient
    check(getattr(lib, f"runet_{prec}_pack_weights")(w_dev.data_ptr(), wp.data_ptr(), taps, c.cout if dgrad else c.cin, c.cin if dgrad else c.cout,
                                                      int(dgrad), st()))
    entry = f"runet_conv_igemm_{prec}"
    refs = {(b, a): p.fn(rounded(p.x, prec), rounded(p.w, prec), p.bias.double() if b else None, p.old.double() if a else None)[0].to(DEV)
            for b in (False, True) for a in (0, 1)}
    for variant in variants:
        if variant is not None:
            force(variant, lowp=True)
        for bias in (False, True):
            for acc in (0, 1):
                xbuf, xptr, ldx = src_slice(p.x)
                d = Dst((c.n,) + p.dst_hw, c.cout, p.old if acc else None)
                check(getattr(lib, entry)(xptr, ldx, wp.data_ptr(), bias_dev.data_ptr() if bias else None, d.ptr, d.ld, c.n, c.h, c.w, c.cin, c.cout,
                                          c.k, c.k, c.dil, MODE[c.kind], acc, st()))
                lowp_close(entry, d.result(), refs[bias, acc], f"{c.id} variant {variant} bias {bias} accumulate {acc}")


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("c", R.lowp_cases(), ids=lambda c: c.id)
def test_lowp_igemm_every_tile_variant_equals_the_convolution_of_rounded_operands(c, prec, force):
    lowp_run(c, prec, range(3), force)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("c", R.lowp_c3_cases(), ids=lambda c: c.id)
def test_lowp_patch_kernel_ragged_last_patch(c, prec, force):
    """3 x 3, dilation 1: the patch kernel of height 8 here, of height 16 in the child run below (RUNET_C3_PH=16); h = 5, 17, 33 leave a
    ragged last patch either way"""
    lowp_run(c, prec, (None,), force)


def test_lowp_patch_height_16_in_a_child_process():
    """RUNET_C3_PH is read once per process: tests/test_gpu_bf16.py's two kernel-level tests and the ragged-patch cases above run again in ONE
    fresh child with the patch height forced to 16 (the choice that needs >= 512 blocks otherwise)"""
    env = dict(os.environ, RUNET_C3_PH="16")
    here = os.path.abspath(__file__)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(os.path.dirname(here), "test_gpu_bf16.py"), here, "-q", "-x", "-s", "-m", "gpu", "-k",
                        "conv_fwd_dgrad_wgrad_equal_fp32_conv_of_rounded_operands or lowp_patch_kernel_ragged", "-p", "no:cacheprovider"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=os.path.dirname(os.path.dirname(here)))
    print("\n".join(ln for ln in r.stdout.splitlines() if "worst" in ln).replace("worst", "worst (RUNET_C3_PH=16)"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    ran = 9 + 4 + 2 * len(R.lowp_c3_cases())          # test_gpu_bf16.py's nine bf16 and four fp16 kernel-level cases, the ragged patches in both types
    assert f"{ran} passed" in r.stdout, r.stdout[-500:]


def test_the_forced_variant_hooks_are_back_at_automatic():
    """runs last in this file: the name the automatic choice reports (128 x 64 for 297 pixels x 36 channels; 64 x 64 for a 1 x 1 with K <= 128)"""
    lib, _ = L()
    assert "<128, 64, 64, 32," in lib.runet_conv_igemm_kernel_name(3, 9, 11, 20, 36, 3, R.FWD).decode()
    assert "<64, 64, 32, 32," in lib.runet_conv_igemm_kernel_name(3, 9, 11, 48, 132, 1, R.FWD).decode()
