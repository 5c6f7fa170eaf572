"""The split-operand ("bf16x6") kernels at non-finite, huge and tiny operands (contract C1 - C4): the position GEMMs
and their packer, the TN GEMM, the 1x1 / k2-s2 transposed convolutions with their TN weight gradients, the fused F(2x2) kernel and
F(4x4) on the position GEMMs.  Every case compares with the float64 reference of the same run (tests/x3_ref.py, which also holds the
edge sets, the touched-output geometry and the limits; tests/test_x3_ref_cpu.py shows that these checks reject the parent's split
and three named mistakes).  The clean run of a case replaces the planted elements by 0.5; every output outside the touched mask
must equal it bit for bit.

Accuracy bounds: the GEMM forms 4e-6 of scale and the rms bound x3_ref.rms_tol(k) of their contraction, the Winograd forms what
tests/test_gpu_conv.py holds them to on Gaussian data (F(2x2) 3e-4, F(4x4) 2e-4, its weight gradient 5e-4), tiny operands
x3_ref.tiny_limit(s)."""
import importlib
import itertools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import x3_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TWO_120 = 2.0 ** 120

def _cases(*axes):
    """the product of R.KINDS and `axes`: one kernel and one planted kind per case, so that no failure hides another"""
    return list(itertools.product(R.KINDS, *axes))


def _ops():
    return importlib.import_module("eusipco-2026-robust-unet_amd.ops")


def _lib():
    return importlib.import_module("eusipco-2026-robust-unet_amd._lib")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _x3_route(ops, monkeypatch):
    monkeypatch.setattr(ops, "CONV_X3_MIN_K", 16)
    monkeypatch.setattr(ops, "CONV_X3_WIDE_N", 4)
    seen = []
    real = ops._conv_x3
    monkeypatch.setattr(ops, "_conv_x3", lambda mode, *a, **kw: (seen.append(mode), real(mode, *a, **kw))[1])
    return seen


# ------------------------------------------------------------------------------------------------------------ 1, 2: the GEMMs themselves
def _gemm_nn(a, b):
    """runet_gemm_x3_pack + runet_gemm_x3_batched, row stride n + 4: the columns beyond n stay 7.0 bit for bit"""
    L = _lib()
    B, rows, k = a.shape
    n = b.shape[2]
    a, b = a.to(DEV), b.to(DEV)
    bp = torch.empty(L.lib.runet_gemm_x3_pack_elems(B, k, n), device=DEV, dtype=torch.bfloat16)
    L.check(L.lib.runet_gemm_x3_pack(b.data_ptr(), k * n, bp.data_ptr(), B, k, n, _stream()))
    c = torch.full((B, rows, n + 4), 7.0, device=DEV)
    L.check(L.lib.runet_gemm_x3_batched(a.data_ptr(), k, rows * k, bp.data_ptr(), c.data_ptr(), n + 4, rows * (n + 4), B, rows, k, n, _stream()))
    assert torch.equal(c[..., n:], torch.full((B, rows, 4), 7.0, device=DEV))
    return c[..., :n].cpu()


def _gemm_tn(a, b, rps=48):
    """runet_gemm_x3_tn_batched -> the per-split products [splits, B, k, n], before the host-side sum"""
    L = _lib()
    B, rows, k = a.shape
    n = b.shape[2]
    a, b = a.to(DEV), b.to(DEV)
    cu = torch.full((-(-rows // rps), B, k, n), 7.0, device=DEV)
    L.check(L.lib.runet_gemm_x3_tn_batched(a.data_ptr(), k, rows * k, b.data_ptr(), n, rows * n, cu.data_ptr(), B, rows, k, n, rps, _stream()))
    return cu.cpu()


@pytest.mark.parametrize("kind,side", _cases(("a", "b")))
def test_position_gemm_and_packer_keep_the_contract(kind, side):
    """side a: the operand split inside gemm_nn_x3_kernel; side b: the one split by runet_gemm_x3_pack.  Elements at the first and last k,
    both sides of the k-octet (7 | 8) and k-step (15 | 16), rows 127 | 128 and the ragged row 129, columns 31 | 32 and the ragged column 35."""
    es = R.gemm_edge_set(kind, side)
    got, clean = _gemm_nn(es["a"], es["b"]), _gemm_nn(es["a_clean"], es["b_clean"])
    R.check_finite_contract(got, R.mm64(es["a"], es["b"]), es["touched"], clean, rms_tol=R.RMS_TOL, what=f"NN, {kind} in {side}")


@pytest.mark.parametrize("kind,side", _cases(("a", "b")))
def test_tn_gemm_keeps_the_contract_per_split(kind, side):
    """144 rows in three splits of 48: an element of row r reaches output row (side a) or column (side b) of ITS split only"""
    es = R.tn_edge_set(kind, side)
    got, clean = _gemm_tn(es["a"], es["b"]), _gemm_tn(es["a_clean"], es["b_clean"])
    R.check_finite_contract(got, R.tn_split_ref(es["a"], es["b"]), es["touched"], clean, rms_tol=R.RMS_TOL, what=f"TN, {kind} in {side}")


# ------------------------------------------------------------------------------------------------------------ 3: 1x1 and transposed convolutions
# activation spots (image, row, column, channel) of a 6 x 10 image: pixels 0, 7 | 8, 15 | 16 and the last (60 pixels: ragged row tile),
# channels = the k positions of the GEMM set; one element per pixel
X_SPOTS = ((0, 0, 0, 0), (0, 0, 7, 7), (0, 0, 8, 8), (0, 1, 5, 15), (0, 1, 6, 16), (0, 5, 9, 47))
# the same for the 12 x 20 gradient of the transposed convolution: one element per LOW-resolution pixel (its dot product holds the four taps)
DY2_SPOTS = ((0, 0, 0, 0), (0, 1, 14, 7), (0, 0, 17, 8), (0, 3, 11, 15), (0, 2, 12, 16), (0, 11, 19, 47))
# weight spots (tap row, tap column, ci, co): forward modes contract over ci (one element per co), data-gradient modes over co (one per ci)
W_FWD_SPOTS = ((0, 0, 0, 0), (0, 1, 7, 31), (1, 0, 8, 32), (1, 1, 47, 35), (0, 0, 15, 5), (1, 1, 16, 33))
W_DGRAD_SPOTS = ((0, 0, 0, 0), (0, 1, 31, 7), (1, 0, 32, 8), (1, 1, 47, 47), (0, 0, 5, 15), (1, 1, 33, 16))


def _kpos(spots, axis):
    return sorted({s[axis] for s in spots})


CONV_FORMS = ("1x1 forward", "1x1 data gradient", "transposed forward", "transposed data gradient")


@pytest.mark.parametrize("kind,side,form", _cases(("activation", "weight"), CONV_FORMS))
def test_conv_x3_forms_keep_the_contract(kind, side, form, monkeypatch):
    """ops.conv_fwd (channel-slice source, accumulate destination with finite content), conv_dgrad, convt_fwd, convt_dgrad at 1 x 6 x 10,
    48 -> 36 (48 -> 48 for the data gradients, whose contraction must be a multiple of 16), each on the split-operand route; rms bound of
    the contraction's length (48; 192 for the transposed data gradient) beside the 4e-6 of scale"""
    ops = _ops()
    seen = _x3_route(ops, monkeypatch)
    n, h, w, ci = 1, 6, 10, 48

    def case(name, act_shape, w_shape, x_spots, w_spots, w_axis, run, ref, touch_x, touch_w, mode, k=48):
        if name != form:
            return
        act, wt = R.gaussian(act_shape, 70), R.gaussian(w_shape, 71) / ci ** 0.5
        if side == "activation":
            e, c = R.plant(act, kind, x_spots, 3)
            wt = R.partner(wt, kind, _kpos(x_spots, 3), w_axis)
            pairs, touched = ((e, wt), (c, wt)), touch_x(x_spots)
        else:
            spots = [s if len(w_shape) == 4 and w_shape[0] == 2 else (0, 0) + tuple(s[2:]) for s in w_spots]
            e, c = R.plant(wt, kind, spots, w_axis)
            act = R.partner(act, kind, _kpos(spots, w_axis), 3)
            pairs, touched = ((act, e), (act, c)), touch_w(spots)
        got, clean = (run(a.to(DEV), b.to(DEV)).cpu() for a, b in pairs)
        worst = R.check_finite_contract(got, ref(*pairs[0]), touched, clean, rms_tol=R.rms_tol(k), what=f"{name}, {kind} in the {side}")
        print(f"{name}: {kind} in the {side}: worst finite error {worst:.2e} of scale")
        assert seen == [mode, mode], seen

    def px_mask(shape, pixels):
        m = torch.zeros(shape, dtype=torch.bool)
        for p in pixels:
            m[p] = True
        return m

    def ch_mask(shape, chans, parity=None):
        m = torch.zeros(shape, dtype=torch.bool)
        for s, c in chans:
            if parity:
                m[:, s[0]::2, s[1]::2, c] = True
            else:
                m[..., c] = True
        return m

    # 1x1 forward: source a channel slice of a wider buffer, destination accumulates onto 2.0
    def fwd(x, wt):
        big = torch.zeros(n, h, w, ci + 32, device=DEV)
        big[..., 16:16 + ci] = x
        out = torch.full((n, h, w, 36 + 8), 2.0, device=DEV)
        ops.conv_fwd(big[..., 16:16 + ci], wt, None, out=out[..., 4:40], accumulate=True)
        assert torch.equal(out[..., :4], torch.full((n, h, w, 4), 2.0, device=DEV)) and torch.equal(out[..., 40:], out[..., :4])
        return out[..., 4:40]
    case("1x1 forward", (n, h, w, ci), (1, 1, ci, 36), X_SPOTS, W_FWD_SPOTS, 2, fwd,
         lambda x, wt: R.mm64(x.reshape(1, -1, ci), wt[0, 0][None]).reshape(n, h, w, 36) + 2.0,
         lambda sp: px_mask((n, h, w, 36), [s[:3] for s in sp]), lambda sp: ch_mask((n, h, w, 36), [(s, s[3]) for s in sp]), ops.CONV_FWD)
    case("1x1 data gradient", (n, h, w, 48), (1, 1, ci, 48), X_SPOTS, W_DGRAD_SPOTS, 3, lambda dy, wt: ops.conv_dgrad(dy, wt),
         lambda dy, wt: R.mm64(dy.reshape(1, -1, 48), wt[0, 0].t()[None]).reshape(n, h, w, ci),
         lambda sp: px_mask((n, h, w, ci), [s[:3] for s in sp]), lambda sp: ch_mask((n, h, w, ci), [(s, s[2]) for s in sp]), ops.CONV_DGRAD)
    case("transposed forward", (n, h, w, ci), (2, 2, ci, 36), X_SPOTS, W_FWD_SPOTS, 2, lambda x, wt: ops.convt_fwd(x, wt), R.convt_ref,
         lambda sp: px_mask((n, 2 * h, 2 * w, 36), [(s[0], 2 * s[1] + a, 2 * s[2] + b) for s in sp for a in (0, 1) for b in (0, 1)]),
         lambda sp: ch_mask((n, 2 * h, 2 * w, 36), [(s, s[3]) for s in sp], parity=True), ops.CONVT_FWD)
    case("transposed data gradient", (n, 2 * h, 2 * w, 48), (2, 2, ci, 48), DY2_SPOTS, W_DGRAD_SPOTS, 3, lambda dy, wt: ops.convt_dgrad(dy, wt),
         R.convt_dgrad_ref, lambda sp: px_mask((n, h, w, ci), [(s[0], s[1] // 2, s[2] // 2) for s in sp]),
         lambda sp: ch_mask((n, h, w, ci), [(s, s[2]) for s in sp]), ops.CONVT_DGRAD, k=192)
    assert len(seen) == 2, (form, seen)


# ------------------------------------------------------------------------------------------------------------ 4: their weight gradients (TN route)
@pytest.mark.parametrize("kind,side,form", _cases(("x", "dy"), ("1x1", "transposed")))
def test_tn_weight_gradients_keep_the_contract(kind, side, form):
    """ops.conv_wgrad (1x1) at 2 x 16 x 16, 128 -> 128 and ops.convt_wgrad at 1 x 4 x 16, 64 -> 64: the smallest shapes csrc/conv_igemm.hip
    sends to the split-operand TN GEMM (1x1: both channel counts >= 128 and a multiple of 16 pixels - 512 of them make two splits and the
    slab reduction; transposed: width a multiple of 16, both channel counts >= 64).  One poisoned element of x makes row ci of dW
    non-finite, one of dy column co, nothing else.  Both routes are pinned by bit-equality of the clean run with the TN GEMM's own entry point
    (runet_gemm_x3_tn_batched, two slabs of 256 rows summed; runet_gemm_x3_tn_convt, one slab of 64 rows); rms bound of the contraction's length."""
    ops, L = _ops(), _lib()
    for name, (n, h, w, ci, co), spot, chan in (("1x1", (2, 16, 16, 128, 128), (1, 7, 8), 33), ("transposed", (1, 4, 16, 64, 64), (0, 3, 15), 63)):
        if name != form:
            continue
        up = 1 if name == "1x1" else 2
        x, dy = R.gaussian((n, h, w, ci), 80), R.gaussian((n, up * h, up * w, co), 81)
        touched = torch.zeros(up, up, ci, co, dtype=torch.bool)
        if side == "x":
            xs = (spot[0], spot[1], spot[2], chan)
            e, c = _plant_pixel(x, kind, R._VALUE[kind], xs, second=(spot[0], spot[1], spot[2] - 1, chan))
            d = dy.clone()
            if kind in R.HUGE_KINDS:
                d *= R.PARTNER_SCALE
            if kind in ("inf_x_zero", "inf_x_one"):      # the partners of the pixel: its up x up gradient pixels
                d[spot[0], up * spot[1]:up * spot[1] + up, up * spot[2]:up * spot[2] + up] = 0.0 if kind == "inf_x_zero" else 1.0
            pairs = ((e, d), (c, d))
            touched[:, :, chan] = True
        else:                                            # the gradient pixel of tap (up - 1, 0); the -Inf of "pinf_ninf" one low-resolution pixel to the left
            ds = (spot[0], up * spot[1] + up - 1, up * spot[2], chan)
            e, c = _plant_pixel(dy, kind, R._VALUE[kind], ds, second=(ds[0], ds[1], ds[2] - up, chan))
            xx = x.clone()
            if kind in R.HUGE_KINDS:
                xx *= R.PARTNER_SCALE
            if kind in ("inf_x_zero", "inf_x_one"):
                xx[spot[0], spot[1], spot[2]] = 0.0 if kind == "inf_x_zero" else 1.0
            pairs = ((xx, e), (xx, c))
            touched[((slice(None), slice(None)) if up == 1 else (up - 1, 0)) + (slice(None), chan)] = True

        def run(a, b):
            a, b = a.to(DEV), b.to(DEV)
            got = ops.conv_wgrad(a, b, 1, 1, on_side=False) if up == 1 else ops.convt_wgrad(a, b)
            return got.cpu()
        got, clean = run(*pairs[0]), run(*pairs[1])
        ref = R.mm64(pairs[0][0].reshape(1, -1, ci).transpose(1, 2), pairs[0][1].reshape(1, -1, co)) if up == 1 else R.convt_wgrad_ref(*pairs[0])
        worst = R.check_finite_contract(got, ref.reshape(up, up, ci, co), touched, clean, rms_tol=R.rms_tol(n * h * w),
                                        what=f"{name} weight gradient, {kind} in {side}")
        print(f"{name} weight gradient: {kind} in {side}: worst finite error {worst:.2e} of scale")
        if up == 1:
            a, b = pairs[1][0].to(DEV), pairs[1][1].to(DEV)
            cu = torch.empty(2, ci, co, device=DEV)
            L.check(L.lib.runet_gemm_x3_tn_batched(a.data_ptr(), ci, 0, b.data_ptr(), co, 0, cu.data_ptr(), 1, n * h * w, ci, co, 256, _stream()))
            assert torch.equal((cu[0] + cu[1]).cpu(), clean[0, 0]), "the 1x1 weight gradient did not take the split-operand TN GEMM"
        else:
            a, b = pairs[1][0].to(DEV), pairs[1][1].to(DEV)
            cu = torch.empty(2, 2, ci, co, device=DEV)
            L.check(L.lib.runet_gemm_x3_tn_convt(a.data_ptr(), ci, b.data_ptr(), co, cu.data_ptr(), n, h, w, ci, co, 64, _stream()))
            assert torch.equal(cu.cpu(), clean), "the transposed weight gradient did not take the split-operand TN GEMM"


# ------------------------------------------------------------------------------------------------------------ 5, 6: Winograd
F2 = (2, 8, 8, 16, 32)


def _positions(n, h, w, dil):
    """(image, row, column, channel): pixel (0, 0), a tile corner (3, 4) (of the sub-image for dil > 1), the last pixel, image 1 only"""
    pos = [(0, 0, 0, 0), (0, 3 * dil + dil - 1, 4 * dil + dil - 1, 7), (0, h - 1, w - 1, 15)]
    return pos + ([(1, 3 * dil + dil - 1, 4 * dil + dil - 1, 8)] if n > 1 else [])


def _wino_kind(kind, m):
    """F(4x4): the huge-finite kinds plant +-2^120 in an activation - its input transform multiplies by up to 5 per side, and an overflow there
    is the algorithm's, not the split's"""
    if m == 4 and kind in R.HUGE_KINDS:
        return {"flt_max": TWO_120, "neg_flt_max": -TWO_120}.get(kind)
    return R._VALUE[kind]


def _plant_pixel(t, kind, value, pos, second=None):
    """second: where the -Inf of "pinf_ninf" goes (default: the next channel of the same pixel - the same dot products of a convolution that
    contracts over channels; the weight gradients contract over pixels and name a neighbouring pixel of the same channel)"""
    e, c = R.plant(t, "pinf" if second is not None and kind == "pinf_ninf" else kind, (pos,), 3)
    e[pos] = value
    if second is not None and kind == "pinf_ninf":
        e[second], c[second] = float("-inf"), R.CLEAN
    return e, c


def _wino_case(kind, m, act, wt, pos, dil, run, ref, out_ch, adjoint, tol, what):
    """One activation element poisoned: the outputs of the tiles whose window holds the pixel may change, image and tiles beyond are bit-equal."""
    value = _wino_kind(kind, m)
    if value is None:
        return
    n, h, w, k = act.shape
    e, c = _plant_pixel(act, kind, value, pos)
    wt = R.partner(wt, kind, [pos[3]], 2 if not adjoint else 3)
    got, clean = run(e, wt), run(c, wt)
    touched = R.wino_touched((n, h, w), m, dil, (pos[:3],), adjoint=adjoint)[..., None].expand(n, h, w, out_ch)
    if pos[0] == 1:
        assert torch.equal(got[0], clean[0]), f"{what}: image 0 changed with an element of image 1"
    worst = R.check_finite_contract(got, ref(e, wt), touched, clean, tol=tol, strict_inside=kind in R.HUGE_KINDS, what=f"{what}, {kind} at {pos}")
    print(f"{what}: {kind} at {pos}: worst finite error {worst:.2e} of scale")


def _f2_operands():
    n, h, w, ci, co = F2
    return R.gaussian((n, h, w, ci), 90), R.gaussian((n, h, w, co), 91), R.gaussian((3, 3, ci, co), 92) / (9 * ci) ** 0.5


def _f2_run(a, wv, dgrad=False):
    ops = _ops()
    ci, co = F2[3:]
    U = ops.wino_weights(wv.to(DEV), dgrad=dgrad)
    k, nn_ = (co, ci) if dgrad else (ci, co)
    assert U.dtype == torch.bfloat16 and U.numel() == 16 * 3 * k * nn_, "not the split-plane filter"
    return ops.wino_conv(a.to(DEV), U).cpu()


@pytest.mark.parametrize("kind,pos,form", _cases(_positions(*F2[:3], 1), ("forward", "data gradient")))
def test_fused_f2_keeps_the_contract(kind, pos, form):
    """ops.wino_conv on the split-plane filter, 2 x 8 x 8, 16 -> 32, forward and dgrad=True, one poisoned pixel per case"""
    n, h, w, ci, co = F2
    x, dy, wt = _f2_operands()
    if form == "forward":
        _wino_case(kind, 2, x, wt, pos, 1, _f2_run, R.conv3_ref, co, False, 3e-4, "F(2x2) forward")
    else:
        _wino_dgrad_case(kind, 2, dy, wt, pos, lambda a, wv: _f2_run(a, wv, True), ci)


@pytest.mark.parametrize("kind", R.KINDS)
def test_fused_f2_filter_keeps_the_contract(kind):
    """the filter (runet_wino_weights_x3: G g G^T + split): element (r, s, ci, co) reaches output channel co (forward) / input channel ci
    (data gradient) only"""
    n, h, w, ci, co = F2
    x, dy, wt = _f2_operands()
    for spot, act, dgrad, ref, out_ch, ch in (((1, 2, 7, 31), x, False, R.conv3_ref, co, 31), ((2, 0, 8, 16), dy, True, R.conv3_dgrad_ref, ci, 8)):
        e, c = R.plant(wt, kind, (spot,), 3 if dgrad else 2)
        a = R.partner(act, kind, [spot[3 if dgrad else 2]], 3)
        got, clean = _f2_run(a, e, dgrad), _f2_run(a, c, dgrad)
        touched = torch.zeros(n, h, w, out_ch, dtype=torch.bool)
        touched[..., ch] = True
        R.check_finite_contract(got, ref(a, e), touched, clean, tol=3e-4, strict_inside=kind in R.HUGE_KINDS, what=f"F(2x2) filter {spot}, dgrad {dgrad}, {kind}")


def _wino_dgrad_case(kind, m, dy, wt, pos, run, cin, dil=1, adjoint=False, tol=3e-4, what="F(2x2) data gradient"):
    """the data gradient reads dy (channels = the filter's output side): partner elements along the filter's co axis"""
    value = _wino_kind(kind, m)
    if value is None:
        return
    n, h, w, _ = dy.shape
    e, c = _plant_pixel(dy, kind, value, pos)
    wv = R.partner(wt, kind, [pos[3]], 3)
    got, clean = run(e, wv), run(c, wv)
    touched = R.wino_touched((n, h, w), m, dil, (pos[:3],), adjoint=adjoint)[..., None].expand(n, h, w, cin)
    if pos[0] == 1:
        assert torch.equal(got[0], clean[0]), f"{what}: image 0 changed with an element of image 1"
    worst = R.check_finite_contract(got, R.conv3_dgrad_ref(e, wv, dil), touched, clean, tol=tol, strict_inside=kind in R.HUGE_KINDS,
                                    what=f"{what}, {kind} at {pos}")
    print(f"{what}: {kind} at {pos}: worst finite error {worst:.2e} of scale")


F4_SHAPES = [(2, 8, 8, 32, 48, 1), (1, 12, 20, 64, 32, 1), (2, 16, 16, 64, 32, 2)]
F4_KINDS = R.NONFINITE_KINDS + ("flt_max", "neg_flt_max")      # the two huge-finite kinds plant +2^120 / -2^120 here (_wino_kind)


@pytest.mark.parametrize("n,h,w,ci,co,dil", F4_SHAPES)
@pytest.mark.parametrize("kind", F4_KINDS)
def test_f4_on_the_position_gemm_keeps_the_contract(kind, n, h, w, ci, co, dil):
    """ops.wino4_conv, ops.wino4_dgrad_adj (touched: the 6 x 6 window of the tile that holds the gradient pixel) and ops.wino4_wgrad (direct,
    from the forward's kept V, from the adjoint data gradient's kept Z): a poisoned x pixel reaches rows ci of dW, a poisoned dy pixel columns co"""
    ops = _ops()
    assert ops.wino4_ok(h // dil, w // dil, ci, co) and ops._x3_case(ci) and ops._x3_case(co)
    x, dy, wt = R.gaussian((n, h, w, ci), 100), R.gaussian((n, h, w, co), 101), R.gaussian((3, 3, ci, co), 102) / (9 * ci) ** 0.5

    def fwd(a, wv):
        U = ops.wino4_weights(wv.to(DEV))
        assert U.dtype == torch.bfloat16
        return ops.wino4_conv(a.to(DEV), U, dil=dil).cpu()

    def adj(a, wv):
        return ops.wino4_dgrad_adj(a.to(DEV), wv.to(DEV), dil=dil).cpu()
    for pos in _positions(n, h, w, dil):
        _wino_case(kind, 4, x, wt, pos, dil, fwd, lambda a, wv: R.conv3_ref(a, wv, dil), co, False, 2e-4, f"F(4x4) forward dil {dil}")
        _wino_dgrad_case(kind, 4, dy, wt, pos, adj, ci, dil=dil, adjoint=True, tol=2e-4, what=f"F(4x4) adjoint data gradient dil {dil}")
    # weight gradients: one run per side at the tile-corner position
    pos = _positions(n, h, w, dil)[1]
    value = _wino_kind(kind, 4)
    for side in ("x", "dy"):
        src, other = (x, dy) if side == "x" else (dy, x)
        e, c = _plant_pixel(src, kind, value, pos, second=(pos[0], pos[1], pos[2] - dil, pos[3]))
        o = other.clone()
        if kind in R.HUGE_KINDS:
            o *= R.PARTNER_SCALE
        if kind in ("inf_x_zero", "inf_x_one"):      # every partner the 3x3 window can pair the pixel with
            i, j = pos[1], pos[2]
            o[pos[0], max(0, i - dil):i + dil + 1, max(0, j - dil):j + dil + 1] = 0.0 if kind == "inf_x_zero" else 1.0
        pairs = ((e, o), (c, o)) if side == "x" else ((o, e), (o, c))
        touched = torch.zeros(3, 3, ci, co, dtype=torch.bool)
        touched[(slice(None), slice(None), pos[3]) if side == "x" else (slice(None), slice(None), slice(None), pos[3])] = True
        ref = R.conv3_wgrad_ref(*pairs[0], dil)
        wd = wt.to(DEV)

        def direct(a, b):
            return ops.wino4_wgrad(a.to(DEV), b.to(DEV), dil=dil).cpu()

        def from_v(a, b):
            keep = {}
            ops.wino4_conv(a.to(DEV), ops.wino4_weights(wd), keep_v=keep, dil=dil)
            return ops.wino4_wgrad(a.to(DEV), b.to(DEV), v=keep["V"], dil=dil).cpu()

        def from_z(a, b):
            kz = {}
            ops.wino4_dgrad_adj(b.to(DEV), wd, dil=dil, keep_z=kz)
            return ops.wino4_wgrad(a.to(DEV), b.to(DEV), z=kz["Z"], dil=dil).cpu()
        for name, run in (("direct", direct), ("kept V", from_v), ("kept Z", from_z)):
            got, clean = run(*pairs[0]), run(*pairs[1])
            R.check_finite_contract(got, ref, touched, clean, tol=5e-4, strict_inside=kind in R.HUGE_KINDS,
                                    what=f"F(4x4) weight gradient ({name}) dil {dil}, {kind} in {side}")


@pytest.mark.parametrize("kind", R.KINDS)
def test_f4_filter_and_tn_weight_gradient_keep_the_contract(kind):
    """the F(4x4) filter transform + split (derive_weights.h): element (2, 2, ci, co), which position (5, 5) of G g G^T carries unscaled, so
    the huge-finite kinds are the real ones here; and ops.wino4_wgrad at 1 x 16 x 16, 80 -> 80, the smallest shape on the split-operand TN
    GEMM (16 tiles, both channel counts above 64)"""
    ops = _ops()
    n, h, w, ci, co = 2, 8, 8, 32, 48
    x, wt = R.gaussian((n, h, w, ci), 110), R.gaussian((3, 3, ci, co), 111) / (9 * ci) ** 0.5
    spot = (2, 2, 15, 33)
    e, c = R.plant(wt, kind, (spot,), 2)
    a = R.partner(x, kind, [spot[2]], 3).to(DEV)
    got, clean = (ops.wino4_conv(a, ops.wino4_weights(v.to(DEV))).cpu() for v in (e, c))
    touched = torch.zeros(n, h, w, co, dtype=torch.bool)
    touched[..., spot[3]] = True
    R.check_finite_contract(got, R.conv3_ref(a.cpu(), e), touched, clean, tol=2e-4, strict_inside=kind in R.HUGE_KINDS, what=f"F(4x4) filter, {kind}")

    value = _wino_kind(kind, 4)
    if value is None:
        return
    n, h, w, ci, co = 1, 16, 16, 80, 80
    assert ops.wino4_ok(h, w, ci, co) and ops.USE_X3 and (n * (h // 4) * (w // 4)) % 16 == 0 and ci > 64 and co > 64
    x, dy = R.gaussian((n, h, w, ci), 112), R.gaussian((n, h, w, co), 113)
    pos = (0, 7, 8, 33)
    for side in ("x", "dy"):
        src, other = (x, dy) if side == "x" else (dy, x)
        e, c = _plant_pixel(src, kind, value, pos, second=(pos[0], pos[1], pos[2] - 1, pos[3]))
        o = other.clone()
        if kind in R.HUGE_KINDS:
            o *= R.PARTNER_SCALE
        if kind in ("inf_x_zero", "inf_x_one"):
            o[0, 6:9, 7:10] = 0.0 if kind == "inf_x_zero" else 1.0
        pairs = ((e, o), (c, o)) if side == "x" else ((o, e), (o, c))
        touched = torch.zeros(3, 3, ci, co, dtype=torch.bool)
        touched[(slice(None), slice(None), pos[3]) if side == "x" else (slice(None), slice(None), slice(None), pos[3])] = True
        got, clean = (ops.wino4_wgrad(p.to(DEV), q.to(DEV)).cpu() for p, q in pairs)
        R.check_finite_contract(got, R.conv3_wgrad_ref(*pairs[0]), touched, clean, tol=5e-4, strict_inside=kind in R.HUGE_KINDS,
                                what=f"F(4x4) weight gradient on the TN GEMM, {kind} in {side}")


# ------------------------------------------------------------------------------------------------------------ C4: tiny operands
def _tiny(t, s, seed=0):
    """t scaled by s; s = None: 1 % of the elements replaced by the fp32 denormal 1e-40"""
    if s is not None:
        return (t * s).float()
    t = t.clone()
    pick = torch.rand(t.shape, generator=torch.Generator().manual_seed(seed)) < 0.01
    t[pick] = 1e-40
    return t


@pytest.mark.parametrize("s", R.TINY_SCALES + (None,), ids=lambda s: "denormal" if s is None else f"{s:g}")
def test_tiny_operands_stay_within_the_limit_of_their_magnitude(s, monkeypatch):
    """C4, forward forms: one operand scaled by s; the limit is x3_ref.tiny_limit(s) = 4e-6 + 4 x the flushed-planes figure of the CPU
    restatement, never what the kernels give.  Prints the measured error of every form (profiles/x3_edge_accuracy.txt records a run)."""
    ops = _ops()
    seen = _x3_route(ops, monkeypatch)
    out = []
    B, rows, k, n = R.GEMM_SHAPE
    a, b = R.gaussian((B, rows, k), 120), R.gaussian((B, k, n), 121)
    out.append(("NN GEMM, A tiny", R.check_tiny(_gemm_nn(_tiny(a, s), b), R.mm64(_tiny(a, s), b), s, "NN, A", rms_tol=R.RMS_TOL)))
    out.append(("NN GEMM, packed B tiny", R.check_tiny(_gemm_nn(a, _tiny(b, s)), R.mm64(a, _tiny(b, s)), s, "NN, B", rms_tol=R.RMS_TOL)))
    B, rows, k, n = R.TN_SHAPE
    a, z = R.gaussian((B, rows, k), 122), R.gaussian((B, rows, n), 123)
    out.append(("TN GEMM, A tiny", R.check_tiny(_gemm_tn(_tiny(a, s), z).double().sum(0), R.mm64(_tiny(a, s).transpose(1, 2), z), s, "TN", rms_tol=R.RMS_TOL)))
    x, w1, w2 = _tiny(R.gaussian((1, 6, 10, 48), 124), s), R.gaussian((1, 1, 48, 36), 125) / 7, R.gaussian((2, 2, 48, 36), 126) / 7
    out.append(("1x1 forward, x tiny", R.check_tiny(ops.conv_fwd(x.to(DEV), w1.to(DEV)), R.mm64(x.reshape(1, 60, 48), w1[0, 0][None]).reshape(1, 6, 10, 36), s, "1x1")))
    out.append(("transposed forward, x tiny", R.check_tiny(ops.convt_fwd(x.to(DEV), w2.to(DEV)), R.convt_ref(x, w2), s, "transposed")))
    assert seen == [ops.CONV_FWD, ops.CONVT_FWD], seen
    x, wt = _tiny(R.gaussian((2, 8, 8, 32), 127), s), R.gaussian((3, 3, 32, 48), 128) / 17
    assert ops.wino4_ok(8, 8, 32, 48) and ops._x3_case(32)
    out.append(("F(4x4) forward, x tiny", R.check_tiny(ops.wino4_conv(x.to(DEV), ops.wino4_weights(wt.to(DEV))), R.conv3_ref(x, wt), s, "F(4x4)")))
    for name, err in out:
        print(f"s = {s}: {name}: {err:.3e} of scale (limit {1.0 if s is None else R.tiny_limit(s):.3e})")
