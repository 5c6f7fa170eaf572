"""Float64 reference, CPU restatement and the comparisons for the split-operand ("bf16x6") kernels at non-finite, huge and tiny
operands.  CPU only; tests/test_x3_ref_cpu.py checks this file against itself and against torch, tests/test_gpu_x3_edges.py calls it
with what the kernels give.

The kernels (csrc/x3_common.h `split1`, the "fixed" variant below, at every site) write an fp32 operand as x = h + m + l, three bf16
planes, and form a product from six bf16 MFMAs accumulated in fp32.  `planes` restates the split in torch (planes as bf16 tensors), `x3_matmul` the six products in the
kernels' order, each an exact float64 product of plane values, summed in float64 - so what it shows is the representation alone.

    variant "parent": h = bf16(x).  Any finite |x| >= 0x7F7F8000 (3.3961e38, FLT_MAX included) rounds to h = +-Inf, then
                      x - h = -+Inf and the next residual Inf - Inf = NaN: a finite operand poisons its whole dot product.
    variant "fixed":  h = bf16(clamp(x, +-bf16max)), residuals still from x itself: the same h for every |x| below the threshold,
                      x = h + m + l exact for every finite x, and Inf / NaN stay in the m plane.
    flush:            bf16 plane values below the smallest normal (2^-126) are read as 0 (a matrix core that flushes denormal A/B
                      inputs) or kept.

The contract, the reference being the same operation in float64 on the same fp32 operands:
    C1  finite operands whose float64 partial sums stay below 2^126 give finite outputs within the accuracy bound;
    C2  where the reference is +-Inf or NaN ours is non-finite; WHICH of the three is not specified: Inf x 1.0 is Inf in the
        reference and NaN here, because the m and l planes of 1.0 are exactly 0 and Inf x 0 = NaN;
    C3  an edge element changes only the outputs that read it (`touched`): every other output is bit-equal to the run with that
        element replaced by 0.5.  Inside a touched Winograd tile the output may be non-finite where the reference is finite (the
        transforms subtract);
    C4  the accuracy against float64 as a function of the operand magnitude s (`check_tiny`).

Representation error of a 130 x 48 x 36 product with A scaled by s, max |err| / max |ref|, by `measure()` (MEASURED; the CPU
test repeats it and fails if a figure has moved by more than a factor 2):

      s        planes kept    planes flushed
    1e+00       7.8e-09         7.8e-09
    1e-20       6.7e-09         6.7e-09
    1e-30       7.1e-09         7.1e-09
    1e-32       7.2e-09         3.3e-07
    1e-33       2.2e-08         2.8e-06
    1e-34       2.5e-07         2.8e-05
    1e-35       2.4e-06         4.4e-04
    1e-36       2.2e-05         1.8e-03
    1e-37       2.3e-04         2.4e-02

`tiny_limit(s)` = 4e-6 + 4 x the flushed figure at s: 4e-6 is what tests/test_gpu_conv.py holds these kernels to on O(1) data, the
flushed model is the weaker of the two possible hardware behaviours (a right kernel passes whichever holds), and 4 is the factor of
tests/optim_ref.py for fp32 accumulation order and contraction.  Nothing here is taken from what the kernels give.
"""
import numpy as np
import torch

BF16_MAX = float(np.array(0x7F7F0000, dtype=np.uint32).view(np.float32))       # 3.3895e38
FLT_MAX = float(np.finfo(np.float32).max)
H_OVERFLOWS = float(np.array(0x7F7F8000, dtype=np.uint32).view(np.float32))    # the first finite value whose bf16 rounding is Inf
H_LAST = float(np.array(0x7F7F7FFF, dtype=np.uint32).view(np.float32))         # the last that rounds to bf16-max
PARTNER_SCALE = 2.0 ** -12                                                       # partner operand of a huge-finite element
MIN_NORMAL = 2.0 ** -126
CLEAN = 0.5

NONFINITE_KINDS = ("pinf", "ninf", "nan", "pinf_ninf", "inf_x_zero", "inf_x_one")
HUGE_KINDS = ("flt_max", "neg_flt_max", "h_overflows", "h_last")
KINDS = NONFINITE_KINDS + HUGE_KINDS
_VALUE = {"pinf": float("inf"), "ninf": float("-inf"), "nan": float("nan"), "pinf_ninf": float("inf"), "inf_x_zero": float("inf"),
          "inf_x_one": float("-inf"), "flt_max": FLT_MAX, "neg_flt_max": -FLT_MAX, "h_overflows": H_OVERFLOWS, "h_last": -H_LAST}
MISTAKES = ("inf_to_finite", "poison_leaks", "drop_l_plane")
TINY_SCALES = (1e-20, 1e-30, 1e-32, 1e-33, 1e-35, 1e-37)
BASE_TOL = 4e-6
# A second, sharper bound for the k = 48 GEMM forms: rms error over rms reference.  The maximum-norm bound of 4e-6 is 16 x what an fp32 dot
# product of 48 terms needs, so a split that drops its l plane (16 of 24 bits: 3.4e-6 rms, 3.5 - 4.0e-6 maximum) can slip under it; in rms it
# is 27 x the fp32 figure.  RMS_MEASURED is torch's own fp32 bmm against float64 on the GEMM shape (CPU; the CPU test repeats it), the limit
# 4 x that, the factor of tests/optim_ref.py.
RMS_MEASURED = 1.26e-7
RMS_TOL = 4 * RMS_MEASURED


def rms_tol(k):
    """the rms bound at a contraction of k terms: RMS_TOL at k <= 48; beyond, the rounding errors of an fp32 accumulation add like a random
    walk over partial sums that grow like sqrt(i), so the error relative to the result grows like sqrt(k) (1.6e-6 at k = 512: still half of
    what a dropped l plane gives, which does not depend on k)"""
    return RMS_TOL * max(1.0, (k / 48.0) ** 0.5)


# max |err| / max |ref| of the restatement, A scaled by s: {s: (planes kept, planes flushed)}
MEASURED = {1.0: (7.8e-9, 7.8e-9), 1e-20: (6.7e-9, 6.7e-9), 1e-30: (7.1e-9, 7.1e-9), 1e-32: (7.2e-9, 3.3e-7), 1e-33: (2.2e-8, 2.8e-6),
            1e-34: (2.5e-7, 2.8e-5), 1e-35: (2.4e-6, 4.4e-4), 1e-36: (2.2e-5, 1.8e-3), 1e-37: (2.3e-4, 2.4e-2)}


# ---------------------------------------------------------------------------------------------------------------- float64 reference
def mm64(a, b):
    """a [..., r, k] x b [..., k, n] in float64 by elementwise products and a sum: no BLAS, so Inf x 0 = NaN and NaN are carried the
    IEEE way whatever library torch was built with."""
    a, b = a.double(), b.double()
    r = a.shape[-2]
    step = max(1, (1 << 22) // max(1, a.shape[-1] * b.shape[-1]))
    out = [(a[..., i:i + step, :, None] * b[..., None, :, :]).sum(-2) for i in range(0, r, step)]
    return torch.cat(out, -2)


def conv3_ref(x, w, dil=1):
    """3x3 'same' convolution, x NHWC, w HWIO -> float64 NHWC."""
    n, h, wd, ci = x.shape
    xp = torch.zeros(n, h + 2 * dil, wd + 2 * dil, ci, dtype=torch.float64)
    xp[:, dil:dil + h, dil:dil + wd] = x.double()
    y = torch.zeros(n, h, wd, w.shape[3], dtype=torch.float64)
    for r in range(3):
        for s in range(3):
            y += mm64(xp[:, r * dil:r * dil + h, s * dil:s * dil + wd].reshape(1, -1, ci), w[r, s][None]).reshape(n, h, wd, -1)
    return y


def conv3_dgrad_ref(dy, w, dil=1):
    return conv3_ref(dy, w.flip(0, 1).transpose(2, 3), dil)


def conv3_wgrad_ref(x, dy, dil=1):
    n, h, wd, ci = x.shape
    xp = torch.zeros(n, h + 2 * dil, wd + 2 * dil, ci, dtype=torch.float64)
    xp[:, dil:dil + h, dil:dil + wd] = x.double()
    d = dy.double().reshape(1, -1, dy.shape[3])
    return torch.stack([torch.stack([mm64(xp[:, r * dil:r * dil + h, s * dil:s * dil + wd].reshape(1, -1, ci).transpose(1, 2), d)[0]
                                     for s in range(3)]) for r in range(3)])


def convt_ref(x, w):
    """ConvTranspose2d(k2, s2): x [n, h, w, ci], w [2, 2, ci, co] -> [n, 2h, 2w, co] float64."""
    n, h, wd, ci = x.shape
    y = torch.zeros(n, 2 * h, 2 * wd, w.shape[3], dtype=torch.float64)
    for a in range(2):
        for b in range(2):
            y[:, a::2, b::2] = mm64(x.reshape(1, -1, ci), w[a, b][None]).reshape(n, h, wd, -1)
    return y


def convt_dgrad_ref(dy, w):
    n, h2, w2, co = dy.shape
    dx = torch.zeros(n, h2 // 2, w2 // 2, w.shape[2], dtype=torch.float64)
    for a in range(2):
        for b in range(2):
            dx += mm64(dy[:, a::2, b::2].reshape(1, -1, co), w[a, b].t()[None]).reshape(dx.shape)
    return dx


def convt_wgrad_ref(x, dy):
    ci, co = x.shape[3], dy.shape[3]
    return torch.stack([torch.stack([mm64(x.reshape(1, -1, ci).transpose(1, 2), dy[:, a::2, b::2].reshape(1, -1, co))[0] for b in range(2)])
                        for a in range(2)])


# ---------------------------------------------------------------------------------------------------------------- the restatement
def planes(x, variant="fixed", flush=False, mistake=None):
    """fp32 tensor -> (h, m, l) bf16 tensors."""
    assert variant in ("parent", "fixed") and mistake in (None,) + MISTAKES
    x = x.float()
    src = x.clamp(-BF16_MAX, BF16_MAX) if variant == "fixed" else x
    h = src.bfloat16()
    r = (src if mistake == "inf_to_finite" else x) - h.float()
    m = r.bfloat16()
    l = (r - m.float()).bfloat16()
    if mistake == "drop_l_plane":
        l = torch.zeros_like(l)
    if flush:
        h, m, l = (torch.where(p.float().abs() < MIN_NORMAL, torch.zeros_like(p), p) for p in (h, m, l))
    return h, m, l


def x3_matmul(a, b, variant="fixed", flush=False, mistake=None, variant_b=None):
    """[..., r, k] x [..., k, n] as the kernels form it (X3_MMA: l h, m m, h l, m h, h m, h h), float64 sums -> float64.
    variant_b: the split of B where it differs from A's (a packer and a kernel that split differently)."""
    ah, am, al = planes(a, variant, flush, mistake)
    bh, bm, bl = planes(b, variant_b or variant, flush, mistake)
    acc = None
    for p, q in ((al, bh), (am, bm), (ah, bl), (am, bh), (ah, bm), (ah, bh)):
        t = mm64(p, q)
        acc = t if acc is None else acc + t
    out = acc
    if mistake == "poison_leaks":
        out[..., out.shape[-2] // 2, :] = float("nan")
    return out


# ---------------------------------------------------------------------------------------------------------------- operand builders
def gaussian(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def plant(t, kind, where, axis):
    """-> (copy of t with the kind's element at every index of `where`, the same copy with CLEAN there instead).  axis: the contraction
    axis of t; "pinf_ninf" puts -Inf at the next index along it (wrapping), in the same dot products."""
    edge, clean = t.clone(), t.clone()
    for idx in where:
        idx = tuple(idx)
        spots = [(idx, _VALUE[kind])]
        if kind == "pinf_ninf":
            nxt = list(idx)
            nxt[axis] = (idx[axis] + 1) % t.shape[axis]
            spots.append((tuple(nxt), float("-inf")))
        for i, v in spots:
            edge[i] = v
            clean[i] = CLEAN
    return edge, clean


def partner(p, kind, kpos, axis):
    """The other operand of a run of `kind`: scaled by 2^-12 for the huge-finite kinds (every float64 partial sum then stays below
    2^126 with one huge element per dot product), exactly 0 / exactly 1.0 at the contraction indices `kpos` for the two Inf-against kinds."""
    p = p.clone()
    if kind in HUGE_KINDS:
        p *= PARTNER_SCALE
    if kind in ("inf_x_zero", "inf_x_one"):
        for k in kpos:
            p.select(axis, k).fill_(0.0 if kind == "inf_x_zero" else 1.0)
    return p


# GEMM edge set: B = 2, rows 130 (row 127 | 128, ragged 129), k 48 (k-octets 7 | 8, k-step 15 | 16, first / last), n 36 (31 | 32, ragged 35).
# One element per row (A side) / per column (B side): one huge element per dot product.  Batch 1 carries none.
GEMM_SHAPE = (2, 130, 48, 36)
A_SPOTS = ((0, 0, 0), (0, 127, 7), (0, 128, 8), (0, 129, 47), (0, 5, 15), (0, 64, 16))          # (batch, row, k)
B_SPOTS = ((0, 0, 0), (0, 7, 31), (0, 8, 32), (0, 47, 35), (0, 15, 5), (0, 16, 33))             # (batch, k, column)
# TN edge set: C[k][n] = sum over 144 rows (three splits of 48) of A[row][k] B[row][n]
TN_SHAPE = (2, 144, 48, 36)
TN_A_SPOTS = ((0, 0, 0), (0, 7, 31), (0, 8, 32), (0, 47, 47), (0, 48, 5), (0, 143, 33), (0, 15, 7), (0, 16, 8), (0, 95, 15), (0, 96, 16))   # (batch, row, k)
TN_B_SPOTS = ((0, 0, 0), (0, 7, 31), (0, 8, 32), (0, 47, 35), (0, 48, 5), (0, 143, 33), (0, 15, 7), (0, 16, 8), (0, 95, 15), (0, 96, 16))   # (batch, row, n)


def gemm_edge_set(kind, side, seed=5):
    """-> dict(a, b, a_clean, b_clean, touched [B, rows, n] bool) for C = A . B with the kind's elements planted in `side`."""
    B, rows, k, n = GEMM_SHAPE
    a, b = gaussian((B, rows, k), seed), gaussian((B, k, n), seed + 1)
    touched = torch.zeros(B, rows, n, dtype=torch.bool)
    if side == "a":
        a, a_clean = plant(a, kind, A_SPOTS, 2)
        kpos = sorted({s[2] for s in A_SPOTS})
        b = b_clean = partner(b, kind, kpos, 1)
        for z, r, _ in A_SPOTS:
            touched[z, r] = True
    else:
        b, b_clean = plant(b, kind, B_SPOTS, 1)
        kpos = sorted({s[1] for s in B_SPOTS})
        a = a_clean = partner(a, kind, kpos, 2)
        for z, _, c in B_SPOTS:
            touched[z, :, c] = True
    return dict(a=a, b=b, a_clean=a_clean, b_clean=b_clean, touched=touched)


def tn_edge_set(kind, side, seed=9):
    """-> dict(a, b, a_clean, b_clean, touched [splits, B, k, n]) for the per-split products C[s] = A[rows of s]^T . B[rows of s]."""
    B, rows, k, n = TN_SHAPE
    a, b = gaussian((B, rows, k), seed), gaussian((B, rows, n), seed + 1)
    touched = torch.zeros(3, B, k, n, dtype=torch.bool)
    spots = TN_A_SPOTS if side == "a" else TN_B_SPOTS
    rpos = sorted({s[1] for s in spots})
    if side == "a":
        a, a_clean = plant(a, kind, spots, 1)
        b = b_clean = partner(b, kind, rpos, 1)
    else:
        b, b_clean = plant(b, kind, spots, 1)
        a = a_clean = partner(a, kind, rpos, 1)
    for z, r, c in spots:
        for rr in ((r, (r + 1) % rows) if kind == "pinf_ninf" else (r,)):
            if side == "a":
                touched[rr // 48, z, c] = True
            else:
                touched[rr // 48, z, :, c] = True
    return dict(a=a, b=b, a_clean=a_clean, b_clean=b_clean, touched=touched)


def tn_split_ref(a, b, mm=mm64):
    """[3 splits, B, k, n]: the product of each 48-row split."""
    return torch.stack([mm(a[:, s * 48:(s + 1) * 48].transpose(1, 2), b[:, s * 48:(s + 1) * 48]) for s in range(3)])


def wino_touched(nhw, m, dil, pixels, adjoint=False):
    """[n, h, w] bool: the outputs of a Winograd F(m x m, 3x3) convolution whose computation reads one of `pixels` (image, row, column).
    Forward form: the m x m outputs of every tile whose (m + 2)^2 input window, rows m t - 1 .. m t + m, contains the pixel.  adjoint
    (the F(4x4) data gradient as the adjoint of the forward algorithm): the (m + 2)^2 window of the one tile that holds the pixel.
    dil > 1: the same inside the pixel's own sub-image (row % dil, column % dil)."""
    n, h, w = nhw
    mask = torch.zeros(n, h, w, dtype=torch.bool)

    def span(p, size):      # rows (of the sub-image) touched by sub-image row p
        if adjoint:
            t = p // m
            return range(max(0, m * t - 1), min(size, m * t + m + 1))
        return [q for t in range(size // m) if m * t - 1 <= p <= m * t + m for q in range(m * t, m * t + m)]
    for img, i, j in pixels:
        for q in span(i // dil, h // dil):
            for r in span(j // dil, w // dil):
                mask[img, q * dil + i % dil, r * dil + j % dil] = True
    return mask


# ---------------------------------------------------------------------------------------------------------------- comparisons
def _bits(t):
    return t.detach().cpu().float().contiguous().view(torch.int32)


def _rms_ratio(err, ref):
    return float(err.double().pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt())


def check_finite_contract(got, ref64, touched_mask, clean=None, tol=BASE_TOL, strict_inside=True, what="", rms_tol=None):
    """C1, C2 and C3.  got: the run with the edge elements (fp32), clean: the run with them replaced by 0.5, ref64: the float64 reference of
    the edge run, touched_mask: the outputs whose computation reads an edge element.  strict_inside=False (Winograd tiles around a
    NON-finite element): inside the mask a finite reference may meet a non-finite output."""
    got = got.detach().cpu().float()
    ref32 = ref64.float()                                   # the class of an output: that of the reference rounded to fp32
    mask = touched_mask.expand_as(got)
    ref_bad, got_bad = ~torch.isfinite(ref32), ~torch.isfinite(got)
    # coverage: the reference alone is non-finite nowhere outside the mask (the mask names every output that reads an edge element)
    assert not bool((ref_bad & ~mask).any()), f"{what}: the reference is non-finite at {int((ref_bad & ~mask).sum())} outputs outside the touched mask"
    # C3
    leak = got_bad & ~mask
    assert not bool(leak.any()), f"{what}: C3, {int(leak.sum())} non-finite outputs outside the touched mask"
    if clean is not None:
        diff = (_bits(got) != _bits(clean)) & ~mask
        assert not bool(diff.any()), f"{what}: C3, {int(diff.sum())} untouched outputs differ from the clean run"
    # C2
    lost = ref_bad & ~got_bad
    assert not bool(lost.any()), f"{what}: C2, {int(lost.sum())} outputs finite where the reference is not"
    # C1
    extra = got_bad & ~ref_bad
    if not strict_inside:
        extra = extra & ~mask
    assert not bool(extra.any()), f"{what}: C1, {int(extra.sum())} outputs non-finite where the reference is finite"
    worst = 0.0
    for region in (mask, ~mask):
        sel = region & ~ref_bad & ~got_bad
        if bool(sel.any()):
            r = ref64[sel]
            err = float((got[sel].double() - r).abs().max() / r.abs().max())
            worst = max(worst, err)
            where = "inside" if region is mask else "outside"
            assert err <= tol, f"{what}: C1, error {err:.3e} of scale (limit {tol:.1e}) {where} the touched mask"
            if rms_tol is not None:
                rms = _rms_ratio(got[sel].double() - r, r)
                assert rms <= rms_tol, f"{what}: C1, rms error {rms:.3e} of the rms (limit {rms_tol:.1e}) {where} the touched mask"
    return worst


def tiny_limit(s):
    """C4 limit at operand magnitude s: 4e-6 + 4 x the flushed-planes figure (that of >= 1e-30 above the table)."""
    key = min((k for k in MEASURED if k >= s * 0.999), default=1.0) if s < 1e-30 else 1e-30
    return BASE_TOL + 4.0 * MEASURED[key][1]


def check_tiny(got, ref64, s, what="", rms_tol=None):
    """C4: finite, and max |err| / max |ref| within tiny_limit(s).  s = None: fp32-denormal operands - finite and |err| <= max |ref|.
    rms_tol (the k = 48 GEMM forms: RMS_TOL): rms error / rms reference within rms_tol + 4 x the flushed figure as well."""
    got = got.detach().cpu().double()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output from tiny finite operands"
    err = float((got - ref64).abs().max() / ref64.abs().max())
    lim = 1.0 if s is None else tiny_limit(s)
    assert err <= lim, f"{what}: s = {s}: error {err:.3e} of scale, limit {lim:.3e}"
    if rms_tol is not None and s is not None:
        rms, rlim = _rms_ratio(got - ref64, ref64), rms_tol + (lim - BASE_TOL)
        assert rms <= rlim, f"{what}: s = {s}: rms error {rms:.3e} of the rms, limit {rlim:.3e}"
    return err


def measure(scales=tuple(MEASURED)):
    """{s: (kept, flushed)}: max |err| / max |ref| of the fixed restatement on a 130 x 48 x 36 product with A scaled by s."""
    a, b = gaussian((130, 48), 21), gaussian((48, 36), 22)
    out = {}
    for s in scales:
        a_s = (a * s).float()
        ref = mm64(a_s, b)
        out[s] = tuple(float((x3_matmul(a_s, b, "fixed", flush).double() - ref).abs().max() / ref.abs().max()) for flush in (False, True))
    return out


if __name__ == "__main__":
    for s, (kept, flushed) in measure().items():
        print(f"    {s:.0e}       {kept:.1e}         {flushed:.1e}")
