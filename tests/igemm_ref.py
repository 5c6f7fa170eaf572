"""Float64 references for the implicit-GEMM convolutions and the plain GEMMs of csrc/conv_igemm.hip and csrc/gemm.hip, on NHWC arrays,
written as loops over the filter taps with one matrix product per tap (no torch.nn.functional, nothing of the package).

Every public function returns (result, magnitude): the magnitude is the same operation on |x|, |w|, |bias|, |old|, i.e. the sum of the
absolute values of the terms of each output element.  bound(nterms, mag) = gamma(nterms) * mag, gamma(n) = n u / (1 - n u), u = 2^-24,
is the componentwise bound of a sum of nterms fp32 products accumulated in fp32 IN ANY ORDER (Higham, Accuracy and Stability of
Numerical Algorithms, section 3.1); nterms is the padded contraction the kernel runs: taps * ceil16(K) + 2 for a forward / data gradient
(bias and `+=` once each), pixels + splits for a weight gradient.  Nothing is tuned.

The case tables of tests/test_gpu_igemm_variants.py live here too, so that tests/test_igemm_ref_cpu.py can show on the CPU, at exactly
those shapes, that the references are torch's float64 operations, that a correct fp32 implementation stays inside the bound and that a
dropped tap, a dropped channel chunk, a shifted source or a misplaced output row does not.

Layouts (csrc/conv_igemm.hip): activations [n, h, w, c]; weights [kh, kw, c_in, c_out] of the forward operation.
"""
from types import SimpleNamespace as NS

import torch

U = 2.0 ** -24
F64 = torch.float64

FWD, DGRAD, CONVT_FWD, CONVT_DGRAD, DGRAD_T, CONVT_DGRAD_T = range(6)      # include/runet_hip.h


def ceil16(k):
    return (k + 15) // 16 * 16


def gamma(nterms):
    return nterms * U / (1.0 - nterms * U)


def bound(nterms, mag):
    return gamma(nterms) * mag


def out_size(h, k, stride, pad, dil):
    return (h + 2 * pad - dil * (k - 1) - 1) // stride + 1


# ------------------------------------------------------------------------------------------------ plain operations (no magnitudes)
def _conv(x, w, stride=1, pad=0, dil=1):
    """y[n, i, j, :] = sum_{r, s} x[n, i stride - pad + r dil, j stride - pad + s dil, :cin_w] . w[r, s]"""
    n, h, wd, _ = x.shape
    kh, kw, ci, co = w.shape
    ho, wo = out_size(h, kh, stride, pad, dil), out_size(wd, kw, stride, pad, dil)
    xp = x.new_zeros(n, h + 2 * pad, wd + 2 * pad, ci)
    xp[:, pad:pad + h, pad:pad + wd] = x[..., :ci]
    y = x.new_zeros(n, ho, wo, co)
    for r in range(kh):
        for s in range(kw):
            y += xp[:, r * dil:r * dil + (ho - 1) * stride + 1:stride, s * dil:s * dil + (wo - 1) * stride + 1:stride] @ w[r, s]
    return y


def _conv_dgrad(dy, w, h, wd, stride=1, pad=0, dil=1):
    """dx [n, h, wd, cin] of _conv for the forward weight w [kh, kw, cin, cout]; dy [n, ho, wo, cout].  Rows / columns of the padded input that
    no window reaches (strided convolutions) stay zero."""
    n, ho, wo, _ = dy.shape
    kh, kw, ci, co = w.shape
    hp, wp = max(h + 2 * pad, (ho - 1) * stride + dil * (kh - 1) + 1), max(wd + 2 * pad, (wo - 1) * stride + dil * (kw - 1) + 1)
    dxp = dy.new_zeros(n, hp, wp, ci)
    for r in range(kh):
        for s in range(kw):
            dxp[:, r * dil:r * dil + (ho - 1) * stride + 1:stride, s * dil:s * dil + (wo - 1) * stride + 1:stride] += dy @ w[r, s].T
    return dxp[:, pad:pad + h, pad:pad + wd].clone()


def _conv_wgrad(x, dy, kh, kw, cin_w, stride=1, pad=0, dil=1):
    """dw[r, s, ci, co] = sum over the output pixels of x[window pixel (r, s), ci] dy[pixel, co], ci < cin_w"""
    n, h, wd, _ = x.shape
    _, ho, wo, co = dy.shape
    xp = x.new_zeros(n, h + 2 * pad, wd + 2 * pad, cin_w)
    xp[:, pad:pad + h, pad:pad + wd] = x[..., :cin_w]
    dw = x.new_zeros(kh, kw, cin_w, co)
    g = dy.reshape(-1, co)
    for r in range(kh):
        for s in range(kw):
            a = xp[:, r * dil:r * dil + (ho - 1) * stride + 1:stride, s * dil:s * dil + (wo - 1) * stride + 1:stride]
            dw[r, s] = a.reshape(-1, cin_w).T @ g
    return dw


def _swap(w):
    return w.transpose(2, 3)


def _plus(y, bias, old):
    if bias is not None:
        y = y + bias
    if old is not None:
        y = y + old
    return y


def _mag(fn, tensors, **kw):
    """(fn(tensors), fn(|tensors|)): every operation here is a sum of products of its tensor arguments"""
    return fn(*tensors, **kw), fn(*[None if t is None else t.abs() for t in tensors], **kw)


# ------------------------------------------------------------------------------------------------ public: (result, magnitude)
def conv(x, w, bias=None, stride=1, pad=0, dil=1, old=None):
    """Conv2d: x [n, h, w, cin >= cin_w], w [kh, kw, cin_w, cout]"""
    return _mag(lambda x, w, b, o: _plus(_conv(x, w, stride, pad, dil), b, o), (x, w, bias, old))


def conv_dgrad(dy, w, h, wd, bias=None, stride=1, pad=0, dil=1, old=None):
    """data gradient of conv: dy [n, ho, wo, cout], w [kh, kw, cin, cout] -> [n, h, wd, cin]"""
    return _mag(lambda dy, w, b, o: _plus(_conv_dgrad(dy, w, h, wd, stride, pad, dil), b, o), (dy, w, bias, old))


def convt(x, w, bias=None, k=2, stride=2, pad=0, old=None):
    """ConvTranspose2d(k, stride, pad) (k2-s2 and k4-s2-p1 here): x [n, h, w, cin], w [k, k, cin, cout] -> [n, (h-1) s - 2 p + k, .., cout]:
    the data gradient of the convolution with the weight's channel axes swapped"""
    n, h, wd, _ = x.shape
    ho, wo = (h - 1) * stride - 2 * pad + k, (wd - 1) * stride - 2 * pad + k
    return _mag(lambda x, w, b, o: _plus(_conv_dgrad(x, _swap(w), ho, wo, stride, pad, 1), b, o), (x, w, bias, old))


def convt_dgrad(dy, w, bias=None, k=2, stride=2, pad=0, old=None):
    """data gradient of convt: dy [n, ho, wo, cout], w [k, k, cin, cout] -> [n, h, w, cin]"""
    return _mag(lambda dy, w, b, o: _plus(_conv(dy, _swap(w), stride, pad, 1), b, o), (dy, w, bias, old))


def gemm(a, b):
    """C[z] = A[z] . B[z]"""
    return _mag(lambda a, b: a @ b, (a, b))


def gemm_tn_split(a, b, rows_per_split):
    """C[split][z] = A[z][rows of the split]^T . B[z][rows of the split]"""
    rows = a.shape[1]
    return _mag(lambda a, b: torch.stack([a[:, r:r + rows_per_split].transpose(1, 2) @ b[:, r:r + rows_per_split]
                                          for r in range(0, rows, rows_per_split)]), (a, b))


def conv_wgrad(x, dy, kh, kw, cin_w=None, stride=1, pad=0, dil=1):
    """weight gradient of conv, [kh, kw, cin_w, cout]; cin_w < cin: the channels of x beyond cin_w have no weight rows"""
    cin_w = x.shape[-1] if cin_w is None else cin_w
    return _mag(lambda x, dy: _conv_wgrad(x, dy, kh, kw, cin_w, stride, pad, dil), (x, dy))


def convt2_wgrad(x, dy):
    """weight gradient of the k2-s2 transposed convolution: dw[r, s] = sum_p x[p]^T dy[2 p + (r, s)], x [n, h, w, cin], dy [n, 2h, 2w, cout]"""
    ci, co = x.shape[-1], dy.shape[-1]
    return _mag(lambda x, dy: torch.stack([torch.stack([x.reshape(-1, ci).T @ dy[:, r::2, s::2].reshape(-1, co) for s in range(2)])
                                           for r in range(2)]), (x, dy))


# ------------------------------------------------------------------------------------------------ inputs
def randn(shape, seed, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32) * std


# ------------------------------------------------------------------------------------------------ the cases
# An "op" case names one forward / data-gradient problem in the calling convention of the C ABI: `cin` channels are READ from the source,
# `cout` channels are WRITTEN.  kind: conv | conv_dgrad | convt2 | convt2_dgrad | gconv | gconv_dgrad | convt4 | convt4_dgrad.
# (h, w) is the SOURCE image except for the data gradients of strided convolutions, where (hin, win) is the gradient's (destination) image.
def _op(kind, n, h, w, cin, cout, k=1, dil=1, stride=1, pad=None, cin_w=None, tag=""):
    pad = dil * (k // 2) if pad is None else pad
    c = NS(kind=kind, n=n, h=h, w=w, cin=cin, cout=cout, k=k, dil=dil, stride=stride, pad=pad, cin_w=cin if cin_w is None else cin_w)
    c.id = f"{kind}-{n}x{h}x{w}-c{cin}" + (f"w{cin_w}" if cin_w else "") + f"-{cout}-k{k}d{dil}s{stride}p{pad}{tag}"
    return c


def igemm_cases():
    """runet_conv_igemm (section a).  P = 297 = 3 x 9 x 11 is > 256 and ragged against 64 / 128 / 256; cin = 20 pads to 32 (general loader, Kx < K
    tail); cout = 36 / 68 / 132 are ragged against 32 / 64 / 128; cout = 8 / 4 lie below every BN (with cin = 16: the Ncols - 4 / Ncols - 1 clamps)."""
    out = []
    for kind in ("conv", "conv_dgrad"):
        out += [_op(kind, 3, 9, 11, 20, 36, 3, 1),
                _op(kind, 2, 3, 5, 16, 68, 3, 2), _op(kind, 2, 3, 5, 16, 68, 3, 4),       # dilation > image: only the centre tap is inside
                _op(kind, 3, 9, 11, 48, 132, 1), _op(kind, 3, 9, 11, 20, 8, 1), _op(kind, 3, 9, 11, 20, 4, 1),
                # cin = 20 takes the general loader, whose columns are predicated; the clamps belong to the loader without predicates (cin % 16 == 0)
                _op(kind, 3, 9, 11, 16, 8, 1), _op(kind, 3, 9, 11, 16, 4, 1)]
    out += [_op("conv", 3, 9, 11, 8, 36, 3, 1, cin_w=5), _op("conv", 3, 9, 11, 4, 36, 1, 1, cin_w=3)]
    for kind in ("convt2", "convt2_dgrad"):
        out += [_op(kind, 3, 5, 7, 32, 36, 2, pad=0), _op(kind, 3, 5, 7, 20, 36, 2, pad=0)]
    return out


def general_cases():
    """runet_conv2d_general and runet_convt4_igemm (section b); the data gradients are given by the geometry of their forward convolution,
    (h, w) = the forward input = the gradient written.  7 x 7 x 12 = 588 and 16 x 32 = 512 products keep the bound below one product."""
    out = []
    for kind in ("gconv", "gconv_dgrad"):
        out += [_op(kind, 3, 13, 10, 12, 36, 7, 1, 2, 3), _op(kind, 3, 9, 11, 20, 36, 3, 1, 2, 1), _op(kind, 3, 9, 11, 20, 36, 3, 6, 1, 6)]
    for s in (2, 4, 8):
        for cin in (16, 20):
            out.append(_op("gconv_dgrad", 3, 3 * s, 5 * s, cin, 36, s, 1, s, 0, tag="-live"))
    for kind in ("convt4", "convt4_dgrad"):
        out += [_op(kind, 3, 5, 7, 20, 36, 4, 1, 2, 1), _op(kind, 3, 5, 7, 32, 36, 4, 1, 2, 1)]
    return out


def op_problem(c, seed=0):
    """-> NS(x, w, bias, old: float32 tensors in the ABI's layouts; src_hw, dst_hw; ref(bias, old) -> (float64 result, magnitude); nterms)"""
    g = lambda shape, i, std=1.0: randn(shape, 1000 * seed + 7 * (c.n + c.h + c.w + c.cin + c.cout + c.k + c.dil + c.stride) + i, std)
    k, n, h, w = c.k, c.n, c.h, c.w
    std = (1.0 / (c.cin * (k * k if c.kind in ("conv", "conv_dgrad", "gconv", "gconv_dgrad") else 1))) ** 0.5
    p = NS(case=c)
    if c.kind in ("conv", "gconv"):
        ho, wo = out_size(h, k, c.stride, c.pad, c.dil), out_size(w, k, c.stride, c.pad, c.dil)
        p.src_hw, p.dst_hw = (h, w), (ho, wo)
        p.w = g((k, k, c.cin_w, c.cout), 2, std)
        fn = lambda x, wt, b, o: conv(x, wt, b, c.stride, c.pad, c.dil, o)
        taps = k * k
    elif c.kind in ("conv_dgrad", "gconv_dgrad"):        # source = dy [n, ho, wo, cin], destination = dx [n, h, w, cout]; w [k, k, cout, cin]
        ho, wo = out_size(h, k, c.stride, c.pad, c.dil), out_size(w, k, c.stride, c.pad, c.dil)
        p.src_hw, p.dst_hw = (ho, wo), (h, w)
        p.w = g((k, k, c.cout, c.cin), 2, std)
        fn = lambda x, wt, b, o: conv_dgrad(x, wt, h, w, b, c.stride, c.pad, c.dil, o)
        taps = 1 if c.id.endswith("-live") else k * k
    elif c.kind in ("convt2", "convt4"):
        p.src_hw, p.dst_hw = (h, w), (2 * h, 2 * w)
        p.w = g((k, k, c.cin, c.cout), 2, std)
        fn = lambda x, wt, b, o: convt(x, wt, b, k, 2, c.pad, o)
        taps = 1 if k == 2 else 4                          # per output parity class
    else:                                                   # convt2_dgrad / convt4_dgrad: source dy [n, 2h, 2w, cin]; w [k, k, cout, cin]
        p.src_hw, p.dst_hw = (2 * h, 2 * w), (h, w)
        p.w = g((k, k, c.cout, c.cin), 2, std)
        fn = lambda x, wt, b, o: convt_dgrad(x, wt, b, k, 2, c.pad, o)
        taps = k * k
    p.x = g((n,) + p.src_hw + (c.cin,), 1)
    p.bias = g((c.cout,), 3)
    p.old = g((n,) + p.dst_hw + (c.cout,), 4)
    p.nterms = taps * ceil16(c.cin) + 2
    p.fn = fn
    p.ref = lambda bias, old: fn(p.x.double(), p.w.double(), p.bias.double() if bias else None, p.old.double() if old else None)
    return p


def gemm_cases():
    """runet_gemm_batched (section c): one case per branch of the dispatch, `name` = what runet_gemm_batched_kernel_name must report"""
    ig, nn = "igemm_kernel<%s, false, %s>", "gemm_nn_kernel<16, %s>"
    mk = lambda batch, rows, k, n, name: NS(batch=batch, rows=rows, k=k, n=n, name=name, id=f"{batch}x{rows}x{k}x{n}")
    return [mk(3, 130, 32, 64, ig % ("128, 64, 64, 32", "true")), mk(3, 130, 20, 64, ig % ("128, 64, 64, 32", "false")),      # few tiles, n % 64 == 0
            mk(3, 130, 32, 100, nn % "true"), mk(3, 130, 20, 100, nn % "false"),
            mk(36, 768, 32, 128, nn % "true"), mk(36, 700, 32, 128, nn % "true"),      # 216 tiles: balance 0.84, n % 64 == 0 -> not the 128 x 64 tile
            mk(3, 130, 32, 36, ig % ("64, 64, 32, 32", "true")), mk(3, 130, 20, 36, ig % ("64, 64, 32, 32", "false")),
            mk(3, 130, 32, 8, ig % ("128, 32, 32, 32", "true")), mk(3, 130, 20, 8, ig % ("128, 32, 32, 32", "false")),
            mk(32, 1000, 20, 36, ig % ("128, 64, 64, 32", "false"))]                   # >= 256 tiles of 128 x 64 at n < 96


TN_KN = (20, 36, 68, 132)
TN_ROWS = (80, 77)            # rows_per_split 32 -> splits of 32, 32 and 16 / 13 rows; 80: every split whole 16-row tiles (FAST loader)
TN_RPS = 32
TN_BATCH = 3


def wgrad_cases():
    """runet_conv_wgrad (section e), one case per route.  slabs: the split-K partial sums the route makes with the workspace it asks for - the
    tile kernels one per tile (3 x 3 x 2 tiles of 4 x 16 pixels; ceil(297 / 64) = 5 tiles of 64 pixels), the generic kernel two splits of 160
    and 137 pixels (at least 256 pixels per split), the direct GEMMs and the transposed tile plan (its splits divided by the 4 taps) one."""
    mk = lambda route, slabs, n, h, w, cin, cin_w, cout, k, dil=1, tr=0: NS(route=route, slabs=slabs, n=n, h=h, w=w, cin=cin, cin_w=cin_w, cout=cout, k=k,
                                                                            dil=dil, tr=tr, id=f"{route}-{n}x{h}x{w}-{cin}w{cin_w}-{cout}-k{k}d{dil}")
    out = [mk("tile3", 18, 3, 9, 19, 20, 20, 36, 3), mk("tile3", 18, 3, 9, 19, 8, 5, 36, 3)]
    out += [mk("tile1", 5, 3, 9, 11, ci, ci, co, 1) for ci, co in ((20, 36), (68, 36), (20, 132), (68, 132))]
    out += [mk("direct_f32", 1, 3, 9, 11, 132, 132, 132, 1), mk("direct_x3", 1, 2, 8, 19, 132, 132, 132, 1)]
    out += [mk("convt_tile", 1, 3, 5, 7, 68, 68, 36, 2, tr=1)]
    out += [mk("generic_small", 2, 3, 9, 11, 20, 20, 36, 3, 2), mk("generic_big", 2, 3, 9, 11, 68, 68, 132, 3, 2)]
    return out


def wgrad_problem(c):
    g = lambda shape, i: randn(shape, 31 * (c.n + c.h + c.w + c.cin + c.cout + c.k + c.dil) + i)
    p = NS(case=c, x=g((c.n, c.h, c.w, c.cin), 1))
    up = 2 if c.tr else 1
    p.dy = g((c.n, up * c.h, up * c.w, c.cout), 2)
    if c.tr:
        p.fn = lambda x, dy: convt2_wgrad(x, dy)
    else:
        p.fn = lambda x, dy: conv_wgrad(x, dy, c.k, c.k, c.cin_w, 1, c.dil * (c.k // 2), c.dil)
    p.ref = lambda: p.fn(p.x.double(), p.dy.double())
    p.pixels = c.n * c.h * c.w
    return p


def lowp_cases():
    """runet_conv_igemm_bf16 / _fp16 (section f): P = 297 (k2-s2: 3 x 5 x 7 sources), cin in {24, 64}, cout in {36, 68, 132}"""
    out = []
    for cin in (24, 64):
        for cout in (36, 68, 132):
            out += [_op("conv", 3, 9, 11, cin, cout, 1), _op("conv_dgrad", 3, 9, 11, cin, cout, 1),
                    _op("conv", 3, 9, 11, cin, cout, 3, 2), _op("conv_dgrad", 3, 9, 11, cin, cout, 3, 2),
                    _op("convt2", 3, 9, 11, cin, cout, 2, pad=0), _op("convt2_dgrad", 3, 9, 11, cin, cout, 2, pad=0)]
    return out


def lowp_c3_cases():
    """3 x 3, dilation 1 (the patch kernels LP_CONV3_KERNEL<8> / <16>): the last patch of 8 / 16 rows is ragged at h = 5, 17, 33"""
    return [_op(kind, 2, h, 19, 24, 36, 3, 1) for h in (5, 17, 33) for kind in ("conv", "conv_dgrad")]
