"""Bit fingerprints of the entry points whose results rest on a fixed summation order: the two-stage reductions (chunk partials, then the
ordered final pass sum_parts of csrc/runet_common.h), the gather adjoints of the bilinear resizes, every entry point of csrc/norm_act.hip
(BatchNorm statistics, apply and backward: Chan combines in chunk order, first-occurrence max / min, explicit FMAs) and every entry point of
csrc/attention.hip (the residual-block tail and the attention gate: chunk plans, 16-lane pixel sums, the ordered final passes; ATT_SHAPES
below), of csrc/conv_winograd.hip (the fp32 F(2x2) filter transform, convolution and weight gradient; WINO2_CASES) and of the GEMM layer
(the plain and split-operand GEMMs, the 1x1 / transposed split-operand convolutions, runet_conv_wgrad; GEMM_LAYER_CASES).  Every case fills seeded inputs, calls
the entry point once through the package's binding and prints one SHA-256 per output tensor (per case for attention.hip).  Two builds of the library compute the same
bits exactly when their printouts are equal line for line; RUNET_HIP_LIB selects the build (see _lib.py), one fresh process per build:

  RUNET_HIP_LIB=/path/to/other/librunet_hip.so python tools/abi_bits.py > a.txt
  python tools/abi_bits.py > b.txt && diff a.txt b.txt

The shapes are the smallest at which an order can go wrong: fewer partial rows than the final pass has part-lanes (16 or 8), more than
twice as many, a reduced width that is no multiple of the 16 / 32 outputs of a block; odd non-square and one-row maps for the resizes;
NA_SHAPES below for norm_act.hip.  New cases go at the end: the seeded generator is drawn from in case order.
"""
import hashlib
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import igemm_ref      # noqa: E402  (tests/: the GEMM-layer shapes are the ones its tests use)
importlib.import_module("eusipco-2026-robust-unet_amd")
ops = importlib.import_module("eusipco-2026-robust-unet_amd.ops")
L = importlib.import_module("eusipco-2026-robust-unet_amd._lib")
lib, check = L.lib, L.check
DEV = torch.device("cuda:0")
G = torch.Generator().manual_seed(20261018)


def rnd(*shape):
    return torch.randn(shape, generator=G).to(DEV)


def pos(*shape):
    return (torch.rand(shape, generator=G) + 0.5).to(DEV)


def out(*shape):
    return torch.zeros(shape, device=DEV)


def p(t):
    return t.data_ptr()


def ws(floats):
    assert floats > 0, floats
    return torch.zeros(floats, device=DEV)


def hr_head_bwd_reduce(n, h, w, c):
    dz, t, res = rnd(n, h, w), rnd(n, h, w, c), out(3 * c + 1)
    sc, sh, wt, mean, invstd = rnd(c), rnd(c), rnd(c), rnd(c), pos(c)
    k = ws(lib.runet_hr_head_bwd_workspace_floats(n, h, w, c))
    check(lib.runet_hr_head_bwd_reduce(p(dz), p(t), c, p(sc), p(sh), p(wt), p(mean), p(invstd), p(k), k.numel(), p(res), n, h, w, c, ops.stream()))
    return [res]


def bilinear_nhwc_bwd_sums(n, h, w, c, s):
    dy, x, g, sums = rnd(n, s * h, s * w, c), rnd(n, h, w, c), out(n, h, w, c), out(2 * c)
    mean, invstd = rnd(c), pos(c)
    k = ws(lib.runet_bilinear_nhwc_bwd_sums_workspace_floats(n, h, w, c))
    check(lib.runet_bilinear_nhwc_bwd_sums(p(dy), c, p(x), c, p(mean), p(invstd), p(g), c, p(k), k.numel(), p(sums), n, h, w, s, c, ops.stream()))
    return [g, sums]


def up2_sigmoid_bwd(n, h, w):
    dprob, prob, dz = rnd(n, 2 * h, 2 * w), torch.sigmoid(rnd(n, 2 * h, 2 * w)), out(n, h, w)
    check(lib.runet_up2_sigmoid_bwd(p(dprob), p(prob), p(dz), n, h, w, ops.stream()))
    return [dz]


def up_sigmoid_bwd(n, h, w, s):
    dprob, prob, dz = rnd(n, s * h, s * w), torch.sigmoid(rnd(n, s * h, s * w)), out(n, h, w)
    check(lib.runet_up_sigmoid_bwd(p(dprob), p(prob), p(dz), n, h, w, s, ops.stream()))
    return [dz]


def dw3_wgrad(n, h, w, c, stride):
    ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride
    x, dy, dw = rnd(n, h, w, c), rnd(n, ho, wo, c), out(9, c)
    k = ws(lib.runet_dw3_wgrad_workspace_floats(n, h, w, c, stride))
    check(lib.runet_dw3_wgrad(p(x), c, p(dy), c, p(k), k.numel(), p(dw), n, h, w, c, stride, ops.stream()))
    return [dw]


def dwconv3x3_gelu_bwd_wgrad(n, h, w, c, keep_z):
    x, wt, b, da, g, dwdb = rnd(n, h, w, c), rnd(9, c), rnd(c), rnd(n, h, w, c), out(n, h, w, c), out(10, c)
    z = rnd(n, h, w, c) if keep_z else None
    k = ws(lib.runet_dwconv3x3_gelu_bwd_workspace_floats(n, h, w, c))
    check(lib.runet_dwconv3x3_gelu_bwd_wgrad(p(x), c, p(wt), p(b), p(da), c, p(z) if keep_z else None, c, p(g), c, p(k), k.numel(), p(dwdb), n, h, w, c,
                                             ops.stream()))
    return [g, dwdb]


def dwsep_wgrad_pw(n, h, w, cin, cout, stride):
    ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride
    x, wd, dt, dwp = rnd(n, h, w, cin), rnd(9, cin), rnd(n, ho, wo, cout), out(cin, cout)
    k = ws(lib.runet_dwsep_wgrad_pw_workspace_floats(n, h, w, cin, cout, stride))
    check(lib.runet_dwsep_wgrad_pw(p(x), cin, p(wd), p(dt), cout, p(k), k.numel(), p(dwp), n, h, w, cin, cout, stride, ops.stream()))
    return [dwp]


def nchw_src(n, h, w):
    x = rnd(n, 3, h, w)
    return x, (p(x), *x.stride(), n, h, w)


def ms_stem_bwd_reduce(n, h, w):
    x, src = nchw_src(n, h, w)
    wts = [rnd(k * 3 * 16) for k in (1, 9, 25, 1)] + [rnd(16) for _ in range(4)]
    sc, sh, de, mean, invstd, sums = rnd(64), rnd(64), rnd(n, h, w, 64), rnd(64), pos(64), out(128)
    k = ws(lib.runet_ms_stem_workspace_floats(n, h, w))
    check(lib.runet_ms_stem_bwd_reduce(*src, *map(p, wts), p(sc), p(sh), p(de), 64, p(mean), p(invstd), p(k), k.numel(), p(sums), ops.stream()))
    return [sums]


def water_index_bwd(n, h, w):
    """runet_water_index_bwd_reduce, then runet_water_index_bwd_apply on the sums it left"""
    x, src = nchw_src(n, h, w)
    g, w1, b1, sc, sh, w2, b2, mean, invstd = rnd(n, h, w, 4), rnd(48), rnd(16), rnd(16), rnd(16), rnd(64), rnd(4), rnd(16), pos(16)
    red, app = out(100), out(64)
    k = ws(lib.runet_water_index_workspace_floats(n, h, w))
    coef = (p(g), 4, p(w1), p(b1), p(sc), p(sh), p(w2), p(b2), p(mean), p(invstd))
    check(lib.runet_water_index_bwd_reduce(*src, *coef, p(k), k.numel(), p(red), ops.stream()))
    check(lib.runet_water_index_bwd_apply(*src, *coef, p(red), 0, p(k), k.numel(), p(app), ops.stream()))
    return [red, app]


def pyramid_upsample_bwd(n, h, w, cq):
    dy, da = rnd(n, h, w, 4 * cq), out(n * 50, cq)
    check(lib.runet_pyramid_upsample_bwd(p(dy), 4 * cq, p(da), cq, n, h, w, cq, ops.stream()))
    return [da]


def bilinear_bwd(planes, h, w, ho, wo):
    dy, dx = rnd(planes, ho, wo), out(planes, h, w)
    check(lib.runet_bilinear_bwd(p(dy), p(dx), planes, h, w, ho, wo, ops.stream()))
    return [dx]


def bilinear_nhwc_bwd(n, h, w, ho, wo, c):
    dy, dx = rnd(n, ho, wo, c), out(n, h, w, c)
    check(lib.runet_bilinear_nhwc_bwd(p(dy), c, p(dx), c, n, h, w, ho, wo, c, ops.stream()))
    return [dx]


# ---- csrc/norm_act.hip.  A shape is (n, h, w, c, ld): an NHWC view of c channels with pixel stride ld.
NA_SHAPES = [
    (2, 5, 7, 1, 1),            # scalar path, 16-thread grouped row combine, fewer pixels than thread rows
    (2, 32, 32, 1, 1),          # scalar path, several chunks per image
    (2, 6, 10, 12, 16),         # 3 channel groups: 85 thread rows plus one idle thread, strided view, even sides for the pooled forms
    (3, 16, 16, 16, 16),        # the last width on the grouped combine (c * 16 == 256)
    (3, 16, 16, 32, 40),        # the first width on the general combine, strided
    (1, 4, 6, 1024, 1024),      # one thread row
    (16, 64, 64, 4, 4),         # 256 partial rows: the final_cw switch from 32 to 4
]
NA_POOLED = [s for s in NA_SHAPES if s[1] % 2 == 0 and s[2] % 2 == 0 and s[3] % 4 == 0]


def ties(*shape):
    """quantised so that equal values occur and the first-occurrence rule decides the max / min indices"""
    return (torch.round(2 * torch.randn(shape, generator=G)) / 2).to(DEV)


def drop_mask(n, c):
    return ((torch.rand((n, c), generator=G) > 0.5).float() * 2).to(DEV)


def red_ws(n, h, w, c):
    return ws(lib.runet_reduce_workspace_floats(n, h * w, c))


def chan_stats(n, h, w, c, ld, minmax):
    x, k = (ties if minmax else rnd)(n, h, w, ld), red_ws(n, h, w, c)
    f = [out(n, c) for _ in range(4)]
    i = [torch.zeros(n, c, dtype=torch.int32, device=DEV) for _ in range(2)]
    mm = [p(t) if minmax else None for t in f[2:] + i]
    check(lib.runet_chan_stats(p(x), ld, n, h * w, c, p(k), p(f[0]), p(f[1]), *mm, minmax, ops.stream()))
    return f + i if minmax else f[:2]


def bn_params(c):
    """gamma, beta, running mean, running variance, num_batches_tracked | scale, shift, saved mean, saved invstd"""
    return [rnd(c), rnd(c), rnd(c), pos(c), torch.zeros(1, dtype=torch.int64, device=DEV)], [out(c) for _ in range(4)]


def bn_stats(n, h, w, c, ld):
    x, k, (par, res) = rnd(n, h, w, ld), red_ws(n, h, w, c), bn_params(c)
    check(lib.runet_bn_stats(p(x), ld, n, h * w, c, p(k), *map(p, par), 0.1, 1e-5, *map(p, res), ops.stream()))
    return res + par[2:]


def bn_stats_finalize(nparts, c):
    part = torch.stack([torch.randint(1, 50, (nparts, c), generator=G).float(), torch.randn((nparts, c), generator=G),
                        torch.rand((nparts, c), generator=G) * 40], dim=2).contiguous().to(DEV)
    par, res = bn_params(c)
    check(lib.runet_bn_stats_finalize(p(part), nparts, c, *map(p, par), 0.1, 1e-5, *map(p, res), ops.stream()))
    return res + par[2:]


def bn_finalize(n, c, hw, training):
    mean_nc, m2_nc, (par, res) = rnd(n, c), pos(n, c), bn_params(c)
    check(lib.runet_bn_finalize(p(mean_nc), p(m2_nc), n, c, hw, *map(p, par), 0.1, 1e-5, training, *map(p, res), ops.stream()))
    return res + par[2:]


def bn_apply(n, h, w, c, ld, act, relu=1, mask=False):
    x, y, sc, sh = rnd(n, h, w, ld), out(n, h, w, ld), rnd(c), rnd(c)
    head = (p(x), ld, p(y), ld, n * h * w, h * w, c, p(sc), p(sh))
    if act == "relu":
        m = drop_mask(n, c) if mask else None
        check(lib.runet_bn_apply(*head, p(m) if mask else None, relu, ops.stream()))
    elif act == "leaky":
        check(lib.runet_bn_apply_leaky(*head, 0.1, ops.stream()))
    else:
        check(lib.runet_bn_apply_gelu(*head, ops.stream()))
    return [y]


def bn_bwd(n, h, w, c, ld, form, mask=False, m_total=0):
    """the reduce entry, then the apply entry on the sums it left.  form: the ReLU entries with the saved activation ("act"), with the
    decision recomputed from x ("shift") or without ReLU ("plain"); the "leaky" and "gelu" entries"""
    dy, x, dx, sums, k = rnd(n, h, w, ld), rnd(n, h, w, ld), out(n, h, w, ld), out(2 * c), red_ws(n, h, w, c)
    mean, invstd, sc, sh = rnd(c), pos(c), rnd(c), rnd(c)
    hw, pixels, st = h * w, n * h * w, ops.stream()
    if form in ("leaky", "gelu"):
        tail = (0.1,) if form == "leaky" else ()
        red, app = (lib.runet_bn_bwd_reduce_leaky, lib.runet_bn_bwd_apply_leaky) if form == "leaky" else (lib.runet_bn_bwd_reduce_gelu, lib.runet_bn_bwd_apply_gelu)
        check(red(p(dy), ld, p(x), ld, n, hw, c, p(mean), p(invstd), p(k), p(sums), p(sc), p(sh), *tail, st))
        check(app(p(dy), ld, p(x), ld, p(dx), ld, pixels, hw, c, p(mean), p(invstd), p(sc), p(sums), m_total, p(sh), *tail, st))
        return [sums, dx]
    act = torch.relu(rnd(n, h, w, ld)) if form == "act" else None
    m = drop_mask(n, c) if mask else None
    a = (p(act), ld) if form == "act" else (None, 0)
    rs, rh = (p(sc), p(sh)) if form == "shift" else (None, None)
    pm = p(m) if mask else None
    check(lib.runet_bn_bwd_reduce(p(dy), ld, p(x), ld, *a, n, hw, c, p(mean), p(invstd), pm, p(k), p(sums), rs, rh, st))
    check(lib.runet_bn_bwd_apply(p(dy), ld, p(x), ld, *a, p(dx), ld, pixels, hw, c, p(mean), p(invstd), p(sc), p(sums), pm, m_total, rh, st))
    return [sums, dx]


def bn_bwd_pooled(n, h, w, c, ld, leaky):
    """gradient at pooled resolution + the 2x2 max-pool's winner bytes (seeded values in 0..3)"""
    dpool, x, dx, sums, k = rnd(n, h // 2, w // 2, ld), rnd(n, h, w, ld), out(n, h, w, ld), out(2 * c), red_ws(n, h, w, c)
    idx = torch.randint(0, 4, (n, h // 2, w // 2, c), generator=G, dtype=torch.uint8).to(DEV)
    mean, invstd, sc, sh = rnd(c), pos(c), rnd(c), rnd(c)
    red, app = (lib.runet_bn_bwd_reduce_pooled_leaky, lib.runet_bn_bwd_apply_pooled_leaky) if leaky else (lib.runet_bn_bwd_reduce_pooled, lib.runet_bn_bwd_apply_pooled)
    tail = (0.1,) if leaky else ()
    check(red(p(dpool), ld, p(idx), p(x), ld, n, h, w, c, p(mean), p(invstd), p(k), p(sums), p(sc), p(sh), *tail, ops.stream()))
    check(app(p(dpool), ld, p(idx), p(x), ld, p(dx), ld, n, h, w, c, p(mean), p(invstd), p(sc), p(sums), 0, p(sh), *tail, ops.stream()))
    return [sums, dx]


def chan_sum(n, h, w, c, ld, accumulate):
    x, res, k = rnd(n, h, w, ld), rnd(c), red_ws(n, h, w, c)
    check(lib.runet_chan_sum(p(x), ld, n * h * w, c, p(k), p(res), accumulate, ops.stream()))
    return [res]


def wino_conv_x3(n, h, w, k, nn, bias, accumulate, ldx, ldy, dgrad, stats):
    """runet_wino_weights_x3, then runet_wino_conv_x3 or runet_wino_conv_x3_stats (csrc/conv_winograd_x3.hip): every bit of y rests on the
    order of the six products per chunk and of the two output-transform stages, the partials on the order of the Chan combines"""
    x, wt = rnd(n, h, w, ldx), rnd(3, 3, *((nn, k) if dgrad else (k, nn)))
    b = rnd(nn) if bias else None
    y = rnd(n, h, w, ldy) if accumulate else out(n, h, w, ldy)
    up = torch.empty(lib.runet_wino_x3_pack_elems(k, nn), device=DEV, dtype=torch.bfloat16)
    check(lib.runet_wino_weights_x3(p(wt), p(up), wt.shape[2], wt.shape[3], dgrad, ops.stream()))
    head = (p(x), ldx, p(up), p(b) if bias else None, p(y), ldy, n, h, w, k, nn, accumulate)
    if not stats:
        check(lib.runet_wino_conv_x3(*head, ops.stream()))
        return [y]
    part = out(lib.runet_wino_conv_x3_stats_parts(n, h, w), nn, 3)
    check(lib.runet_wino_conv_x3_stats(*head, p(part), ops.stream()))
    return [y, part]


# n, h, w, K, N, bias, accumulate, ldx, ldy, dgrad: one partial patch | one full patch at K = N = 64, with and without bias | a second output
# chunk of 6 channels | 18 patches (remainder group of the block remap), three K chunks, accumulate into a strided slice | data-gradient weights
WINO_X3_SHAPES = [(1, 6, 10, 16, 6, 1, 0, 16, 6, 0), (1, 8, 16, 64, 64, 1, 0, 64, 64, 0), (1, 8, 16, 64, 64, 0, 0, 64, 64, 0),
                  (2, 12, 20, 32, 70, 1, 0, 32, 70, 0), (3, 16, 48, 48, 128, 1, 1, 64, 160, 0), (1, 8, 16, 64, 64, 0, 0, 64, 64, 1)]

NORM_ACT_CASES = [
    *[(chan_stats, (*s, mm)) for s in NA_SHAPES for mm in (0, 1)],
    *[(bn_stats, s) for s in NA_SHAPES],
    # partials per thread of the one-channel block: none for most | 2 | 4
    (bn_stats_finalize, (5, 3)), (bn_stats_finalize, (300, 12)), (bn_stats_finalize, (1000, 1)),
    # one block of 128 channels, partly filled | two blocks
    *[(bn_finalize, (*s, tr)) for s in ((2, 12, 35), (16, 200, 4096)) for tr in (1, 0)],
    *[(bn_apply, (*s, "relu", relu, mask)) for s in NA_SHAPES for relu in (0, 1) for mask in (False, True)],
    *[(bn_bwd, (*s, form, mask)) for s in NA_SHAPES for form in ("act", "shift", "plain") for mask in (False, True)],
    *[(bn_bwd, (*s, "shift", True, 3 * s[0] * s[1] * s[2])) for s in NA_SHAPES],
    *[(bn_bwd_pooled, (*s, False)) for s in NA_POOLED],
    *[(fn, (*s, *a)) for s in NA_SHAPES for fn, a in ((bn_apply, ("leaky",)), (bn_bwd, ("leaky",)))],
    *[(bn_bwd_pooled, (*s, True)) for s in NA_POOLED],
    *[(fn, (*s, *a)) for s in NA_SHAPES for fn, a in ((bn_apply, ("gelu",)), (bn_bwd, ("gelu",)))],
    *[(chan_sum, (*s, acc)) for s in NA_SHAPES for acc in (0, 1)],
]


# ---- csrc/attention.hip.  (n, h, w, c): more than one chunk per image and partial 16 x 16 tiles | idle threads in a row group (12 channel
# groups) | one thread row, image smaller than the 7 x 7 window | C < 64 in the 16-lane kernels, Cr = 1 | four thread rows.  All sides even.
ATT_SHAPES = [(2, 20, 36, 64), (2, 8, 8, 48), (1, 2, 2, 1024), (3, 6, 10, 16), (1, 4, 4, 256)]


def ri(hi, *shape, dtype=torch.int32):
    return torch.randint(0, hi, shape, generator=G, dtype=dtype).to(DEV)


def tail_inputs(n, h, w, c):
    """t2, A, B, sa of the residual-block tail"""
    return rnd(n, h, w, c), rnd(n, c), rnd(n, c), torch.sigmoid(rnd(n, h, w))


def att_rb_out(n, h, w, c, bits, pool, affine, ex=1):
    t2, A, B, sa = tail_inputs(n, h, w, c)
    r, rs, rh, o = rnd(n, h, w, c), rnd(c), rnd(c), out(n, h, w, c)
    rb = torch.zeros((n * h * w, c // 4), dtype=torch.uint8, device=DEV)
    pooled, pidx = out(n, h // 2, w // 2, c), torch.zeros((n, h // 2, w // 2, c), dtype=torch.uint8, device=DEV)
    head = (p(t2), c, p(A), p(B), p(sa), p(r), c, p(rs) if affine else None, p(rh) if affine else None, p(o), c)
    if not ex:
        check(lib.runet_rb_out(*head, n * h * w, h * w, c, ops.stream()))
        return [o]
    check(lib.runet_rb_out_ex(*head, p(rb) if bits else None, p(pooled) if pool else None, c if pool else 0, p(pidx) if pool else None, n, h, w, c,
                              ops.stream()))
    return [o] + ([rb] if bits else []) + ([pooled, pidx] if pool else [])


def att_rb_bwd1(n, h, w, c, form, pool=0, bits=0):
    """form: "plain" runet_rb_bwd1 with `out`, "noact" the same with out NULL, "ex" runet_rb_bwd1_ex in its four template cases"""
    t2, A, B, sa = tail_inputs(n, h, w, c)
    dout, o, dv, dq = rnd(n, h, w, c), torch.relu(rnd(n, h, w, c)), out(n, h, w, c), out(n, h, w)
    dpool, pidx, rb = rnd(n, h // 2, w // 2, c), ri(4, n, h // 2, w // 2, c, dtype=torch.uint8), ri(16, n * h * w, c // 4, dtype=torch.uint8)
    tail = (p(t2), c, p(A), p(B), p(sa), p(dv), c, p(dq))
    if form == "ex":
        check(lib.runet_rb_bwd1_ex(p(dout), c, p(dpool) if pool else None, c if pool else 0, p(pidx) if pool else None, p(o), c, p(rb) if bits else None,
                                   *tail, n, h, w, c, ops.stream()))
    else:
        check(lib.runet_rb_bwd1(p(dout), c, p(o) if form == "plain" else None, c, *tail, n * h * w, h * w, c, ops.stream()))
    return [dv, dq]


def att_rb_bwd2(n, h, w, c, bn):
    dv, t2, sa, dsm, amax = rnd(n, h, w, c), rnd(n, h, w, c), torch.sigmoid(rnd(n, h, w)), rnd(n * h * w, 2), ri(c, n * h * w)
    sdu, sdut, sums_s, k = out(n, c), out(n, c), out(2 * c), ws(lib.runet_rb_bwd2_bn_workspace_floats(n, h * w, c))
    head = (p(dv), c, p(t2), c, p(sa), p(dsm), p(amax))
    if not bn:
        check(lib.runet_rb_bwd2(*head, n, h * w, c, p(k), p(sdu), p(sdut), ops.stream()))
        return [sdu, sdut]
    r, mean_s, invstd_s = rnd(n, h, w, c), rnd(c), pos(c)
    check(lib.runet_rb_bwd2_bn(*head, p(r), c, p(mean_s), p(invstd_s), n, h * w, c, p(k), k.numel(), p(sdu), p(sdut), p(sums_s), ops.stream()))
    return [sdu, sdut, sums_s]


def att_rb_bwd3(n, h, w, c, sc, m_total):
    dv, t2, sa, dsm, amax = rnd(n, h, w, c), rnd(n, h, w, c), torch.sigmoid(rnd(n, h, w)), rnd(n * h * w, 2), ri(c, n * h * w)
    ca, davg, dmx, idx = rnd(n, c), rnd(n, c), rnd(n, c), ri(h * w, n, c)
    mean2, invstd2, s2, sums2, dt2 = rnd(c), pos(c), rnd(c), rnd(2 * c), out(n, h, w, c)
    head = (p(dv), c, p(t2), c, p(sa), p(dsm), p(amax), p(ca), p(davg), p(dmx), p(idx), p(mean2), p(invstd2), p(s2), p(sums2), p(dt2), c)
    if not sc:
        check(lib.runet_rb_bwd3(*head, n * h * w, h * w, c, m_total, ops.stream()))
        return [dt2]
    r, mean_s, invstd_s, scale_s, sums_s = rnd(n, h, w, c), rnd(c), pos(c), rnd(c), rnd(2 * c)
    check(lib.runet_rb_bwd3_sc(*head, p(r), c, p(mean_s), p(invstd_s), p(scale_s), p(sums_s), m_total, n * h * w, h * w, c, m_total, ops.stream()))
    return [dt2, dv]


def att_sa(n, h, w, c):
    """runet_sa_reduce, runet_sa_conv7 on its map, runet_sa_conv7_bwd on both"""
    t2, A, B, _ = tail_inputs(n, h, w, c)
    P = n * h * w
    smap, amax, sa, wp = out(P, 2), torch.zeros(P, dtype=torch.int32, device=DEV), out(P), rnd(98)
    check(lib.runet_sa_reduce(p(t2), c, p(A), p(B), P, h * w, c, p(smap), p(amax), ops.stream()))
    check(lib.runet_sa_conv7(p(smap), p(wp), p(sa), n, h, w, ops.stream()))
    dq, dsm, dwp, k = rnd(P), out(P, 2), out(98), ws(lib.runet_sa_conv7_bwd_workspace_floats(n, h, w))
    check(lib.runet_sa_conv7_bwd(p(smap), p(dq), p(wp), p(dsm), p(dwp), p(k), n, h, w, ops.stream()))
    return [smap, amax, sa, dsm, dwp]


def att_ca(n, c, cr):
    """runet_ca_coeff, then runet_ca_bwd on what it saved"""
    mean_nc, max_nc, min_nc, imax, imin = rnd(n, c), rnd(n, c), rnd(n, c), ri(64, n, c), ri(64, n, c)
    s2, h2, w0p, w2p = rnd(c), rnd(c), rnd(c, cr), rnd(cr, c)
    A, B, ca, avg, mx, tval = (out(n, c) for _ in range(6))
    idx = torch.zeros((n, c), dtype=torch.int32, device=DEV)
    check(lib.runet_ca_coeff(p(mean_nc), p(max_nc), p(min_nc), p(imax), p(imin), p(s2), p(h2), p(w0p), p(w2p), n, c, cr, p(A), p(B), p(ca), p(avg),
                             p(mx), p(idx), p(tval), ops.stream()))
    sdu, sdut, mean2, invstd2 = rnd(n, c), rnd(n, c), rnd(c), pos(c)
    davg, dmx, sums2, dw0p, dw2p, k = out(n, c), out(n, c), out(2 * c), out(c, cr), out(cr, c), ws(lib.runet_ca_bwd_workspace_floats(n, c, cr))
    check(lib.runet_ca_bwd(p(sdu), p(sdut), p(s2), p(h2), p(ca), p(avg), p(mx), p(w0p), p(w2p), p(mean_nc), p(tval), p(mean2), p(invstd2), n, c, cr,
                           p(k), p(davg), p(dmx), p(sums2), p(dw0p), p(dw2p), ops.stream()))
    return [A, B, ca, avg, mx, idx, tval, davg, dmx, sums2, dw0p, dw2p]


def att_gate(P, f, ld):
    """runet_ag_psi, runet_ag_out, runet_ag_bwd1, runet_ag_bwd2 and runet_ag_bwd2_bn over P pixels of f channels with pixel stride ld"""
    g1, x1, s = rnd(P, ld), rnd(P, ld), out(P)
    sg, hg, sx, hx, wpsi, bpsi, sp, hp = rnd(f), rnd(f), rnd(f), rnd(f), rnd(f), rnd(1), rnd(1), rnd(1)
    st = ops.stream()
    check(lib.runet_ag_psi(p(g1), ld, p(x1), ld, p(sg), p(hg), p(sx), p(hx), p(wpsi), p(bpsi), p(s), P, f, st))
    att, datt, dxs, dsbn = out(P, ld), rnd(P, ld), out(P, ld), out(P)
    check(lib.runet_ag_out(p(x1), ld, p(s), p(sp), p(hp), p(att), ld, P, f, st))
    check(lib.runet_ag_bwd1(p(datt), ld, p(x1), ld, p(s), p(sp), p(hp), p(dxs), ld, p(dsbn), P, f, st))
    ds, mean_g, invstd_g, mean_x, invstd_x = rnd(P), rnd(f), pos(f), rnd(f), pos(f)
    res = [s, att, dxs, dsbn]
    for bn in (0, 1):
        dpre, dw, sums_g, sums_x, k = out(P, ld), out(f + 1), out(2 * f), out(2 * f), ws(lib.runet_ag_bwd2_bn_workspace_floats(P, f))
        head = (p(ds), p(g1), ld, p(x1), ld, p(sg), p(hg), p(sx), p(hx), p(wpsi))
        if bn:
            check(lib.runet_ag_bwd2_bn(*head, p(mean_g), p(invstd_g), p(mean_x), p(invstd_x), p(dpre), ld, p(k), k.numel(), p(dw), p(sums_g), p(sums_x),
                                       P, f, st))
        else:
            check(lib.runet_ag_bwd2(*head, p(dpre), ld, p(k), p(dw), P, f, st))
        res += [dpre, dw] + ([sums_g, sums_x] if bn else [])
    return res


def att_outc(P, c, opt):
    """runet_outc_fwd with the logit wanted or not, runet_outc_bwd on the probability's or (prob NULL) the logit's gradient"""
    x, wt, b, logit, prob = rnd(P, c), rnd(c), rnd(1), out(P), out(P)
    check(lib.runet_outc_fwd(p(x), c, p(wt), p(b), p(logit) if opt else None, p(prob), P, c, ops.stream()))
    dprob, dx, dw_db, k = rnd(P), out(P, c), out(c + 1), ws(lib.runet_reduce_workspace_floats(1, P, c))
    check(lib.runet_outc_bwd(p(dprob), p(prob) if opt else None, p(x), c, p(wt), p(dx), c, p(k), p(dw_db), P, c, ops.stream()))
    return [logit, prob, dx, dw_db]


ATTENTION_CASES = [
    *[(att_rb_out, (*s, bits, pool, aff)) for s in ATT_SHAPES for bits in (0, 1) for pool in (0, 1) for aff in (0, 1)],
    *[(att_rb_out, (*s, 0, 0, 1, 0)) for s in ATT_SHAPES],
    *[(att_rb_bwd1, (*s, form)) for s in ATT_SHAPES for form in ("plain", "noact")],
    *[(att_rb_bwd1, (*s, "ex", pool, bits)) for s in ATT_SHAPES for pool in (0, 1) for bits in (0, 1)],
    *[(att_rb_bwd2, (*s, bn)) for s in ATT_SHAPES for bn in (0, 1)],
    *[(att_rb_bwd3, (*s, sc, m)) for s in ATT_SHAPES for sc in (0, 1) for m in (0, 3 * s[0] * s[1] * s[2])],
    *[(att_sa, s) for s in ATT_SHAPES],
    *[(att_ca, (s[0], s[3], cr)) for s in ATT_SHAPES for cr in (1, 3, 64) if cr <= s[3]],
    # f = 64 over the 2 x 20 x 36 pixels of strided views (pixel stride 2 f); f = 256 over 8 pixels
    (att_gate, (128, 8, 8)), (att_gate, (180, 12, 12)), (att_gate, (2 * 20 * 36, 64, 128)), (att_gate, (8, 256, 256)),
    *[(att_outc, (s[0] * s[1] * s[2], s[3], opt)) for s in ATT_SHAPES for opt in (1, 0)],
]


def wino2_weights(cin, cout, dgrad):
    """runet_wino_weights (csrc/conv_winograd.hip): U[16][K/4][N][4] of the forward or the rotated data-gradient filter"""
    wt, k, nn = rnd(3, 3, cin, cout), (cout if dgrad else cin), (cin if dgrad else cout)
    U = out(16, k, nn)
    check(lib.runet_wino_weights(p(wt), p(U), cin, cout, dgrad, ops.stream()))
    return [U]


def wino2_conv(n, h, w, cin, cout, dgrad):
    """runet_wino_weights, then runet_wino_conv: the forward with bias, or the data gradient accumulated into a channel slice"""
    k, nn = (cout, cin) if dgrad else (cin, cout)
    x, wt, b, U = rnd(n, h, w, k), rnd(3, 3, cin, cout), rnd(nn), out(16, k, nn)
    y = rnd(n, h, w, nn + 8) if dgrad else out(n, h, w, nn)
    check(lib.runet_wino_weights(p(wt), p(U), cin, cout, dgrad, ops.stream()))
    check(lib.runet_wino_conv(p(x), k, p(U), None if dgrad else p(b), p(y[..., 8:] if dgrad else y), nn + 8 if dgrad else nn, n, h, w, k, nn, dgrad,
                              ops.stream()))
    return [y]


def wino2_wgrad(n, h, w, cin, cout, ldx, ldy):
    """runet_wino_wgrad on channel slices (the last cin / cout channels of pixel strides ldx / ldy): slabs per tile range, summed in order"""
    x, dy, dw = rnd(n, h, w, ldx), rnd(n, h, w, ldy), out(3, 3, cin, cout)
    k = ws(lib.runet_wino_wgrad_workspace_floats(n, h, w, cin, cout))
    check(lib.runet_wino_wgrad(p(x[..., ldx - cin:]), ldx, p(dy[..., ldy - cout:]), ldy, p(dw), p(k), k.numel(), n, h, w, cin, cout, ops.stream()))
    return [dw]


# ---- csrc/conv_winograd.hip: the shapes of tests/test_gpu_wino2_f32.py.  (n, h, w, cin, cout); the data gradient contracts over cout (a multiple of 16)
WINO2_FWD = [(2, 8, 8, 16, 32), (1, 12, 20, 64, 128), (3, 4, 4, 128, 256), (2, 16, 16, 32, 48), (2, 64, 64, 64, 64), (1, 32, 32, 256, 64),
             (5, 6, 10, 48, 32), (1, 4, 36, 16, 6), (1, 20, 36, 16, 6)]
# (n, h, w, cin, cout, ldx, ldy): zig-zag with one / two tile ranges | odd tile columns, two ranges (x2) | odd tile rows | w < 4: the LDS form | slices
WINO2_WGRAD = [(1, 8, 8, 16, 16, 16, 16), (2, 16, 12, 48, 80, 48, 80), (4, 16, 6, 16, 16, 16, 16), (2, 16, 10, 32, 48, 32, 48),
               (5, 6, 10, 48, 32, 48, 32), (3, 8, 2, 16, 32, 16, 32), (2, 16, 12, 48, 80, 56, 96)]
WINO2_CASES = [
    *[(wino2_weights, (s[3], s[4], dg)) for s in WINO2_FWD[:4] + WINO2_FWD[7:8] for dg in (0, 1) if s[3 + dg] % 16 == 0],
    *[(wino2_conv, (*s, dg)) for s in WINO2_FWD for dg in (0, 1) if s[3 + dg] % 16 == 0],
    *[(wino2_wgrad, s) for s in WINO2_WGRAD],
]


# ---- the GEMM layer (csrc/gemm.hip, gemm_split.hip, conv_x3.hip and the weight-gradient and GEMM entry points of conv_igemm.hip): which
# kernel, tile and split count a shape takes is a host decision, and the split count fixes the order of the sums
def gemm_batched(batch, rows, k, n):
    a, b, c = rnd(batch, rows, k), rnd(batch, k, n), out(batch, rows, n)
    check(lib.runet_gemm_batched(p(a), k, rows * k, p(b), k * n, p(c), n, rows * n, batch, rows, k, n, ops.stream()))
    return [c]


def gemm_tn_batched(batch, rows, k, n, rps):
    a, b, c = rnd(batch, rows, k), rnd(batch, rows, n), out(-(-rows // rps), batch, k, n)
    check(lib.runet_gemm_tn_batched(p(a), k, rows * k, p(b), n, rows * n, p(c), batch, rows, k, n, rps, ops.stream()))
    return [c]


def conv_wgrad(n, h, w, cin, cin_w, cout, k, dil, tr):
    """runet_conv_wgrad with the workspace runet_conv_wgrad_workspace_floats asks for; the size is part of the fingerprint"""
    up = 2 if tr else 1
    x, dy, dw = rnd(n, h, w, cin), rnd(n, up * h, up * w, cout), out(k, k, cin_w, cout)
    floats = lib.runet_conv_wgrad_workspace_floats(n, h, w, cin_w, cout, k, k)
    buf = ws(max(floats, 4))
    check(lib.runet_conv_wgrad(p(x), cin, p(dy), cout, p(dw), p(buf), floats, n, h, w, cin, cin_w, cout, k, k, dil, tr, ops.stream()))
    return [dw, torch.tensor([floats])]


def gemm_x3_batched(batch, rows, k, n):
    a, b, c = rnd(batch, rows, k), rnd(batch, k, n), out(batch, rows, n)
    bp = torch.empty(lib.runet_gemm_x3_pack_elems(batch, k, n), device=DEV, dtype=torch.bfloat16)
    check(lib.runet_gemm_x3_pack(p(b), k * n, p(bp), batch, k, n, ops.stream()))
    check(lib.runet_gemm_x3_batched(p(a), k, rows * k, p(bp), p(c), n, rows * n, batch, rows, k, n, ops.stream()))
    return [c]


def gemm_x3_tn_batched(batch, rows, k, n, rps):
    a, b, c = rnd(batch, rows, k), rnd(batch, rows, n), out(-(-rows // rps), batch, k, n)
    check(lib.runet_gemm_x3_tn_batched(p(a), k, rows * k, p(b), n, rows * n, p(c), batch, rows, k, n, rps, ops.stream()))
    return [c]


def gemm_x3_tn_convt(n, h, w, cin, cout, rps):
    x, dy, c = rnd(n, h, w, cin), rnd(n, 2 * h, 2 * w, cout), out(-(-n * h * w // rps), 2, 2, cin, cout)
    check(lib.runet_gemm_x3_tn_convt(p(x), cin, p(dy), cout, p(c), n, h, w, cin, cout, rps, ops.stream()))
    return [c]


def conv_x3(n, h, w, cin, cout, mode, stats):
    """runet_conv_x3_pack, then runet_conv_x3 or runet_conv_x3_stats with a bias, accumulating onto old content.  cin: the channels the
    mode reads; h, w: the low-resolution side of the transposed modes"""
    taps = 2 if mode in (ops.CONVT_FWD, ops.CONVT_DGRAD) else 1
    wt = rnd(taps, taps, *((cout, cin) if mode in (ops.CONV_DGRAD, ops.CONVT_DGRAD) else (cin, cout)))
    sx, sy = (2 if mode == ops.CONVT_DGRAD else 1), (2 if mode == ops.CONVT_FWD else 1)
    x, b, y = rnd(n, sx * h, sx * w, cin), rnd(cout), rnd(n, sy * h, sy * w, cout)
    wp = torch.empty(lib.runet_conv_x3_pack_elems(cin, cout, mode), device=DEV, dtype=torch.bfloat16)
    check(lib.runet_conv_x3_pack(p(wt), p(wp), cin, cout, mode, ops.stream()))
    head = (p(x), cin, p(wp), p(b), p(y), cout, n, h, w, cin, cout, mode, 1)
    if not stats:
        check(lib.runet_conv_x3(*head, ops.stream()))
        return [y]
    part = out(lib.runet_conv_x3_stats_parts(n, h, w), cout, 3)
    check(lib.runet_conv_x3_stats(*head, p(part), ops.stream()))
    return [y, part]


# (n, h, w, cin, cin_w, cout, k, dil, transposed): the nine narrow 1x1 channel classes and the one-case-per-route list of
# tests/test_gpu_igemm_variants.py, then the routes that list leaves out: the stem, the transposed split-operand GEMM, a TN GEMM of two splits
WGRAD_SHAPES = [
    *[(3, 9, 11, ci, ci, co, 1, 1, 0) for ci in (20, 36, 68) for co in (20, 36, 68)],
    *[(c.n, c.h, c.w, c.cin, c.cin_w, c.cout, c.k, c.dil, c.tr) for c in igemm_ref.wgrad_cases()],
    (2, 9, 11, 4, 3, 16, 3, 1, 0), (1, 4, 16, 64, 64, 64, 2, 1, 1), (2, 16, 16, 128, 128, 128, 1, 1, 0),
]
GEMM_LAYER_CASES = [
    *[(gemm_batched, (c.batch, c.rows, c.k, c.n)) for c in igemm_ref.gemm_cases()],
    *[(gemm_tn_batched, (igemm_ref.TN_BATCH, rows, k, n, igemm_ref.TN_RPS)) for rows in igemm_ref.TN_ROWS for k in igemm_ref.TN_KN for n in igemm_ref.TN_KN],
    *[(conv_wgrad, s) for s in WGRAD_SHAPES],
    # gemm_nn_x3_kernel<64> (n <= 64) | <128>: 15 x 2 x 36 = 1080 tiles of 128 x 128
    (gemm_x3_batched, (2, 130, 48, 36)), (gemm_x3_batched, (36, 1800, 16, 132)),
    # the shapes of tests/test_gpu_x3_edges.py: three splits of 48 rows | the 1x1 weight gradient's two splits of 256 | the transposed one's single slab
    (gemm_x3_tn_batched, (2, 144, 48, 36, 48)), (gemm_x3_tn_batched, (1, 512, 128, 128, 256)), (gemm_x3_tn_convt, (1, 4, 16, 64, 64, 64)),
    # 1 x 6 x 10, 48 -> 36 (48 -> 48 for the data gradients) in the four modes, the 1x1 modes with statistics; conv_nn_x3_kernel<128>:
    # 205 x 2 tiles of 128 x 128 fill 0.8 of a round of 512
    *[(conv_x3, (1, 6, 10, 48, 36 if mode in (0, 2) else 48, mode, 0)) for mode in (0, 1, 2, 3)],
    *[(conv_x3, (1, 6, 10, 48, 36 if mode == 0 else 48, mode, 1)) for mode in (0, 1)],
    (conv_x3, (1, 164, 160, 16, 132, 0, 0)),
]


def stem_conv(n, h, w, cin_w, cout, shortcut):
    """runet_stem_conv_stats (csrc/conv_stem.hip): both outputs and their BatchNorm partials, one per 8 x 32 tile at the tile's index whichever
    block of the persistent grid computes it"""
    x, w3, w1 = rnd(n, h, w, 4), rnd(3, 3, cin_w, cout), rnd(1, 1, cin_w, cout) if shortcut else None
    parts = lib.runet_stem_conv_stats_parts(n, h, w)
    y3, s3 = out(n, h, w, cout), out(parts, cout, 3)
    y1, s1 = (out(n, h, w, cout), out(parts, cout, 3)) if shortcut else (None, None)
    check(lib.runet_stem_conv_stats(p(x), 4, p(w3), p(w1) if shortcut else None, p(y3), cout, p(y1) if shortcut else None, cout if shortcut else 0, n, h, w,
                                    cin_w, cout, p(s3), p(s1) if shortcut else None, ops.stream()))
    return [y3, s3] + ([y1, s1] if shortcut else [])


def fused_equal(name, fused, unfused):
    for i, (a, b) in enumerate(zip(fused, unfused)):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"{name}: output {i} differs from the unfused composition"


def att_head_fwd(n, h, w, c):
    """runet_rb_out_ex + runet_outc_fwd: the fingerprint; runet_rb_out_head (where the build has it) must give the same bytes"""
    t2, A, B, sa = tail_inputs(n, h, w, c)
    r, rs, rh, wt, b = rnd(n, h, w, c), rnd(c), rnd(c), rnd(c), rnd(1)
    P = n * h * w
    head = (p(t2), c, p(A), p(B), p(sa), p(r), c, p(rs), p(rh))
    res = [out(n, h, w, c), torch.zeros((P, c // 4), dtype=torch.uint8, device=DEV), out(P), out(P)]
    check(lib.runet_rb_out_ex(*head, p(res[0]), c, p(res[1]), None, 0, None, n, h, w, c, ops.stream()))
    check(lib.runet_outc_fwd(p(res[0]), c, p(wt), p(b), p(res[2]), p(res[3]), P, c, ops.stream()))
    if hasattr(lib, "runet_rb_out_head"):
        f = [torch.zeros_like(t) for t in res]
        check(lib.runet_rb_out_head(*head, p(f[0]), c, p(f[1]), p(wt), p(b), p(f[2]), p(f[3]), n, h, w, c, ops.stream()))
        fused_equal("runet_rb_out_head", f, res)
    return res


def att_head_bwd(n, h, w, c):
    """runet_outc_bwd + runet_rb_bwd1_ex on its dx: the fingerprint; runet_outc_bwd_dl + runet_rb_bwd1_rank1 must give the same bytes"""
    t2, A, B, sa = tail_inputs(n, h, w, c)
    P = n * h * w
    x, wt, dprob, prob, rb = torch.relu(rnd(n, h, w, c)), rnd(c), rnd(P), torch.sigmoid(rnd(P)), ri(16, P, c // 4, dtype=torch.uint8)
    k = ws(lib.runet_reduce_workspace_floats(1, P, c))
    dx, res = out(n, h, w, c), [out(c + 1), out(n, h, w, c), out(P)]
    tail = (p(t2), c, p(A), p(B), p(sa))
    check(lib.runet_outc_bwd(p(dprob), p(prob), p(x), c, p(wt), p(dx), c, p(k), p(res[0]), P, c, ops.stream()))
    check(lib.runet_rb_bwd1_ex(p(dx), c, None, 0, None, None, c, p(rb), *tail, p(res[1]), c, p(res[2]), n, h, w, c, ops.stream()))
    if hasattr(lib, "runet_rb_bwd1_rank1"):
        dl, f = out(P), [torch.zeros_like(t) for t in res]
        check(lib.runet_outc_bwd_dl(p(dprob), p(prob), p(x), c, p(dl), p(k), p(f[0]), P, c, ops.stream()))
        check(lib.runet_rb_bwd1_rank1(p(dl), p(wt), p(rb), *tail, p(f[1]), c, p(f[2]), n, h, w, c, ops.stream()))
        fused_equal("runet_rb_bwd1_rank1", f, res)
    return res


# the stem: one tile | ragged tile rows and columns | 27 tiles | the one- and two-column-tile instances.  The head folded into the last
# block's tail (C = 64): the unfused composition is the fingerprint, the fused entry points are held to it in the same run
STEM_HEAD_CASES = [
    (stem_conv, (1, 8, 32, 3, 64, 1)), (stem_conv, (2, 10, 40, 3, 64, 0)), (stem_conv, (3, 24, 96, 3, 64, 1)), (stem_conv, (2, 10, 40, 1, 32, 0)),
    (stem_conv, (2, 10, 40, 3, 32, 1)),
    *[(fn, s) for s in ((2, 6, 10, 64), (1, 16, 16, 64)) for fn in (att_head_fwd, att_head_bwd)],
]


# (entry point, arguments).  Partial rows each reducing case yields, from its file's chunk rule, against the 16 (hrnet, multiscale,
# water_index) or 8 (fastscnn, dwsep, dwconv) part-lanes of the final pass:
CASES = [
    # ceil(P c / 16384) chunks, width 3c + 1: 1 | 17 (one past the lanes) | 34
    (hr_head_bwd_reduce, (2, 3, 5, 8)), (hr_head_bwd_reduce, (2, 33, 65, 64)), (hr_head_bwd_reduce, (2, 33, 65, 128)),
    # ceil(P / rows) chunks, rows = 256 / (c / 4) (c = 12: 85 rows, width 24): 1 | 51 | 5 | 1 (a one-row map)
    *[(bilinear_nhwc_bwd_sums, (*shape, s)) for s in (2, 4) for shape in ((2, 3, 5, 8), (2, 33, 65, 12), (2, 5, 7, 64), (1, 1, 3, 8))],
    (up2_sigmoid_bwd, (2, 5, 7)), (up2_sigmoid_bwd, (1, 1, 3)), (up2_sigmoid_bwd, (2, 4, 8)),
    *[(up_sigmoid_bwd, (*shape, s)) for s in (2, 3, 4) for shape in ((2, 5, 7), (1, 1, 3))],
    # ceil(P / (4 rows)) chunks over the OUTPUT pixels, widths 9c / 10c (72, 108: no multiples of 32): 1 | 13 | 68 (stride 2: 1 | 4 | 18)
    *[(dw3_wgrad, (*shape, stride)) for stride in (1, 2) for shape in ((2, 3, 5, 8), (2, 33, 65, 12), (2, 33, 65, 64))],
    (dwconv3x3_gelu_bwd_wgrad, (2, 3, 5, 8, True)), (dwconv3x3_gelu_bwd_wgrad, (2, 33, 65, 12, False)), (dwconv3x3_gelu_bwd_wgrad, (2, 33, 65, 64, True)),
    # one chunk per 64-pixel tile up to 128 (cin cout is always a multiple of 32): 1 | 68 (stride 2: 1 | 18)
    *[(dwsep_wgrad_pw, (*shape, stride)) for stride in (1, 2) for shape in ((2, 3, 5, 16, 16), (2, 33, 65, 16, 48))],
    # one partial row per 8 x 32 tile, width 128: 2 | 30 | 45
    (ms_stem_bwd_reduce, (2, 3, 5)), (ms_stem_bwd_reduce, (2, 33, 65)), (ms_stem_bwd_reduce, (3, 33, 65)),
    # one partial row per 2048 pixels, widths 100 and 64: 1 | 3 | 33
    (water_index_bwd, (2, 3, 5)), (water_index_bwd, (2, 33, 65)), (water_index_bwd, (2, 129, 257)),
    (pyramid_upsample_bwd, (2, 5, 7, 8)), (pyramid_upsample_bwd, (1, 1, 3, 4)), (pyramid_upsample_bwd, (2, 33, 65, 16)),
    (bilinear_bwd, (3, 5, 7, 11, 13)), (bilinear_bwd, (2, 1, 3, 2, 9)), (bilinear_bwd, (2, 9, 11, 5, 7)),
    (bilinear_nhwc_bwd, (2, 5, 7, 11, 13, 8)), (bilinear_nhwc_bwd, (1, 1, 3, 2, 9, 4)), (bilinear_nhwc_bwd, (2, 9, 11, 5, 7, 12)),
    *NORM_ACT_CASES,
    *[(wino_conv_x3, (*s, st)) for s in WINO_X3_SHAPES for st in (0, 1)],
    *ATTENTION_CASES,
    *WINO2_CASES,
    *GEMM_LAYER_CASES,
    *STEM_HEAD_CASES,
]


def main():
    for fn, args in CASES:
        outs = fn(*args)
        torch.cuda.synchronize()
        if fn.__name__.startswith("att_"):      # up to twelve outputs per case: one fingerprint over all of them, in order
            h = hashlib.sha256()
            for t in outs:
                h.update(t.cpu().numpy().tobytes())
            print(f"{fn.__name__}{args} {len(outs)} outputs {h.hexdigest()}")
            continue
        for i, t in enumerate(outs):
            print(f"{fn.__name__}{args} out{i} {tuple(t.shape)} {hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()}")


if __name__ == "__main__":
    main()
