"""Bit fingerprints of the entry points whose results rest on a fixed summation order: the two-stage reductions (chunk partials, then the
ordered final pass sum_parts of csrc/runet_common.h), the gather adjoints of the bilinear resizes, and every entry point of csrc/norm_act.hip
(BatchNorm statistics, apply and backward: Chan combines in chunk order, first-occurrence max / min, explicit FMAs).  Every case fills seeded inputs, calls
the entry point once through the package's binding and prints one SHA-256 per output tensor.  Two builds of the library compute the same
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
sys.path.insert(0, ROOT)
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
]


def main():
    for fn, args in CASES:
        outs = fn(*args)
        torch.cuda.synchronize()
        for i, t in enumerate(outs):
            print(f"{fn.__name__}{args} out{i} {tuple(t.shape)} {hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()}")


if __name__ == "__main__":
    main()
