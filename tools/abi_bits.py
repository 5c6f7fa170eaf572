"""Bit fingerprints of the entry points whose results rest on a fixed summation order: the two-stage reductions (chunk partials, then the
ordered final pass sum_parts of csrc/runet_common.h) and the gather adjoints of the bilinear resizes.  Every case fills seeded inputs, calls
the entry point once through the package's binding and prints one SHA-256 per output tensor.  Two builds of the library compute the same
bits exactly when their printouts are equal line for line; RUNET_HIP_LIB selects the build (see _lib.py), one fresh process per build:

  RUNET_HIP_LIB=/path/to/other/librunet_hip.so python tools/abi_bits.py > a.txt
  python tools/abi_bits.py > b.txt && diff a.txt b.txt

The shapes are the smallest at which an order can go wrong: fewer partial rows than the final pass has part-lanes (16 or 8), more than
twice as many, a reduced width that is no multiple of the 16 / 32 outputs of a block; odd non-square and one-row maps for the resizes.
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
]


def main():
    for fn, args in CASES:
        outs = fn(*args)
        torch.cuda.synchronize()
        for i, t in enumerate(outs):
            print(f"{fn.__name__}{args} out{i} {tuple(t.shape)} {hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()}")


if __name__ == "__main__":
    main()
