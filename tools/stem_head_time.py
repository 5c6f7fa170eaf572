"""Single-stream timings of the launches the persistent stem and the fused head touch, at the flagship's shapes (16 x 256^2, fp32), for the
library of the tree it runs in: device events around `--reps` launches after a warm-up, median [min-max] over `--rounds` rounds, next to
the rate of a 1 GiB float copy (read + write) of the same process.

  stem       runet_stem_conv_stats 3 -> 64 with the 1x1 shortcut (writes 2 x 268 MB, reads 4 MB)
  head fwd   runet_rb_out_ex(bits) + runet_outc_fwd          | runet_rb_out_head
  head bwd   runet_outc_bwd + runet_rb_bwd1_ex(bits)         | runet_outc_bwd_dl + runet_rb_bwd1_rank1

The fused forms are timed where the library has them, so the same file runs in a checkout of the parent commit.  Prints one JSON line.
  python tools/stem_head_time.py [--n 16] [--size 256] [--reps 20] [--rounds 5]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
importlib.import_module("eusipco-2026-robust-unet_amd")
ops = importlib.import_module("eusipco-2026-robust-unet_amd.ops")
L = importlib.import_module("eusipco-2026-robust-unet_amd._lib")
lib, check = L.lib, L.check
DEV = torch.device("cuda:0")


def timed(fn, reps, rounds):
    """-> microseconds per call: median, min, max over the rounds"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        us.append(1e3 * a.elapsed_time(b) / reps)
    return dict(median=round(statistics.median(us), 1), min=round(min(us), 1), max=round(max(us), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    n, h, w, c = a.n, a.size, a.size, 64
    P = n * h * w
    g = torch.Generator().manual_seed(7)

    def rnd(*shape):
        return torch.randn(shape, generator=g).to(DEV)
    st = ops.stream()
    p = torch.Tensor.data_ptr
    res = {"lib": L.LIB_PATH, "n": n, "size": a.size, "device": torch.cuda.get_device_name(0)}
    src, dst = torch.empty(1 << 28, device=DEV), torch.empty(1 << 28, device=DEV)
    t = timed(lambda: dst.copy_(src), 10, a.rounds)
    res["copy_TBps"] = round(2 * 4 * (1 << 28) / (t["median"] * 1e-6) / 1e12, 3)
    del src, dst
    # ---- stem
    x, w3, w1 = rnd(n, h, w, 4), rnd(3, 3, 3, c), rnd(1, 1, 3, c)
    y3, y1 = torch.empty((n, h, w, c), device=DEV), torch.empty((n, h, w, c), device=DEV)
    parts = lib.runet_stem_conv_stats_parts(n, h, w)
    s3, s1 = torch.empty((parts, c, 3), device=DEV), torch.empty((parts, c, 3), device=DEV)
    res["stem"] = timed(lambda: check(lib.runet_stem_conv_stats(p(x), 4, p(w3), p(w1), p(y3), c, p(y1), c, n, h, w, 3, c, p(s3), p(s1), st)), a.reps, a.rounds)
    res["stem"]["bytes"] = 2 * P * c * 4 + P * 16 + 2 * parts * c * 12
    res["stem"]["at_copy_rate_us"] = round(res["stem"]["bytes"] / (res["copy_TBps"] * 1e12) * 1e6, 1)
    del y1, s3, s1
    # ---- head forward
    t2, r, sa, A, B = rnd(n, h, w, c), rnd(n, h, w, c), torch.sigmoid(rnd(P)), rnd(n, c), rnd(n, c)
    hw_, hb = rnd(c), rnd(1)
    out, bits = y3, torch.empty((P, c // 4), device=DEV, dtype=torch.uint8)
    logit, prob = torch.empty(P, device=DEV), torch.empty(P, device=DEV)
    head = (p(t2), c, p(A), p(B), p(sa), p(r), c, None, None, p(out), c, p(bits))

    def fwd_pair():
        check(lib.runet_rb_out_ex(*head, None, 0, None, n, h, w, c, st))
        check(lib.runet_outc_fwd(p(out), c, p(hw_), p(hb), None, p(prob), P, c, st))
    res["head_fwd_pair"] = timed(fwd_pair, a.reps, a.rounds)
    res["rb_out_ex"] = timed(lambda: check(lib.runet_rb_out_ex(*head, None, 0, None, n, h, w, c, st)), a.reps, a.rounds)
    if hasattr(lib, "runet_rb_out_head"):
        res["head_fwd_fused"] = timed(lambda: check(lib.runet_rb_out_head(*head, p(hw_), p(hb), None, p(prob), n, h, w, c, st)), a.reps, a.rounds)
    # ---- head backward
    dprob, dx, dv, dq, dl = rnd(P), r, torch.empty((n, h, w, c), device=DEV), logit, torch.empty(P, device=DEV)
    dw = torch.empty(c + 1, device=DEV)
    ws = torch.empty(lib.runet_reduce_workspace_floats(1, P, c), device=DEV)
    tail = (p(bits), p(t2), c, p(A), p(B), p(sa), p(dv), c, p(dq), n, h, w, c, st)

    def bwd_pair():
        check(lib.runet_outc_bwd(p(dprob), p(prob), p(out), c, p(hw_), p(dx), c, p(ws), p(dw), P, c, st))
        check(lib.runet_rb_bwd1_ex(p(dx), c, None, 0, None, None, c, *tail))
    res["head_bwd_pair"] = timed(bwd_pair, a.reps, a.rounds)
    res["outc_bwd"] = timed(lambda: check(lib.runet_outc_bwd(p(dprob), p(prob), p(out), c, p(hw_), p(dx), c, p(ws), p(dw), P, c, st)), a.reps, a.rounds)
    if hasattr(lib, "runet_rb_bwd1_rank1"):
        def bwd_fused():
            check(lib.runet_outc_bwd_dl(p(dprob), p(prob), p(out), c, p(dl), p(ws), p(dw), P, c, st))
            check(lib.runet_rb_bwd1_rank1(p(dl), p(hw_), *tail))
        res["head_bwd_fused"] = timed(bwd_fused, a.reps, a.rounds)
        res["outc_bwd_dl"] = timed(lambda: check(lib.runet_outc_bwd_dl(p(dprob), p(prob), p(out), c, p(dl), p(ws), p(dw), P, c, st)), a.reps, a.rounds)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
