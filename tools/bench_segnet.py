"""SegNet baseline (comne.py:84-211) on one MI355X: train-step throughput at 16 x 256^2 (BCE + Adam, fp32 and bf16), and single-stream kernel
times of the fused encoder-end kernels against the launches they replace, at the four encoder-end shapes (n = 16):

  forward    runet_bn_relu_maxpool2_fwd                             vs  runet_bn_apply(relu) + runet_maxpool2_fwd
  backward   runet_bn_bwd_reduce_pooled + runet_bn_bwd_apply_pooled  vs  runet_maxpool2_bwd + runet_bn_bwd_reduce + runet_bn_bwd_apply

Not a bench line of the contract (bench.py measures the Robust U-Net metric); the figures are quoted in DESIGN.md.
  python tools/bench_segnet.py [--what all|step|kernels] [--reps 50] [--steps 30]
  python tools/bench_segnet.py --counters fused|composed     one pass of one variant per shape, no timing (for rocprofv3 --pmc runs)
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("eusipco-2026-robust-unet_amd")
B = importlib.import_module("eusipco-2026-robust-unet_amd.blocks")

SHAPES = ((256, 256, 64), (128, 128, 128), (64, 64, 256), (32, 32, 512))
DEV = torch.device("cuda:0")


def step_throughput(precision, n=16, size=256, steps=30, warm=5):
    torch.manual_seed(0)
    model = pkg.SegNet().to(DEV).train().set_precision(precision)
    opt = pkg.FusedAdam(model.parameters(), lr=1e-4, weight_decay=1e-4)
    x, y = pkg.synthetic_batch(n, size, seed=1234)
    x, y = x.to(DEV), y.to(DEV)

    def step():
        opt.zero_grad()
        loss = pkg.bce_loss(model(x), y)
        loss.backward()
        opt.step()
        return loss

    for _ in range(warm):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"model": "SegNet baseline", "precision": precision, "images_per_s": round(n * steps / dt, 1), "ms_per_step": round(1e3 * dt / steps, 3),
            "batch": n, "size": size, "final_loss": round(float(loss.item()), 5)}


def _operands(h, w, c, n=16):
    g = torch.Generator().manual_seed(h + c)
    t = torch.randn((n, h, w, c), generator=g).to(DEV)
    bn = B.BNState(torch.ones(c, device=DEV), torch.zeros(c, device=DEV), torch.zeros(c, device=DEV), torch.ones(c, device=DEV),
                   torch.zeros((), dtype=torch.int64, device=DEV))
    s, sh, mean, invstd, _ = B.bn_coeff(t, bn, True, B.Small(DEV))
    _, idx = B.bn_relu_maxpool_forward(t, s, sh)
    dp = torch.randn((n, h // 2, w // 2, c), generator=g).to(DEV)
    sums = torch.empty(2 * c, device=DEV)
    return dict(t=t, s=s, sh=sh, mean=mean, invstd=invstd, idx=idx, dp=dp, sums=sums)


def _variants(o):
    def fwd_fused():
        B.bn_relu_maxpool_forward(o["t"], o["s"], o["sh"])

    def fwd_composed():
        B.maxpool_forward(B.bn_apply(o["t"], o["s"], o["sh"], None, relu=True))

    def bwd_fused():
        B.bn_backward_pooled(o["dp"], o["idx"], o["t"], o["mean"], o["invstd"], o["s"], o["sums"], o["sh"])

    def bwd_composed():
        g = B.maxpool_backward(o["dp"], o["idx"])
        B.bn_backward(g, o["t"], o["mean"], o["invstd"], o["s"], o["sums"], relu_shift=o["sh"])
    return {"fwd": (fwd_fused, fwd_composed), "bwd": (bwd_fused, bwd_composed)}


def kernel_times(reps=50):
    rows = []
    for h, w, c in SHAPES:
        o = _operands(h, w, c)
        for kind, fns in _variants(o).items():
            for f in fns:
                f(); f()                                      # warm: code objects, allocator
            times = ([], [])
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            for r in range(reps):
                for j in ((0, 1) if r % 2 == 0 else (1, 0)):   # alternate the order
                    ev[0].record()
                    fns[j]()
                    ev[1].record()
                    ev[1].synchronize()
                    times[j].append(ev[0].elapsed_time(ev[1]) * 1e3)
            fused, composed = statistics.median(times[0]), statistics.median(times[1])
            n = 16
            full = n * h * w * c * 4
            # bytes each variant must move: full = one full-resolution fp32 tensor, pooled values full / 4, index bytes full / 16.
            # fwd fused: t in, y + idx out; composed: + the activation written and read again.  bwd fused: (dpool, idx, x) read by both
            # launches + dx out; composed: the scatter writes g (full), the reduce and apply read (g, x) each, dx out
            need = {"fwd": (full + full // 4 + full // 16, 3 * full + full // 4 + full // 16),
                    "bwd": (2 * (full + full // 4 + full // 16) + full, 6 * full + full // 4 + full // 16)}[kind]
            rows.append({"shape": [n, h, w, c], "pass": kind, "fused_us": round(fused, 1), "composed_us": round(composed, 1),
                         "speedup": round(composed / fused, 3), "fused_bytes_min": need[0], "composed_bytes_min": need[1]})
            print(json.dumps(rows[-1]), flush=True)
        del o
        torch.cuda.empty_cache()
    return rows


def counters(which):
    """Operands of all four shapes first (their set-up launches one runet_bn_relu_maxpool2_fwd per shape for the indices), then ONE pass of the
    chosen variant per shape in SHAPES order: forward, then backward (fused: 1 + 3 dispatches per shape, composed: 2 + 4)."""
    ops_ = [_operands(h, w, c) for h, w, c in SHAPES]
    torch.cuda.synchronize()
    j = 0 if which == "fused" else 1
    for o in ops_:
        for kind, fns in _variants(o).items():
            fns[j]()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="all", choices=("all", "step", "kernels"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--counters", choices=("fused", "composed"))
    a = ap.parse_args()
    if a.counters:
        counters(a.counters)
        return
    out = {}
    if a.what in ("all", "kernels"):
        out["kernels"] = kernel_times(a.reps)
    if a.what in ("all", "step"):
        out["step"] = [step_throughput(p, steps=a.steps) for p in ("f32", "bf16")]
        for r in out["step"]:
            print(json.dumps(r), flush=True)
    print(json.dumps({"segnet_bench": out}))


if __name__ == "__main__":
    main()
