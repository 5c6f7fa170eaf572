"""YOLOSeg baseline (Main_Final.py:436-510) on one MI355X: train-step throughput (BCE + Adam, fp32) at 16 x 256^2 and 4 x 512^2, and
single-stream kernel times of the two fusions against the launches they replace (n = 16):

  pool fwd   runet_bn_leaky_maxpool2_fwd                                        vs  runet_bn_apply_leaky + runet_maxpool2_fwd
  pool bwd   runet_bn_bwd_reduce_pooled_leaky + runet_bn_bwd_apply_pooled_leaky  vs  runet_maxpool2_bwd + runet_bn_bwd_reduce_leaky + _apply_leaky
             at the four stage-end shapes of the backbone
  convt4     runet_convt4_igemm_stats + runet_bn_stats_finalize                 vs  runet_convt4_igemm + runet_bn_stats
             at the four seg_head shapes

Not a bench line of the contract (bench.py measures the Robust U-Net metric); the figures are quoted in DESIGN.md.
  python tools/bench_yolo.py [--what all|step|kernels] [--reps 50] [--steps 30]
  python tools/bench_yolo.py --counters fused|composed     one pass of one variant per shape, no timing (for rocprofv3 --pmc runs)
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
ops = importlib.import_module("eusipco-2026-robust-unet_amd.ops")

POOL_SHAPES = ((256, 256, 32), (128, 128, 64), (64, 64, 128), (32, 32, 256))
DEC_SHAPES = ((16, 16, 256, 128), (32, 32, 128, 64), (64, 64, 64, 32), (128, 128, 32, 16))
SLOPE = 0.1
DEV = torch.device("cuda:0")


def step_throughput(n, size, steps=30, warm=5):
    torch.manual_seed(0)
    model = pkg.YOLOSeg().to(DEV).train()
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
    return {"model": "YOLOSeg baseline", "precision": "f32", "images_per_s": round(n * steps / dt, 1), "ms_per_step": round(1e3 * dt / steps, 3),
            "batch": n, "size": size, "final_loss": round(float(loss.item()), 5)}


def _bn():
    return lambda c: B.BNState(torch.ones(c, device=DEV), torch.zeros(c, device=DEV), torch.zeros(c, device=DEV), torch.ones(c, device=DEV),
                               torch.zeros((), dtype=torch.int64, device=DEV))


def _pool_operands(h, w, c, n=16):
    g = torch.Generator().manual_seed(h + c)
    t = torch.randn((n, h, w, c), generator=g).to(DEV)
    s, sh, mean, invstd, _ = B.bn_coeff(t, _bn()(c), True, B.Small(DEV))
    _, idx = B.bn_leaky_maxpool_forward(t, s, sh, SLOPE)
    dp = torch.randn((n, h // 2, w // 2, c), generator=g).to(DEV)
    return dict(t=t, s=s, sh=sh, mean=mean, invstd=invstd, idx=idx, dp=dp, sums=torch.empty(2 * c, device=DEV))


def _pool_variants(o):
    def fwd_fused():
        B.bn_leaky_maxpool_forward(o["t"], o["s"], o["sh"], SLOPE)

    def fwd_composed():
        B.maxpool_forward(B.bn_apply_leaky(o["t"], o["s"], o["sh"], SLOPE))

    def bwd_fused():
        B.bn_backward_pooled_leaky(o["dp"], o["idx"], o["t"], o["mean"], o["invstd"], o["s"], o["sums"], o["sh"], SLOPE)

    def bwd_composed():
        B.bn_backward_leaky(B.maxpool_backward(o["dp"], o["idx"]), o["t"], o["mean"], o["invstd"], o["s"], o["sums"], o["sh"], SLOPE)
    return {"pool_fwd": (fwd_fused, fwd_composed), "pool_bwd": (bwd_fused, bwd_composed)}


def _dec_operands(h, w, cin, cout, n=16):
    g = torch.Generator().manual_seed(h + cin)
    return dict(x=torch.randn((n, h, w, cin), generator=g).to(DEV), w=(torch.randn((4, 4, cin, cout), generator=g) / (4 * cin ** 0.5)).to(DEV),
                b=torch.zeros(cout, device=DEV), bn=_bn()(cout), sm=B.Small(DEV))


def _dec_variants(o):
    def fused():
        fs = {}
        y = ops.convt4_fwd(o["x"], o["w"], o["b"], stats=fs)
        B.bn_coeff(y, o["bn"], True, o["sm"], fused=fs)

    def composed():
        y = ops.convt4_fwd(o["x"], o["w"], o["b"])
        B.bn_coeff(y, o["bn"], True, o["sm"])
    return {"convt4_bn_stats": (fused, composed)}


def _time(fns, reps):
    for f in fns:
        f(); f()                                              # warm: code objects, allocator
    times = ([], [])
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for r in range(reps):
        for j in ((0, 1) if r % 2 == 0 else (1, 0)):         # alternate the order
            ev[0].record()
            fns[j]()
            ev[1].record()
            ev[1].synchronize()
            times[j].append(ev[0].elapsed_time(ev[1]) * 1e3)
    return statistics.median(times[0]), statistics.median(times[1])


def kernel_times(reps=50):
    rows = []
    cases = [((16, h, w, c), _pool_operands(h, w, c), _pool_variants) for h, w, c in POOL_SHAPES]
    for shape, o, var in cases + [((16, h, w, ci, co), _dec_operands(h, w, ci, co), _dec_variants) for h, w, ci, co in DEC_SHAPES]:
        for kind, fns in var(o).items():
            fused, composed = _time(fns, reps)
            rows.append({"shape": list(shape), "pass": kind, "fused_us": round(fused, 1), "composed_us": round(composed, 1),
                         "speedup": round(composed / fused, 3)})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def counters(which):
    """ONE pass of the chosen variant per shape (pool forward, pool backward, then the four decoder shapes), operands built first."""
    cases = [(_pool_operands(h, w, c), _pool_variants) for h, w, c in POOL_SHAPES] + \
            [(_dec_operands(h, w, ci, co), _dec_variants) for h, w, ci, co in DEC_SHAPES]
    torch.cuda.synchronize()
    j = 0 if which == "fused" else 1
    for o, var in cases:
        for _, fns in var(o).items():
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
        out["step"] = [step_throughput(n, s, steps=a.steps) for n, s in ((16, 256), (4, 512))]
        for r in out["step"]:
            print(json.dumps(r), flush=True)
    print(json.dumps({"yolo_bench": out}))


if __name__ == "__main__":
    main()
