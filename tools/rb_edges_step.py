"""Robust U-Net train step (fp32, BCE + FusedAdam as bench.py runs it) with the ResidualBlock edge fusions of blocks.FUSED_RB_EDGES toggled one at a
time: each of the three kernels alone (out: runet_rb_out_ex, bwd1: runet_rb_bwd1_ex, bwd3: runet_rb_bwd3_sc), all of them (the default) and
none (RUNET_NO_FUSED_RB_EDGES=1).  The settings are warmed up and then timed in interleaved rounds inside one process (none, out, bwd1, bwd3,
all, none, ...), the device synchronised before the clock is read; the figure of a setting is the median of its rounds, the spread their
min / max.  Prints one JSON line; --out merges it under the key "per_part" into an existing JSON file (profiles/rb_edges_16x256_ab.json).

Not a bench line of the contract (bench.py measures the metric); the figures are quoted in DESIGN.md.
  python tools/rb_edges_step.py [--n 16] [--size 256] [--warmup 5] [--rounds 7] [--min-seconds 1.0] [--out FILE]
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
DEV = torch.device("cuda:0")
ALL = frozenset(("out", "bwd1", "bwd3"))
SETTINGS = (("none", False, ALL), ("out", True, frozenset(("out",))), ("bwd1", True, frozenset(("bwd1",))), ("bwd3", True, frozenset(("bwd3",))),
            ("all", True, ALL))


def set_config(on, parts):
    B.FUSED_RB_EDGES, B.RB_EDGE_PARTS = on, parts


def run_for(step, min_seconds):
    torch.cuda.synchronize()
    steps, t0 = 0, time.perf_counter()
    while True:
        loss = step()
        steps += 1
        if steps % 5 == 0:
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if dt >= min_seconds:
                return steps, dt, float(loss.item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--base", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--min-seconds", type=float, default=1.0, help="per setting and round")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(1234)
    model = pkg.RobustUNet(3, 1, a.base).to(DEV).train()
    train = pkg.TrainStep(model, lr=1e-4, weight_decay=1e-4)
    x, y = pkg.synthetic_batch(a.n, a.size, seed=1234)
    x, y = x.to(DEV), y.to(DEV)

    def step():
        return train(x, y)
    for _, on, parts in SETTINGS:
        set_config(on, parts)
        for _ in range(a.warmup):
            step()
    rounds = {name: [] for name, _, _ in SETTINGS}
    for _ in range(a.rounds):
        for name, on, parts in SETTINGS:
            set_config(on, parts)
            k, dt, _ = run_for(step, a.min_seconds)
            rounds[name].append(1e3 * dt / k)
    set_config(True, ALL)
    res = {"model": "RobustUNet", "precision": "f32", "batch": a.n, "size": a.size, "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "settings": {}}
    base = statistics.median(rounds["none"])
    for name, _, _ in SETTINGS:
        ms = statistics.median(rounds[name])
        res["settings"][name] = {"ms_per_step": round(ms, 3), "min_ms": round(min(rounds[name]), 3), "max_ms": round(max(rounds[name]), 3),
                                 "rounds_ms": [round(v, 3) for v in rounds[name]], "images_per_s": round(1e3 * a.n / ms, 1),
                                 "ms_saved_vs_none": round(base - ms, 3)}
    line = json.dumps(res)
    print(line)
    if a.out:
        doc = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                doc = json.load(f)
        doc["per_part"] = res
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
