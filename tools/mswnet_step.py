"""MSWNet (Extended_Baseline_Comparison.py:479-548) train step on one MI355X, fp32, BCE + Adam(1e-4, weight decay 1e-4): the HIP module
(`MSWNet` + FusedAdam) against the CPU restatement tests/mswnet_ref.py run eagerly on torch-ROCm on the same GPU (torch.optim.Adam), same
inputs and initial state, and against its own A/B partner.  The two HIP configurations (fused multi-scale stem, RUNET_NO_FUSED_MS_STEM - selected
here through the flag blocks.py reads that variable into) are warmed up and then timed in interleaved rounds (fused, unfused, fused, ...), the
device synchronised before the clock is read; the figure of a configuration is the median of its rounds, the spread their min / max.
"stem_default": the rule the default of blocks.FUSED_MS_STEM follows - fused stays the default only if its median is not above the partner's by
more than the round-to-round spread (the larger max - min of the two configurations) seen in this run.  Prints one JSON line; --out also writes
it to a file.

--kernels: single-stream times of the six new kernels at the 16 x 256^2 shape (the pool at level 2's 16 x 128^2 x 64) with the bytes each moves
(derived from the tensor sizes) and the HBM bandwidth that makes, and the first level's forward and backward as a whole, fused against unfused.

Not a bench line of the contract (bench.py measures the Robust U-Net metric); the figures are quoted in DESIGN.md.
  python tools/mswnet_step.py [--n 16] [--size 256] [--warmup 5] [--rounds 5] [--min-seconds 0.4] [--only hip|torch] [--out FILE]
  python tools/mswnet_step.py --kernels [--reps 50] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("eusipco-2026-robust-unet_amd")
B = importlib.import_module("eusipco-2026-robust-unet_amd.blocks")
mref = importlib.import_module("mswnet_ref")
DEV = torch.device("cuda:0")
CONFIGS = (("fused", True), ("unfused_ms_stem", False))


def set_config(fused):
    B.FUSED_MS_STEM = fused


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


def hip_step(st, x, y):
    model = pkg.MSWNet()
    model.load_state_dict(st, strict=True)
    model.to(DEV).train()
    opt = pkg.FusedAdam(model.parameters(), lr=1e-4, weight_decay=1e-4)

    def step():
        opt.zero_grad()
        loss = pkg.bce_loss(model(x), y)
        loss.backward()
        opt.step()
        return loss
    return step


def torch_step(st, x, y):
    names = mref.param_names()
    P = {k: v.clone().to(DEV) for k, v in st.items()}
    params = [P[k].requires_grad_(True) for k in names]
    opt = torch.optim.Adam(params, lr=1e-4, weight_decay=1e-4)

    def step():
        opt.zero_grad()
        loss = torch.nn.functional.binary_cross_entropy(mref.forward(P, x, True), y)
        loss.backward()
        opt.step()
        return loss
    return step


def _time_us(fn, reps):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(1e3 * e0.elapsed_time(e1) / reps, 2)


def kernel_times(n, size, reps):
    ops = importlib.import_module("eusipco-2026-robust-unet_amd.ops")
    L = importlib.import_module("eusipco-2026-robust-unet_amd._lib")
    lib, check = L.lib, L.check
    g = torch.Generator().manual_seed(0)
    P = n * size * size
    out = {"batch": n, "size": size, "device": torch.cuda.get_device_name(0), "kernels": [], "first_level": {}}

    def row(name, us, nbytes):
        out["kernels"].append({"kernel": name, "us": us, "MB": round(nbytes / 1e6, 1), "GB_per_s": round(nbytes / us / 1e3, 1)})

    net = pkg.MSWNet().to(DEV).train()
    p = net.enc1.handles()
    x = torch.rand((n, 3, size, size), generator=g).to(DEV)
    cat = torch.empty((n, size, size, 128), device=DEV)
    dcat = torch.randn((n, size, size, 128), generator=g).to(DEV)
    e, de = cat[..., 64:], dcat[..., 64:]                  # as in the model: the skip halves of the level-1 concat buffer and of its gradient
    src = (x.data_ptr(),) + tuple(x.stride()) + (n, size, size)
    wts = tuple(t.data_ptr() for t in p.w) + tuple(t.data_ptr() for t in p.b)
    sm = B.Small(DEV)
    _, ctx = B.ms_stem_forward(x, p, True, sm, out=e, fused=True)
    sc, sh, mean, invstd = (ctx[k].data_ptr() for k in ("scale", "shift", "mean", "invstd"))
    nparts = lib.runet_ms_stem_parts(n, size, size)
    part = torch.empty(4 * nparts * 48, device=DEV)
    ws = B.scratch(lib.runet_ms_stem_workspace_floats(n, size, size), DEV)
    sums, dt = torch.empty(128, device=DEV), torch.empty((n, size, size, 64), device=DEV)
    st = ops.stream()
    xb, eb = 4 * 3 * P, 4 * 64 * P              # the image; a 64-channel tensor
    row("runet_ms_stem_stats", _time_us(lambda: check(lib.runet_ms_stem_stats(*src, *wts, part.data_ptr(), part.numel(), st)), reps), xb)
    row("runet_ms_stem_fwd", _time_us(lambda: check(lib.runet_ms_stem_fwd(*src, *wts, sc, sh, e.data_ptr(), 128, st)), reps), xb + eb)
    row("runet_ms_stem_bwd_reduce", _time_us(lambda: check(lib.runet_ms_stem_bwd_reduce(*src, *wts, sc, sh, de.data_ptr(), 128, mean, invstd, ws.data_ptr(),
                                                                                        ws.numel(), sums.data_ptr(), st)), reps), xb + eb)
    row("runet_ms_stem_bwd_apply", _time_us(lambda: check(lib.runet_ms_stem_bwd_apply(*src, *wts, sc, sh, de.data_ptr(), 128, mean, invstd, sums.data_ptr(), 0,
                                                                                      dt.data_ptr(), 64, st)), reps), xb + 2 * eb)
    # the pool at level 2: 16 x 128^2 x 64 (values read once from HBM, written once, one winner byte each; the backward reads dy and the bytes,
    # reads and writes dx)
    h2 = size // 2
    P2 = n * h2 * h2
    x2, dy2 = torch.randn((n, h2, h2, 64), generator=g).to(DEV), torch.randn((n, h2, h2, 64), generator=g).to(DEV)
    y2, idx2 = B.maxpool3s1_forward(x2)
    dx2 = torch.zeros_like(x2)
    row("runet_maxpool3s1_fwd", _time_us(lambda: B.maxpool3s1_forward(x2, out=y2), reps), P2 * 64 * 9)
    row("runet_maxpool3s1_bwd", _time_us(lambda: B.maxpool3s1_backward(dy2, idx2, dx=dx2), reps), P2 * 64 * 13)
    for name, fused in (("fused", True), ("unfused", False)):
        _, cx = B.ms_stem_forward(x, p, True, sm, out=e, fused=fused)
        out["first_level"][name] = {"fwd_us": _time_us(lambda: B.ms_stem_forward(x, p, True, B.Small(DEV), out=e, fused=fused), reps),
                                    "bwd_us": _time_us(lambda: B.ms_stem_backward(cx, de, {}, pre="enc1."), reps)}
        del cx
    # the reference's order: t written, read for the statistics, read for the apply, e written; backward: de, t read twice, dt written
    out["first_level"]["reference_order_fwd_MB"] = round((xb + 4 * eb) / 1e6, 1)
    out["first_level"]["fused_fwd_MB"] = round((2 * xb + eb) / 1e6, 1)
    out["first_level"]["avoided_tensor_MB"] = round(eb / 1e6, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.4, help="per configuration and round")
    ap.add_argument("--only", choices=("hip", "torch"), default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    if a.kernels:
        res = kernel_times(a.n, a.size, a.reps)
    else:
        st = mref.init_state(seed=0, perturb_bn=True)
        x, y = pkg.synthetic_batch(a.n, a.size, seed=1234)
        x, y = x.to(DEV), y.to(DEV)
        res = {"model": "MSWNet", "precision": "f32", "batch": a.n, "size": a.size, "device": torch.cuda.get_device_name(0)}
        if a.only != "torch":
            steps = {name: hip_step(st, x, y) for name, _ in CONFIGS}
            for name, fused in CONFIGS:
                set_config(fused)
                for _ in range(a.warmup):
                    steps[name]()
            rounds = {name: [] for name, _ in CONFIGS}
            loss = {}
            for _ in range(a.rounds):
                for name, fused in CONFIGS:
                    set_config(fused)
                    k, dt, loss[name] = run_for(steps[name], a.min_seconds)
                    rounds[name].append(1e3 * dt / k)
            set_config(True)
            for name, _ in CONFIGS:
                ms = statistics.median(rounds[name])
                res["hip" if name == "fused" else "hip_" + name] = {
                    "ms_per_step": round(ms, 3), "min_ms": round(min(rounds[name]), 3), "max_ms": round(max(rounds[name]), 3),
                    "rounds": [round(v, 3) for v in rounds[name]], "images_per_s": round(1e3 * a.n / ms, 1), "final_loss": round(loss[name], 5)}
            f, u = res["hip"], res["hip_unfused_ms_stem"]
            spread = max(f["max_ms"] - f["min_ms"], u["max_ms"] - u["min_ms"])
            res["stem_default"] = {"fused_minus_unfused_ms": round(f["ms_per_step"] - u["ms_per_step"], 3), "round_spread_ms": round(spread, 3),
                                   "fused_stays_default": bool(f["ms_per_step"] - u["ms_per_step"] <= spread)}
            del steps
            torch.cuda.empty_cache()
        if a.only != "hip":
            step = torch_step(st, x, y)
            for _ in range(a.warmup):
                step()
            k, dt, last = run_for(step, max(1.0, a.min_seconds))
            res["torch_eager"] = {"steps": k, "seconds": round(dt, 4), "ms_per_step": round(1e3 * dt / k, 3), "images_per_s": round(a.n * k / dt, 1),
                                  "final_loss": round(last, 5)}
        if "hip" in res and "torch_eager" in res:
            res["speedup_hip_over_torch_eager"] = round(res["torch_eager"]["ms_per_step"] / res["hip"]["ms_per_step"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
