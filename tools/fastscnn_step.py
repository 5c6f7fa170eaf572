"""Fast-SCNN (comne.py:305-476) train step on one MI355X, fp32, BCE + Adam(1e-4, weight decay 1e-4): the HIP module (`FastSCNN` + FusedAdam)
against the CPU restatement tests/fastscnn_ref.py run eagerly on torch-ROCm on the same GPU (torch.optim.Adam), same inputs and initial state,
and against its own A/B partners.  The HIP configurations (every fusion on; the separable layers unfused; the feature fusion unfused - selected
here through the flags blocks.py reads RUNET_FUSED_DWSEP / RUNET_NO_FUSED_FFM into) are warmed up and then timed in interleaved rounds (fused,
no_fused_dwsep, no_fused_ffm, fused, ...), the device synchronised before the clock is read; the figure of a configuration is the median of
its rounds, with their min / max and quartiles.  "defaults": the rule the defaults of blocks.FUSED_DWSEP / FUSED_FFM follow - a fusion is the
default only if the fused median is not above its partner's by more than the larger interquartile range of the two configurations in this
run (min - max would let one slow round of the partner hide a steady difference).  Prints one JSON line; --out also writes it to a file.

--kernels: single-stream times of the new kernels at the shapes of the 16 x 256^2 step with the bytes each moves (derived from the tensor
sizes) and the HBM bandwidth that makes, the fused separable kernels beside their partners.
--launches: the kernel-launching C-ABI calls of one step per configuration, counted on the host by wrapping the binding's entries (an entry
launches one to three kernels, so this is a lower bound of the launch count; the size and workspace queries are not counted).

Not a bench line of the contract (bench.py measures the Robust U-Net metric); the figures are quoted in DESIGN.md.
  python tools/fastscnn_step.py [--n 16] [--size 256] [--warmup 20] [--rounds 5] [--min-seconds 0.4] [--only hip|torch] [--out FILE]
  python tools/fastscnn_step.py --kernels [--reps 50] [--out FILE]
  python tools/fastscnn_step.py --launches [--out FILE]
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
fref = importlib.import_module("fastscnn_ref")
DEV = torch.device("cuda:0")
CONFIGS = (("fused", (True, True)), ("no_fused_dwsep", (False, True)), ("no_fused_ffm", (True, False)))


def set_config(cfg):
    B.FUSED_DWSEP, B.FUSED_FFM = cfg


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
    model = pkg.FastSCNN()
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
    names = fref.param_names()
    P = {k: v.clone().to(DEV) for k, v in st.items()}
    params = [P[k].requires_grad_(True) for k in names]
    opt = torch.optim.Adam(params, lr=1e-4, weight_decay=1e-4)

    def step():
        opt.zero_grad()
        loss = torch.nn.functional.binary_cross_entropy(fref.forward(P, x, True), y)
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
    out = {"batch": n, "size": size, "device": torch.cuda.get_device_name(0), "kernels": []}
    st = ops.stream()

    def row(name, shape, us, nbytes):
        out["kernels"].append({"kernel": name, "shape": shape, "us": us, "MB": round(nbytes / 1e6, 2), "GB_per_s": round(nbytes / us / 1e3, 1)})

    def rnd(*shape):
        return torch.randn(shape, generator=g).to(DEV)

    # ---- the separable layers: the largest (dsconv1: 32 -> 48, stride 2, 128^2 -> 64^2) and the most frequent trunk shape (64 -> 64 at 32^2)
    for cin, cout, stride, h in ((32, 48, 2, size // 2), (64, 64, 1, size // 8), (128, 128, 1, size // 16)):
        ho = (h + stride - 1) // stride
        shape = f"{n}x{h}x{h} {cin}->{cout} s{stride}"
        x, wd, wp = rnd(n, h, h, cin), rnd(3, 3, 1, cin), rnd(1, 1, cin, cout)
        dy, dt = rnd(n, ho, ho, cin), rnd(n, ho, ho, cout)
        p = B.DWSepParams(wd, wp, None, stride)
        Pi, Po = 4 * n * h * h, 4 * n * ho * ho              # bytes of one channel's plane, input and output resolution
        row("runet_dw3_fwd", shape, _time_us(lambda: B.dw3_forward(x, wd, stride), reps), Pi * cin + Po * cin)
        row("runet_dw3_wgrad", shape, _time_us(lambda: B.dw3_wgrad(x, dy, stride), reps), Pi * cin + Po * cin)
        row("runet_dw3_dgrad", shape, _time_us(lambda: B.dw3_dgrad(dy, wd, h, h, stride), reps), Pi * cin + Po * cin)
        row("runet_dwsep_fwd", shape, _time_us(lambda: B.dwsep_conv(x, p, True, fused=True), reps), Pi * cin + Po * cout)
        row("partner: runet_dw3_fwd + 1x1 convolution", shape, _time_us(lambda: B.dwsep_conv(x, p, True, fused=False), reps),
            Pi * cin + 2 * Po * cin + Po * cout)
        d = B.dw3_forward(x, wd, stride)
        row("runet_dwsep_wgrad_pw", shape, _time_us(lambda: B.dwsep_wgrad_pw(x, wd, dt, stride), reps), Pi * cin + Po * cout)
        row("partner: 1x1 weight gradient on the kept tensor", shape, _time_us(lambda: ops.conv_wgrad(d, dt, 1, 1, on_side=False), reps),
            Po * cin + Po * cout)
    # ---- pyramid at the H/16 map
    h, c, cq = size // 16, 128, 32
    shape = f"{n}x{h}x{h}x{c}"
    cat, dcat = rnd(n, h, h, 2 * c), rnd(n, h, h, 2 * c)
    pooled, acts = rnd(50 * n, c), rnd(50 * n, cq)
    dx = torch.empty((n, h, h, c), device=DEV)
    xs, up, dup, direct = cat[..., :c], cat[..., c:], dcat[..., c:], dcat[..., :c]
    P = 4 * n * h * h
    row("runet_pyramid_pool_fwd", shape, _time_us(lambda: check(lib.runet_pyramid_pool_fwd(xs.data_ptr(), 2 * c, pooled.data_ptr(), c, n, h, h, c, st)), reps),
        P * c + 4 * 50 * n * c)
    row("runet_pyramid_pool_bwd", shape, _time_us(lambda: check(lib.runet_pyramid_pool_bwd(pooled.data_ptr(), c, direct.data_ptr(), 2 * c, dx.data_ptr(), c,
                                                                                           n, h, h, c, st)), reps), 2 * P * c + 4 * 50 * n * c)
    row("runet_pyramid_upsample_fwd", shape, _time_us(lambda: check(lib.runet_pyramid_upsample_fwd(acts.data_ptr(), cq, up.data_ptr(), 2 * c, n, h, h, cq, st)),
                                                      reps), P * c + 4 * 50 * n * cq)
    row("runet_pyramid_upsample_bwd", shape, _time_us(lambda: check(lib.runet_pyramid_upsample_bwd(dup.data_ptr(), 2 * c, acts.data_ptr(), cq, n, h, h, cq, st)),
                                                      reps), P * c + 4 * 50 * n * cq)
    # ---- fusion (high map H/16 -> H/8) and head (H/8 -> H)
    hl = size // 8
    tl, th, dy = rnd(n, hl, hl, c), rnd(n, h, h, c), rnd(n, hl, hl, c)
    co = tuple(rnd(c) for _ in range(4))
    for name, fused in (("runet_ffm_fwd", True), ("partner: bn_apply + bn_bilinear + add + relu", False)):
        row(name, f"{n}x{hl}x{hl}x{c}", _time_us(lambda: B.ffm_forward(tl, co[:2], th, co[2:], 2, fused=fused), reps),
            4 * n * c * (2 * hl * hl + h * h) if fused else 4 * n * c * (7 * hl * hl + h * h))
    y = B.ffm_forward(tl, co[:2], th, co[2:], 2)
    g_ = torch.empty_like(y)
    row("runet_relu_mask_nhwc", f"{n}x{hl}x{hl}x{c}", _time_us(lambda: check(lib.runet_relu_mask_nhwc(dy.data_ptr(), c, y.data_ptr(), c, g_.data_ptr(), c,
                                                                                                     n * hl * hl, c, st)), reps), 3 * 4 * n * c * hl * hl)
    z, dprob = rnd(n, hl, hl), rnd(n, 1, size, size)
    prob = B.up_sigmoid_forward(z, 8)
    row("runet_up_sigmoid_fwd", f"{n}x{hl}x{hl} x8", _time_us(lambda: B.up_sigmoid_forward(z, 8), reps), 4 * n * (hl * hl + size * size))
    row("runet_up_sigmoid_bwd", f"{n}x{hl}x{hl} x8", _time_us(lambda: B.up_sigmoid_backward(dprob, prob, 8), reps), 4 * n * (hl * hl + 2 * size * size))
    return out


def launch_counts(n, size):
    L = importlib.import_module("eusipco-2026-robust-unet_amd._lib")
    quiet = ("_workspace_floats", "_parts", "_supported", "_fits", "_elems", "_kernel_name", "_last_error", "_abi_version", "_stream_wait")
    calls = {}

    def counted(name, fn):
        def call(*a):
            calls[name] = calls.get(name, 0) + 1
            return fn(*a)
        return call
    for name in L.PROTOS:
        if not name.endswith(quiet):
            setattr(L.lib, name, counted(name, getattr(L.lib, name)))
    st = fref.init_state(seed=0, perturb_bn=True)
    x, y = pkg.synthetic_batch(n, size, seed=1234)
    x, y = x.to(DEV), y.to(DEV)
    out = {"batch": n, "size": size, "abi_calls_per_step": {}, "by_entry": {}}
    for name, cfg in CONFIGS:
        set_config(cfg)
        step = hip_step(st, x, y)
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        calls.clear()
        step()
        torch.cuda.synchronize()
        out["abi_calls_per_step"][name] = sum(calls.values())
        out["by_entry"][name] = dict(sorted(calls.items()))
    set_config((True, True))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.4, help="per configuration and round")
    ap.add_argument("--only", choices=("hip", "torch"), default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    if a.kernels:
        res = kernel_times(a.n, a.size, a.reps)
    elif a.launches:
        res = launch_counts(a.n, a.size)
    else:
        st = fref.init_state(seed=0, perturb_bn=True)
        x, y = pkg.synthetic_batch(a.n, a.size, seed=1234)
        x, y = x.to(DEV), y.to(DEV)
        res = {"model": "FastSCNN", "precision": "f32", "batch": a.n, "size": a.size, "device": torch.cuda.get_device_name(0)}
        if a.only != "torch":
            steps = {name: hip_step(st, x, y) for name, _ in CONFIGS}
            for name, cfg in CONFIGS:
                set_config(cfg)
                for _ in range(a.warmup):
                    steps[name]()
            rounds = {name: [] for name, _ in CONFIGS}
            loss = {}
            for _ in range(a.rounds):
                for name, cfg in CONFIGS:
                    set_config(cfg)
                    k, dt, loss[name] = run_for(steps[name], a.min_seconds)
                    rounds[name].append(1e3 * dt / k)
            set_config((True, True))
            for name, _ in CONFIGS:
                ms = statistics.median(rounds[name])
                q = statistics.quantiles(rounds[name], n=4) if len(rounds[name]) > 1 else [ms, ms, ms]
                res["hip" if name == "fused" else "hip_" + name] = {
                    "ms_per_step": round(ms, 3), "min_ms": round(min(rounds[name]), 3), "max_ms": round(max(rounds[name]), 3), "iqr_ms": round(q[2] - q[0], 3),
                    "rounds": [round(v, 3) for v in rounds[name]], "images_per_s": round(1e3 * a.n / ms, 1), "final_loss": round(loss[name], 5)}
            f = res["hip"]
            res["defaults"] = {}
            for switch, name in (("FUSED_DWSEP", "no_fused_dwsep"), ("FUSED_FFM", "no_fused_ffm")):
                u = res["hip_" + name]
                spread = max(f["iqr_ms"], u["iqr_ms"])
                res["defaults"][switch] = {"fused_minus_partner_ms": round(f["ms_per_step"] - u["ms_per_step"], 3), "round_iqr_ms": round(spread, 3),
                                           "fused_is_default": bool(f["ms_per_step"] - u["ms_per_step"] <= spread)}
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
