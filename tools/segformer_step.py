"""SegFormer-Lite (Extended_Baseline_Comparison.py:622-744) train step on one MI355X, fp32, BCE + Adam(1e-4, weight decay 1e-4): the HIP
module (`SegFormerLite` + FusedAdam) against the CPU restatement tests/segformer_ref.py run eagerly on torch-ROCm on the same GPU (torch.optim.Adam),
same inputs and initial state.  Each is warmed up, then timed over at least --min-seconds of steps with the device synchronised before the clock
is read.  Prints one JSON line; --out also writes it to a file.

--kernels: single-stream times of the new kernels at the 16 x 256^2 stage shapes instead: the attention forward / backward with the bytes they
move and the HBM bandwidth that makes, the depthwise + GELU forward and weight gradient with z kept vs recomputed, and the data gradient of the
kernel = stride key / value reductions (RUNET_NO_LIVE_TAP_DGRAD=1 in the environment: through the general form, for the A/B).

Not a bench line of the contract (bench.py measures the Robust U-Net metric); the figures are quoted in DESIGN.md section 3.8.
  python tools/segformer_step.py [--n 16] [--size 256] [--warmup 5] [--min-seconds 1.0] [--only hip|torch] [--out FILE]
  python tools/segformer_step.py --kernels [--reps 50] [--out FILE]
"""
import argparse
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("eusipco-2026-robust-unet_amd")
fref = importlib.import_module("segformer_ref")
DEV = torch.device("cuda:0")


def timed(step, warmup, min_seconds):
    for _ in range(warmup):
        step()
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
    model = pkg.SegFormerLite()
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


def kernel_times(n, reps):
    sf = importlib.import_module("eusipco-2026-robust-unet_amd.segformer")
    ops = importlib.import_module("eusipco-2026-robust-unet_amd.ops")
    g = torch.Generator().manual_seed(0)
    out = {"batch": n, "device": torch.cuda.get_device_name(0), "attention": [], "dwconv": [], "reduction_dgrad": [],
           "live_tap_dgrad": os.environ.get("RUNET_NO_LIVE_TAP_DGRAD", "0") in ("", "0")}
    for (hw, c, heads, r, hid) in ((64, 32, 1, 8, 128), (32, 64, 2, 4, 256), (16, 128, 4, 2, 512)):
        hr = hw // r
        q = torch.randn((n, hw, hw, c), generator=g).to(DEV)
        kv = torch.randn((n, hr, hr, 2 * c), generator=g).to(DEV)
        do = torch.randn((n, hw, hw, c), generator=g).to(DEV)
        o, lse = sf.kv_attention(q, kv, heads)
        fwd = _time_us(lambda: sf.kv_attention(q, kv, heads), reps)
        bwd = _time_us(lambda: sf.kv_attention_backward(q, kv, o, lse, do, heads), reps)
        act, kvb, lseb = 4 * q.numel(), 4 * kv.numel(), 4 * lse.numel()
        ws = 4 * importlib.import_module("eusipco-2026-robust-unet_amd._lib").lib.runet_kv_attention_bwd_workspace_floats(n, hw * hw, hr * hr, c, heads)
        fb, bb = 2 * act + kvb + lseb, 4 * act + 2 * kvb + lseb + 2 * ws          # fwd: q, kv in, o, lse out; bwd: q, o, dO, kv, lse in, dq, dkv out, slots
        out["attention"].append({"q": list(q.shape), "kv": list(kv.shape), "heads": heads, "fwd_us": fwd, "fwd_MB": round(fb / 1e6, 1),
                                 "fwd_TB_per_s": round(fb / fwd / 1e6, 2), "bwd_us": bwd, "bwd_MB": round(bb / 1e6, 1),
                                 "bwd_TB_per_s": round(bb / bwd / 1e6, 2)})
        x = torch.randn((n, hw, hw, hid), generator=g).to(DEV)
        w3 = (torch.randn((3, 3, 1, hid), generator=g) / 3).to(DEV)
        b = torch.randn(hid, generator=g).to(DEV)
        da = torch.randn((n, hw, hw, hid), generator=g).to(DEV)
        z, _ = sf.dwconv_gelu(x, w3, b, keep_z=True)
        out["dwconv"].append({"x": list(x.shape),
                              "fwd_keep_z_us": _time_us(lambda: sf.dwconv_gelu(x, w3, b, keep_z=True), reps),
                              "fwd_no_z_us": _time_us(lambda: sf.dwconv_gelu(x, w3, b, keep_z=False), reps),
                              "bwd_read_z_us": _time_us(lambda: sf.dwconv_gelu_backward(x, z, da.clone(), w3, b), reps),
                              "bwd_recompute_z_us": _time_us(lambda: sf.dwconv_gelu_backward(x, None, da.clone(), w3, b), reps),
                              "clone_of_da_us": _time_us(lambda: da.clone(), reps)})
        dy = torch.randn((n, hr, hr, c), generator=g).to(DEV)
        wr = torch.randn((r, r, c, c), generator=g).to(DEV)
        out["reduction_dgrad"].append({"dy": list(dy.shape), "dx": [n, hw, hw, c], "kernel_stride": r,
                                       "us": _time_us(lambda: ops.conv_general_dgrad(dy, wr, hw, hw, r, 0), reps)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--only", choices=("hip", "torch"), default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    if a.kernels:
        line = json.dumps(kernel_times(a.n, a.reps))
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    st = fref.init_state(seed=0, perturb_bn=True)
    x, y = pkg.synthetic_batch(a.n, a.size, seed=1234)
    x, y = x.to(DEV), y.to(DEV)
    res = {"model": "SegFormerLite", "precision": "f32", "batch": a.n, "size": a.size, "device": torch.cuda.get_device_name(0)}
    for name, make in (("hip", hip_step), ("torch_eager", torch_step)):
        if a.only and not name.startswith(a.only):
            continue
        steps, dt, loss = timed(make(st, x, y), a.warmup, a.min_seconds)
        res[name] = {"steps": steps, "seconds": round(dt, 4), "ms_per_step": round(1e3 * dt / steps, 3),
                     "images_per_s": round(a.n * steps / dt, 1), "final_loss": round(loss, 5)}
        torch.cuda.empty_cache()
    if "hip" in res and "torch_eager" in res:
        res["speedup_hip_over_torch_eager"] = round(res["torch_eager"]["ms_per_step"] / res["hip"]["ms_per_step"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
