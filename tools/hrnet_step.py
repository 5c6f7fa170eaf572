"""HRNet-Water (Extended_Baseline_Comparison.py:554-616) train step on one MI355X, fp32, BCE + Adam(1e-4, weight decay 1e-4): the HIP module
(`HRNetWater` + FusedAdam) against the CPU restatement tests/hrnet_ref.py run eagerly on torch-ROCm on the same GPU (torch.optim.Adam), same
inputs and initial state, and against its own A/B partners.  The three HIP configurations (fused default, RUNET_NO_FUSED_HR_HEAD,
RUNET_NO_FUSED_BN_UPSAMPLE - selected here through the flags blocks.py reads those variables into) are warmed up and then timed in
interleaved rounds (fused, unfused head, unfused fusion branches, fused, ...), the device synchronised before the clock is read; the figure
of a configuration is the median of its rounds, the spread their min / max.  Prints one JSON line; --out also writes it to a file.

--kernels: single-stream times of the seven new kernels at the 16 x 256^2 shapes with the bytes each moves (derived from the tensor sizes) and
the HBM bandwidth that makes, and the head / fusion-branch forward + backward as a whole, fused against unfused.

Not a bench line of the contract (bench.py measures the Robust U-Net metric); the figures are quoted in DESIGN.md.
  python tools/hrnet_step.py [--n 16] [--size 256] [--warmup 5] [--rounds 5] [--min-seconds 0.4] [--only hip|torch] [--out FILE]
  python tools/hrnet_step.py --kernels [--reps 50] [--out FILE]
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
href = importlib.import_module("hrnet_ref")
DEV = torch.device("cuda:0")
CONFIGS = (("fused", True, True), ("unfused_head", False, True), ("unfused_bn_upsample", True, False))


def set_config(head, upsample):
    B.FUSED_HR_HEAD, B.FUSED_BN_UPSAMPLE = head, upsample


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
    model = pkg.HRNetWater()
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
    names = href.param_names()
    P = {k: v.clone().to(DEV) for k, v in st.items()}
    params = [P[k].requires_grad_(True) for k in names]
    opt = torch.optim.Adam(params, lr=1e-4, weight_decay=1e-4)

    def step():
        opt.zero_grad()
        loss = torch.nn.functional.binary_cross_entropy(href.forward(P, x, True), y)
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
    h = size // 2
    out = {"batch": n, "size": size, "device": torch.cuda.get_device_name(0), "kernels": [], "head": {}, "fusion": []}

    def row(name, us, nbytes):
        out["kernels"].append({"kernel": name, "us": us, "MB": round(nbytes / 1e6, 1), "GB_per_s": round(nbytes / us / 1e3, 1)})

    def vecs(c):
        return [torch.randn(c, generator=g).to(DEV) for _ in range(2)] + [torch.randn(c, generator=g).to(DEV) * 0.1,
                                                                         (torch.rand(c, generator=g) + 0.5).to(DEV)]
    # ---- head: t [n, h, h, 64]
    c = 64
    t = torch.randn((n, h, h, c), generator=g).to(DEV)
    sc, sh, mean, invstd = vecs(c)
    w, b = (torch.randn(c, generator=g) / 8).to(DEV), torch.zeros(1, device=DEV)
    dprob = torch.randn((n, 1, size, size), generator=g).to(DEV)
    z = torch.empty((n, h, h), device=DEV)
    dz = torch.empty((n, h, h), device=DEV)
    prob = torch.empty((n, 1, size, size), device=DEV)
    dt = torch.empty_like(t)
    res = torch.empty(3 * c + 1, device=DEV)
    ws = B.scratch(lib.runet_hr_head_bwd_workspace_floats(n, h, h, c), DEV)
    st = ops.stream()
    tb, zb = 4 * t.numel(), 4 * z.numel()
    row("runet_hr_head_fwd", _time_us(lambda: check(lib.runet_hr_head_fwd(t.data_ptr(), c, sc.data_ptr(), sh.data_ptr(), w.data_ptr(), b.data_ptr(),
                                                                          z.data_ptr(), n, h, h, c, st)), reps), tb + zb)
    row("runet_up2_sigmoid_fwd", _time_us(lambda: check(lib.runet_up2_sigmoid_fwd(z.data_ptr(), prob.data_ptr(), n, h, h, st)), reps), 5 * zb)
    row("runet_up2_sigmoid_bwd", _time_us(lambda: check(lib.runet_up2_sigmoid_bwd(dprob.data_ptr(), prob.data_ptr(), dz.data_ptr(), n, h, h, st)), reps), 9 * zb)
    row("runet_hr_head_bwd_reduce", _time_us(lambda: check(lib.runet_hr_head_bwd_reduce(dz.data_ptr(), t.data_ptr(), c, sc.data_ptr(), sh.data_ptr(), w.data_ptr(),
                                                                                        mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(), ws.numel(),
                                                                                        res.data_ptr(), n, h, h, c, st)), reps), tb + zb)
    row("runet_hr_head_bwd_apply", _time_us(lambda: check(lib.runet_hr_head_bwd_apply(dz.data_ptr(), t.data_ptr(), c, w.data_ptr(), dt.data_ptr(), c, n, h, h, c,
                                                                                      mean.data_ptr(), invstd.data_ptr(), sc.data_ptr(), sh.data_ptr(),
                                                                                      res.data_ptr(), 0, st)), reps), 2 * tb + zb)
    for name, fused in (("fused", True), ("unfused", False)):
        p, saved = B.hr_head_forward(t, sc, sh, w, b, fused=fused)
        out["head"][name] = {"fwd_us": _time_us(lambda: B.hr_head_forward(t, sc, sh, w, b, fused=fused), reps),
                             "bwd_us": _time_us(lambda: B.hr_head_backward(dprob, p, t, sc, sh, w, mean, invstd, saved=saved), reps)}
        del p, saved
    out["head"]["avoided_tensor_MB"] = round(4 * n * size * size * c / 1e6, 1)
    # ---- fusion branches: x [n, h / s, h / s, 48] -> channels of the 144-wide concat at [n, h, h]
    c = 48
    cat = torch.empty((n, h, h, 144), device=DEV)
    dcat = torch.randn((n, h, h, 144), generator=g).to(DEV)
    for j, s in enumerate((2, 4)):
        hs = h // s
        x = torch.randn((n, hs, hs, c), generator=g).to(DEV)
        sc, sh, mean, invstd = vecs(c)
        y, dy = cat[..., 48 * (j + 1):48 * (j + 2)], dcat[..., 48 * (j + 1):48 * (j + 2)]
        gbuf = torch.empty_like(x)
        sums = torch.empty(2 * c, device=DEV)
        ws = B.scratch(lib.runet_bilinear_nhwc_bwd_sums_workspace_floats(n, hs, hs, c), DEV)
        xb = 4 * x.numel()
        row(f"runet_bn_bilinear_nhwc_fwd x{s}", _time_us(lambda: check(lib.runet_bn_bilinear_nhwc_fwd(x.data_ptr(), c, y.data_ptr(), 144, sc.data_ptr(), sh.data_ptr(),
                                                                                                      n, hs, hs, s, c, st)), reps), xb * (1 + s * s))
        row(f"runet_bilinear_nhwc_bwd_sums x{s}", _time_us(lambda: check(lib.runet_bilinear_nhwc_bwd_sums(dy.data_ptr(), 144, x.data_ptr(), c, mean.data_ptr(),
                                                                                                          invstd.data_ptr(), gbuf.data_ptr(), c, ws.data_ptr(),
                                                                                                          ws.numel(), sums.data_ptr(), n, hs, hs, s, c, st)), reps),
            xb * (2 + s * s))
        ent = {"scale": s, "x": list(x.shape)}
        for name, fused in (("fused", True), ("unfused", False)):
            ent[name] = {"fwd_us": _time_us(lambda: B.bn_bilinear_forward(x, sc, sh, y, s, fused=fused), reps),
                         "bwd_us": _time_us(lambda: B.bn_bilinear_backward(dy, x, mean, invstd, sc, sums, s, fused=fused), reps)}
        out["fusion"].append(ent)
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
        st = href.init_state(seed=0, perturb_bn=True)
        x, y = pkg.synthetic_batch(a.n, a.size, seed=1234)
        x, y = x.to(DEV), y.to(DEV)
        res = {"model": "HRNetWater", "precision": "f32", "batch": a.n, "size": a.size, "device": torch.cuda.get_device_name(0)}
        if a.only != "torch":
            steps = {name: hip_step(st, x, y) for name, _, _ in CONFIGS}
            for name, head, up in CONFIGS:
                set_config(head, up)
                for _ in range(a.warmup):
                    steps[name]()
            rounds = {name: [] for name, _, _ in CONFIGS}
            loss = {}
            for _ in range(a.rounds):
                for name, head, up in CONFIGS:
                    set_config(head, up)
                    k, dt, loss[name] = run_for(steps[name], a.min_seconds)
                    rounds[name].append(1e3 * dt / k)
            set_config(True, True)
            for name, _, _ in CONFIGS:
                ms = statistics.median(rounds[name])
                res["hip" if name == "fused" else "hip_" + name] = {
                    "ms_per_step": round(ms, 3), "min_ms": round(min(rounds[name]), 3), "max_ms": round(max(rounds[name]), 3),
                    "rounds": [round(v, 3) for v in rounds[name]], "images_per_s": round(1e3 * a.n / ms, 1), "final_loss": round(loss[name], 5)}
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
