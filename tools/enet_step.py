"""ENet (comne.py:482-608) train step on one MI355X, fp32, BCE + Adam(1e-4, weight decay 1e-4): the HIP module (`ENet` + FusedAdam) against
the CPU restatement tests/enet_ref.py run eagerly on torch-ROCm on the same GPU (torch.optim.Adam), same inputs and initial state, and against
its own A/B partners.  The HIP configurations (every fusion on; the initial block from shared kernels; the bottleneck tail from shared kernels -
selected here through the flags blocks.py reads RUNET_NO_FUSED_ENET_INITIAL / RUNET_NO_FUSED_ENET_TAIL into) are warmed up and then timed in
interleaved rounds (fused, no_fused_initial, no_fused_tail, fused, ...), the device synchronised before the clock is read; the figure of a
configuration is the median of its rounds, with their min / max and quartiles.  "defaults": the rule the defaults of blocks.FUSED_ENET_INITIAL /
FUSED_ENET_TAIL follow - a fusion is the default only if the fused median is not above its partner's by more than the larger interquartile
range of the two configurations in this run.  Prints one JSON line; --out also writes it to a file.

--kernels: single-stream times of the new kernels at the shapes of the 16 x 256^2 step beside their partners, with the bytes each moves
(derived from the tensor sizes) and the HBM bandwidth that makes; and "step_calls": every kernel-launching C-ABI call of one default step timed
with a pair of HIP events on one stream (weight gradients kept on the main stream for this), the twelve most expensive listed with their integer
arguments, and the rank of the two k3-s2 transposed forwards among them ("convt3_fwd_rank_and_us": as the data gradient of a stride-2
convolution they were the step's two most expensive launches, which is why runet_convt3_fwd exists).
--launches: the kernel-launching C-ABI calls of one step per configuration, counted on the host by wrapping the binding's entries.

Not a bench line of the contract (bench.py measures the Robust U-Net metric); the figures are quoted in DESIGN.md.
  python tools/enet_step.py [--n 16] [--size 256] [--warmup 20] [--rounds 5] [--min-seconds 0.4] [--only hip|torch] [--out FILE]
  python tools/enet_step.py --kernels [--reps 50] [--out FILE]
  python tools/enet_step.py --launches [--out FILE]
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
eref = importlib.import_module("enet_ref")
DEV = torch.device("cuda:0")
CONFIGS = (("fused", (True, True)), ("no_fused_initial", (False, True)), ("no_fused_tail", (True, False)))
QUIET = ("_workspace_floats", "_parts", "_supported", "_fits", "_elems", "_kernel_name", "_last_error", "_abi_version", "_stream_wait")


def set_config(cfg):
    B.FUSED_ENET_INITIAL, B.FUSED_ENET_TAIL = cfg


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
    model = pkg.ENet()
    model.load_state_dict(st, strict=True)
    model.to(DEV).train()          # Dropout2d masks are drawn per step, as in training
    opt = pkg.FusedAdam(model.parameters(), lr=1e-4, weight_decay=1e-4)

    def step():
        opt.zero_grad()
        loss = pkg.bce_loss(model(x), y)
        loss.backward()
        opt.step()
        return loss
    return step


def torch_step(st, x, y):
    names = eref.param_names()
    P = {k: v.clone().to(DEV) for k, v in st.items()}
    params = [P[k].requires_grad_(True) for k in names]
    opt = torch.optim.Adam(params, lr=1e-4, weight_decay=1e-4)
    n = x.shape[0]

    def step():
        opt.zero_grad()
        masks = {name: torch.empty((n, cout), device=DEV).bernoulli_(1 - p).div_(1 - p) for name, _, cout, _, _, _, p in eref.BLOCKS}
        loss = torch.nn.functional.binary_cross_entropy(eref.forward(P, x, True, masks), y)
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


def step_calls(n, size):
    """every kernel-launching C-ABI call of one default step, timed by a pair of events (one stream) -> the twelve most expensive and the total"""
    ops = importlib.import_module("eusipco-2026-robust-unet_amd.ops")
    L = importlib.import_module("eusipco-2026-robust-unet_amd._lib")
    ops.USE_WGRAD_STREAM = False
    st = eref.init_state(seed=0, perturb_bn=True)
    x, y = pkg.synthetic_batch(n, size, seed=1234)
    step = hip_step(st, x.to(DEV), y.to(DEV))
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    rec, real = [], {}

    def timed(name, fn):
        def call(*a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a)
            e1.record()
            # the k3-s2 transposed forward: runet_convt3_fwd, or under RUNET_NO_CONVT3_CLASSES=1 runet_conv2d_general with kh, kw, stride, pad, dil, mode =
            # 3, 3, 2, 1, 1, RUNET_CONV_DGRAD
            k3s2 = name == "runet_convt3_fwd" or (name == "runet_conv2d_general" and tuple(a[12:18]) == (3, 3, 2, 1, 1, 1))
            rec.append((name, [v for v in a if isinstance(v, int) and not isinstance(v, bool) and abs(v) < 1 << 20], e0, e1, k3s2))
            return r
        return call
    for name in L.PROTOS:
        if not name.endswith(QUIET):
            real[name] = getattr(L.lib, name)
            setattr(L.lib, name, timed(name, real[name]))
    step()
    torch.cuda.synchronize()
    for name, fn in real.items():
        setattr(L.lib, name, fn)
    rows = sorted(((round(1e3 * e0.elapsed_time(e1), 1), name, ints, k3s2) for name, ints, e0, e1, k3s2 in rec), reverse=True)
    return {"calls": len(rows), "sum_us": round(sum(r[0] for r in rows), 1), "top": [{"us": us, "entry": name, "ints": ints} for us, name, ints, _ in rows[:12]],
            "convt3_fwd_rank_and_us": [{"rank": i + 1, "us": us} for i, (us, _, _, k3s2) in enumerate(rows) if k3s2]}


def kernel_times(n, size, reps):
    ops = importlib.import_module("eusipco-2026-robust-unet_amd.ops")
    g = torch.Generator().manual_seed(0)
    out = {"batch": n, "size": size, "device": torch.cuda.get_device_name(0), "kernels": []}

    def row(name, shape, us, nbytes):
        out["kernels"].append({"kernel": name, "shape": shape, "us": us, "MB": round(nbytes / 1e6, 2), "GB_per_s": round(nbytes / us / 1e3, 1)})

    def rnd(*shape):
        return torch.randn(shape, generator=g).to(DEV)

    def bn(c):
        return B.BNState(torch.ones(c, device=DEV), torch.zeros(c, device=DEV), torch.zeros(c, device=DEV), torch.ones(c, device=DEV),
                         torch.zeros((), dtype=torch.int64, device=DEV))
    # ---- initial block: forward (convolution + pool + statistics + apply) and backward, fused and partner
    x, w13, da = rnd(n, 3, size, size), rnd(3, 3, 3, 13), rnd(n, size // 2, size // 2, 16)
    P2 = 4 * n * (size // 2) ** 2
    for name, fused in (("runet_enet_initial_fwd + finalize + bn_apply", True), ("partner: to_nhwc_pad, conv, pool, copy, bn_stats, bn_apply", False)):
        sm = B.Small(DEV)
        row(name, f"{n}x3x{size}x{size}", _time_us(lambda: B.enet_initial_forward(x, w13, bn(16), True, sm, fused=fused), reps),
            4 * n * 3 * size * size + 3 * P2 * 16 if fused else 4 * n * 7 * size * size + P2 * (16 + 4 + 3 + 16 + 32))
        _, cx = B.enet_initial_forward(x, w13, bn(16), True, sm, fused=fused)
        row(("runet_enet_initial_wgrad" if fused else "partner: runet_conv_wgrad_general") + " + bn_backward", f"{n}x3x{size}x{size}",
            _time_us(lambda: B.enet_initial_backward(cx, da.clone(), {}, "", True), reps), 0)
    # ---- tail at encoder1 (64 channels, H/4) and encoder2 (128 channels, H/8), plain and downsample, forward and backward
    for c, h in ((64, size // 4), (128, size // 8)):
        t3, idn, dout, mask = rnd(n, h, h, c), rnd(n, h, h, c), rnd(n, h, h, c), torch.ones((n, c), device=DEV)
        co = tuple(rnd(c) for _ in range(4))
        T = 4 * n * h * h * c
        for down in (False, True):
            for fused in (True, False):
                tag = ("runet_enet_tail" if fused else "partner: shared kernels") + (" downsample" if down else " plain")
                cd = (co[0], co[1]) if down else None
                row(tag + " fwd", f"{n}x{h}x{h}x{c}", _time_us(lambda: B.enet_tail_forward(t3, (co[0], co[1]), idn, cd, mask, fused=fused), reps),
                    3 * T if fused else (9 if down else 7) * T)
                o = B.enet_tail_forward(t3, (co[0], co[1]), idn, cd, mask, fused=fused)
                sd = (co[2], co[3], co[0]) if down else None
                row(tag + " bwd", f"{n}x{h}x{h}x{c}",
                    _time_us(lambda: B.enet_tail_backward(dout, o, t3, (co[2], co[3], co[0]), idn if down else None, sd, mask, True, fused=fused), reps),
                    ((4 if down else 3) + (5 if down else 4) + 1) * T if fused else (3 + 2 + 5 + (5 if down else 0)) * T)
    # ---- head and the k3-s2 transposed convolutions
    h = size // 2
    xh, w6, b6, dprob = rnd(n, h, h, 16), rnd(2, 2, 16, 1), rnd(1), rnd(n, 1, size, size)
    prob = B.enet_head_forward(xh, w6, b6)
    row("runet_enet_head_fwd", f"{n}x{h}x{h}x16", _time_us(lambda: B.enet_head_forward(xh, w6, b6), reps), 4 * n * (16 * h * h + size * size))
    row("runet_enet_head_bwd", f"{n}x{h}x{h}x16", _time_us(lambda: B.enet_head_backward(dprob, prob, xh, w6, B.DictSink(DEV)), reps),
        4 * n * (32 * h * h + 2 * size * size))
    for cin, cout, hh in ((128, 64, size // 8), (64, 16, size // 4)):
        xt, dyt = rnd(n, hh, hh, cin), rnd(n, 2 * hh, 2 * hh, cout)
        wt = torch.nn.Parameter(torch.empty(3, 3, cin, cout).normal_(generator=g).permute(2, 3, 0, 1)).to(DEV)
        w = ops.hwio_t(wt)
        nb = 4 * n * hh * hh * (cin + 4 * cout)
        row("convt3_fwd (runet_convt3_fwd, four parity-class GEMMs)", f"{n}x{hh}x{hh} {cin}->{cout}",
            _time_us(lambda: ops.convt3_fwd(xt, w, None, classes=True), reps), nb)
        row("partner: convt3_fwd (runet_conv2d_general, data-gradient mode)", f"{n}x{hh}x{hh} {cin}->{cout}",
            _time_us(lambda: ops.convt3_fwd(xt, w, None, classes=False), reps), nb)
        row("convt3_dgrad (runet_conv2d_general, forward mode)", f"{n}x{hh}x{hh} {cin}->{cout}", _time_us(lambda: ops.convt3_dgrad(dyt, w), reps), nb)
        row("convt3_wgrad (runet_conv_wgrad_general + transpose)", f"{n}x{hh}x{hh} {cin}->{cout}", _time_us(lambda: ops.convt3_wgrad(xt, dyt), reps), nb)
    # ---- the asymmetric pair at encoder2
    h = size // 8
    xr, w51, dyr = rnd(n, h, h, 32), rnd(5, 1, 32, 32), rnd(n, h, h, 32)
    nb = 4 * n * h * h * 64
    row("runet_conv2d_rect (5, 1) fwd", f"{n}x{h}x{h} 32->32", _time_us(lambda: ops.conv_rect_fwd(xr, w51, None, 1, (2, 0)), reps), nb)
    row("runet_conv2d_rect (5, 1) dgrad", f"{n}x{h}x{h} 32->32", _time_us(lambda: ops.conv_rect_dgrad(dyr, w51, h, h, 1, (2, 0)), reps), nb)
    row("runet_conv_wgrad_rect (5, 1)", f"{n}x{h}x{h} 32->32", _time_us(lambda: ops.conv_rect_wgrad(xr, dyr, 5, 1, 1, (2, 0)), reps), nb)
    out["step_calls"] = step_calls(n, size)
    return out


def launch_counts(n, size):
    L = importlib.import_module("eusipco-2026-robust-unet_amd._lib")
    calls = {}

    def counted(name, fn):
        def call(*a):
            calls[name] = calls.get(name, 0) + 1
            return fn(*a)
        return call
    for name in L.PROTOS:
        if not name.endswith(QUIET):
            setattr(L.lib, name, counted(name, getattr(L.lib, name)))
    st = eref.init_state(seed=0, perturb_bn=True)
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
        st = eref.init_state(seed=0, perturb_bn=True)
        x, y = pkg.synthetic_batch(a.n, a.size, seed=1234)
        x, y = x.to(DEV), y.to(DEV)
        res = {"model": "ENet", "precision": "f32", "batch": a.n, "size": a.size, "device": torch.cuda.get_device_name(0)}
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
            for switch, name in (("FUSED_ENET_INITIAL", "no_fused_initial"), ("FUSED_ENET_TAIL", "no_fused_tail")):
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
