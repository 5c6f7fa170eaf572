"""PSPNet (comne.py:214-299) train step on one MI355X, fp32, BCE + Adam(1e-4, weight decay 1e-4): the HIP module (`PSPNet` + FusedAdam) against
the CPU restatement tests/pspnet_ref.py run eagerly on torch-ROCm on the same GPU (torch.optim.Adam), same inputs and initial state, and against
its own A/B partners.  The four HIP configurations (tap planes x fused head, selected here through the flags blocks.py reads
RUNET_NO_FUSED_PSP_TAPS / RUNET_NO_FUSED_PSP_HEAD into) are warmed up and then timed in interleaved rounds (taps+head, head, taps, partners,
taps+head, ...), the device synchronised before the clock is read; the figure of a configuration is the median of its rounds, with their
min / max and quartiles.  "defaults": the rule the defaults of blocks.FUSED_PSP_TAPS / FUSED_PSP_HEAD follow - a fusion is the default only if
the step with it is faster than the step without it, with the other switch in either position, by MORE than the round-to-round spread
(max - min over the rounds) of either of the two configurations compared in this run; otherwise it ships opt-in.
Prints one JSON line; --out also writes it to a file.  Reads nothing outside the repository.

--kernels: single-stream times of the three new kernel families at the shapes of the 16 x 256^2 step (H/16 map 16 x 16, 512 channels) beside
the partner launches they replace: final_conv.0 forward (four Z GEMMs + runet_psp_taps_fwd + the 512 -> 512 convolution, against
runet_pyramid_upsample_fwd + the 1024 -> 512 convolution), its backward (runet_psp_taps_bwd + the small GEMMs + the 512-channel data and
weight gradients + the join, against the 1024-channel ones + runet_pyramid_upsample_bwd), and the head forward and backward; and the new
entries alone.

Not a bench line of the contract (bench.py measures the Robust U-Net metric); the figures are quoted in DESIGN.md.
  python tools/pspnet_step.py [--n 16] [--size 256] [--warmup 20] [--rounds 5] [--min-seconds 0.4] [--only hip|torch] [--out FILE]
  python tools/pspnet_step.py --kernels [--reps 50] [--out FILE]
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
pref = importlib.import_module("pspnet_ref")
DEV = torch.device("cuda:0")
# (FUSED_PSP_TAPS, FUSED_PSP_HEAD)
CONFIGS = (("taps_head", (True, True)), ("head_only", (False, True)), ("taps_only", (True, False)), ("partners", (False, False)))


def set_config(cfg):
    B.FUSED_PSP_TAPS, B.FUSED_PSP_HEAD = cfg


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
    model = pkg.PSPNet()
    model.load_state_dict(st, strict=True)
    model.to(DEV).train()          # the Dropout2d mask is drawn per step, as in training
    opt = pkg.FusedAdam(model.parameters(), lr=1e-4, weight_decay=1e-4)

    def step():
        opt.zero_grad()
        loss = pkg.bce_loss(model(x), y)
        loss.backward()
        opt.step()
        return loss
    return step


def torch_step(st, x, y):
    names = pref.param_names()
    P = {k: v.clone().to(DEV) for k, v in st.items()}
    params = [P[k].requires_grad_(True) for k in names]
    opt = torch.optim.Adam(params, lr=1e-4, weight_decay=1e-4)
    n = x.shape[0]

    def step():
        opt.zero_grad()
        masks = {"final_conv.3": torch.empty((n, pref.C), device=DEV).bernoulli_(1 - pref.DROP_P).div_(1 - pref.DROP_P)}
        loss = torch.nn.functional.binary_cross_entropy(pref.forward(P, x, True, masks), y)
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
    ops.USE_WGRAD_STREAM = False          # single stream: the weight gradients inside the timed span
    g = torch.Generator().manual_seed(0)
    h = size // 16
    c, cq = 512, 128
    out = {"batch": n, "size": size, "map": [h, h], "device": torch.cuda.get_device_name(0), "kernels": []}

    def row(name, us):
        out["kernels"].append({"kernel": name, "shape": f"{n}x{h}x{h}", "us": us})

    def rnd(*shape):
        return torch.randn(shape, generator=g).to(DEV)
    w_full = rnd(3, 3, 2 * c, c) / (2 * c * 9) ** 0.5
    wx, wp = B.psp_split_weights(w_full, {})
    x, acts, bias, dt = rnd(n, h, h, c), rnd(50 * n, cq), rnd(c), rnd(n, h, h, c)
    cat = rnd(n, h, h, 2 * c)
    st = ops.stream()

    def taps_fwd():
        return B.psp_taps_forward(ops.conv_fwd(x, wx, bias), acts, wp)

    def partner_fwd():
        up = cat[..., c:]
        check(lib.runet_pyramid_upsample_fwd(acts.data_ptr(), cq, up.data_ptr(), ops.ld(up), n, h, h, cq, st))
        return ops.conv_fwd(cat, w_full, bias)

    def taps_bwd():
        dwx = ops.conv_wgrad(x, dt, 3, 3)
        dacts, dwp = B.psp_taps_backward(dt, acts, wp)
        return B.psp_join_wgrad(dwx, dwp), dacts, ops.conv_dgrad(dt, wx)

    def partner_bwd():
        dw = ops.conv_wgrad(cat, dt, 3, 3)
        dcat = ops.conv_dgrad(dt, w_full)
        dup = dcat[..., c:]
        dacts = torch.empty((50 * n, cq), device=DEV)
        check(lib.runet_pyramid_upsample_bwd(dup.data_ptr(), ops.ld(dup), dacts.data_ptr(), cq, n, h, h, cq, st))
        return dw, dacts, dcat
    row("final_conv.0 forward, tap planes: conv 512->512 + 4 Z GEMMs + runet_psp_taps_fwd", _time_us(taps_fwd, reps))
    row("final_conv.0 forward, partner: runet_pyramid_upsample_fwd + conv 1024->512", _time_us(partner_fwd, reps))
    row("final_conv.0 backward, tap planes: wgrad/dgrad 512 + runet_psp_taps_bwd + 4 dWtap GEMMs + runet_psp_taps_dp + join", _time_us(taps_bwd, reps))
    row("final_conv.0 backward, partner: wgrad/dgrad 1024 + runet_pyramid_upsample_bwd", _time_us(partner_bwd, reps))
    # the new tap entries alone
    z, t = rnd(50 * n, 9 * c), rnd(n, h, h, c)
    row("runet_psp_taps_fwd alone", _time_us(lambda: check(lib.runet_psp_taps_fwd(z.data_ptr(), 9 * c, t.data_ptr(), c, n, h, h, c, st)), reps))
    ws = torch.empty(lib.runet_psp_taps_bwd_workspace_floats(n, h, h, c), device=DEV)
    row("runet_psp_taps_bwd alone (columns + rows)",
        _time_us(lambda: check(lib.runet_psp_taps_bwd(dt.data_ptr(), c, z.data_ptr(), 9 * c, ws.data_ptr(), ws.numel(), n, h, h, c, st)), reps))
    row("conv 512->512 3x3 forward alone", _time_us(lambda: ops.conv_fwd(x, wx, bias), reps))
    row("conv 1024->512 3x3 forward alone", _time_us(lambda: ops.conv_fwd(cat, w_full, bias), reps))
    row("conv 512->512 3x3 data + weight gradient alone", _time_us(lambda: (ops.conv_wgrad(x, dt, 3, 3), ops.conv_dgrad(dt, wx)), reps))
    row("conv 1024->512 3x3 data + weight gradient alone", _time_us(lambda: (ops.conv_wgrad(cat, dt, 3, 3), ops.conv_dgrad(dt, w_full)), reps))
    # the small GEMMs of the tap planes, four launches each: rows 16 / 64 / 144 / 576 (n b^2), 128 x 4608
    pv = B._pyr_view
    dacts, dwp = torch.empty_like(acts), torch.empty_like(wp)
    wj = [wp[:, :, j * cq:(j + 1) * cq, :] for j in range(4)]
    row("4 Z GEMMs (ops.conv_fwd, P_j [n b^2, 128] x [128, 4608])", _time_us(lambda: [ops.conv_fwd(pv(acts, j, n), wj[j], None, out=pv(z, j, n)) for j in range(4)], reps))
    wsd = torch.empty(lib.runet_psp_taps_dp_workspace_floats(n, cq), device=DEV)
    row("runet_psp_taps_dp alone (dP of the four branches: per-tap partials + sum)",
        _time_us(lambda: check(lib.runet_psp_taps_dp(z.data_ptr(), 9 * c, wp.data_ptr(), 9 * c, wsd.data_ptr(), wsd.numel(), dacts.data_ptr(), cq, n, cq, c, st)), reps))
    row("what it replaces: 4 dP GEMMs (ops.conv_dgrad, dZ_j [n b^2, 4608] x [4608, 128])",
        _time_us(lambda: [ops.conv_dgrad(pv(z, j, n), wj[j], out=pv(dacts, j, n)) for j in range(4)], reps))
    row("4 dWtap GEMMs (ops.conv_wgrad, [128, n b^2] x [n b^2, 4608])",
        _time_us(lambda: [ops.conv_wgrad(pv(acts, j, n), pv(z, j, n), 1, 1, out=dwp[:, :, j * cq:(j + 1) * cq, :]) for j in range(4)], reps))
    dwx = torch.empty_like(wx)
    row("join of the two weight-gradient halves (two strided copies)", _time_us(lambda: B.psp_join_wgrad(dwx, dwp), reps))
    row("split of the weight into its halves (two strided copies, once per step)", _time_us(lambda: B.psp_split_weights(w_full, {}), reps))
    # ---- head
    sc, sh, mean, invstd = 1 + 0.1 * rnd(c), 0.1 * rnd(c), 0.1 * rnd(c), 1 + 0.1 * rnd(c).abs()
    mask = torch.empty((n, c), device=DEV).bernoulli_(0.9).div_(0.9)
    wo, bo, dprob = rnd(1, 1, c, 1) / c ** 0.5, rnd(1), rnd(n, 1, size, size)
    for name, fused in (("runet_psp_head_*", True), ("partner: runet_bn_apply + runet_outc_*", False)):
        prob, saved = B.psp_head_forward(t, sc, sh, mask, wo, bo, fused=fused)
        row(f"head forward, {name} (+ runet_up_sigmoid_fwd)", _time_us(lambda: B.psp_head_forward(t, sc, sh, mask, wo, bo, fused=fused), reps))
        row(f"head backward, {name} (+ runet_up_sigmoid_bwd)",
            _time_us(lambda: B.psp_head_backward(dprob, prob, t, sc, sh, mask, wo, mean, invstd, saved, True), reps))
    zz = rnd(n, h, h)
    row("runet_up_sigmoid_fwd alone (factor 16; both paths)", _time_us(lambda: B.up_sigmoid_forward(zz, B.PSP_HEAD_SCALE), reps))
    row("runet_up_sigmoid_bwd alone (factor 16; both paths)", _time_us(lambda: B.up_sigmoid_backward(dprob, prob, B.PSP_HEAD_SCALE), reps))
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
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    if a.kernels:
        res = kernel_times(a.n, a.size, a.reps)
    else:
        st = pref.init_state(seed=0, perturb_bn=True)
        x, y = pkg.synthetic_batch(a.n, a.size, seed=1234)
        x, y = x.to(DEV), y.to(DEV)
        res = {"model": "PSPNet", "precision": "f32", "batch": a.n, "size": a.size, "device": torch.cuda.get_device_name(0)}
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
                res["hip_" + name] = {
                    "ms_per_step": round(ms, 3), "min_ms": round(min(rounds[name]), 3), "max_ms": round(max(rounds[name]), 3), "iqr_ms": round(q[2] - q[0], 3),
                    "spread_ms": round(max(rounds[name]) - min(rounds[name]), 3), "rounds": [round(v, 3) for v in rounds[name]],
                    "images_per_s": round(1e3 * a.n / ms, 1), "final_loss": round(loss[name], 5)}
            res["defaults"] = {}
            pairs = {"FUSED_PSP_TAPS": (("taps_head", "head_only"), ("taps_only", "partners")),
                     "FUSED_PSP_HEAD": (("taps_head", "taps_only"), ("head_only", "partners"))}
            for switch, ps in pairs.items():
                rows = []
                for on, off in ps:
                    f, u = res["hip_" + on], res["hip_" + off]
                    spread = max(f["spread_ms"], u["spread_ms"])
                    rows.append({"with": on, "without": off, "gain_ms": round(u["ms_per_step"] - f["ms_per_step"], 3), "spread_ms": round(spread, 3),
                                 "wins": bool(u["ms_per_step"] - f["ms_per_step"] > spread)})
                res["defaults"][switch] = {"pairs": rows, "fused_is_default": all(r["wins"] for r in rows)}
            del steps
            torch.cuda.empty_cache()
        if a.only != "hip":
            step = torch_step(st, x, y)
            for _ in range(a.warmup):
                step()
            k, dt, last = run_for(step, max(1.0, a.min_seconds))
            res["torch_eager"] = {"steps": k, "seconds": round(dt, 4), "ms_per_step": round(1e3 * dt / k, 3), "images_per_s": round(a.n * k / dt, 1),
                                  "final_loss": round(last, 5)}
        if "hip_taps_head" in res and "torch_eager" in res:
            best = min(res["hip_" + name]["ms_per_step"] for name, _ in CONFIGS)
            res["speedup_best_hip_over_torch_eager"] = round(res["torch_eager"]["ms_per_step"] / best, 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
