"""Bit record of the fused split-operand F(2x2) convolution (csrc/conv_winograd_x3.hip: runet_wino_conv_x3, runet_wino_conv_x3_stats) as a
REFERENCE build of the library computes it: one SHA-256 per output tensor on seeded inputs, written to tests/golden/wino_x3_parent_bits.json.
tests/test_gpu_wino_x3_epilogue.py imports the cases and the runner from here and holds the library under test to these hashes, so a change
of the kernel that is meant to keep every bit (another ownership of the positions, another exchange in the epilogue) is checked mechanically.

The record must come from the build one compares against, never from the code under test: the script refuses to write unless RUNET_HIP_LIB
names that build's librunet_hip.so (see _lib.py), and it wants the commit that build was made from.  One fresh process:

  RUNET_HIP_LIB=/path/to/parent/librunet_hip.so python tools/wino_x3_bits.py --commit <parent commit hash>

It also prints, per case, the accuracy figures the test asserts (the bits being equal, they are the same for both builds).
"""
import argparse
import hashlib
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "wino_x3_parent_bits.json")

# name: n, h, w, K, N, bias, accumulate, ldx, ldy, dgrad.   (n, h, w, K, N) as the kernel sees them: K contraction, N output channels.
CASES = {
    # one partial patch (3 x 5 of the 4 x 8 tiles), one K chunk, columns >= N in every lane group
    "partial_patch_k16_n6": dict(n=1, h=6, w=10, K=16, N=6, bias=True, accumulate=False, ldx=16, ldy=6, dgrad=False),
    # one full patch at the flagship's K and N
    "full_patch_k64_n64_bias": dict(n=1, h=8, w=16, K=64, N=64, bias=True, accumulate=False, ldx=64, ldy=64, dgrad=False),
    "full_patch_k64_n64": dict(n=1, h=8, w=16, K=64, N=64, bias=False, accumulate=False, ldx=64, ldy=64, dgrad=False),
    # a second output chunk of 6 channels, patches partial in both directions
    "second_chunk_k32_n70": dict(n=2, h=12, w=20, K=32, N=70, bias=True, accumulate=False, ldx=32, ldy=70, dgrad=False),
    # 18 patches (the remainder group of the block remap), two output chunks, three K chunks, accumulate into a pre-filled slice
    "remap_tail_k48_n128_accumulate": dict(n=3, h=16, w=48, K=48, N=128, bias=True, accumulate=True, ldx=64, ldy=160, dgrad=False),
    # data-gradient weights (runet_wino_weights_x3(..., dgrad=1))
    "dgrad_k64_n64": dict(n=1, h=8, w=16, K=64, N=64, bias=False, accumulate=False, ldx=64, ldy=64, dgrad=True),
}


def make_inputs(name):
    """Seeded CPU tensors of a case: x [n, h, w, ldx] (the first K channels are read), w HWIO [3, 3, cin, cout] at unit scale, bias [N] or
    None, y0 [n, h, w, ldy] (what the destination holds before the call: Gaussian where the case accumulates, 0.5 otherwise)."""
    c = CASES[name]
    g = torch.Generator().manual_seed(1000 + list(CASES).index(name))
    x = torch.randn(c["n"], c["h"], c["w"], c["ldx"], generator=g)
    cin, cout = (c["N"], c["K"]) if c["dgrad"] else (c["K"], c["N"])
    w = torch.randn(3, 3, cin, cout, generator=g)
    bias = torch.randn(c["N"], generator=g) if c["bias"] else None
    y0 = torch.randn(c["n"], c["h"], c["w"], c["ldy"], generator=g) if c["accumulate"] else torch.full((c["n"], c["h"], c["w"], c["ldy"]), 0.5)
    return dict(x=x, w=w, bias=bias, y0=y0)


def run(lib, check, stream, name, inp, stats, f32=False):
    """One launch on cuda:0 -> (y [n, h, w, ldy] on the CPU, the statistics partials [parts, N, 3] on the CPU or None).
    f32: the f32-MFMA kernel runet_wino_conv on the same inputs (no statistics)."""
    c = CASES[name]
    dev = torch.device("cuda:0")
    x, w, y = inp["x"].to(dev), inp["w"].to(dev), inp["y0"].to(dev).clone()
    bias = inp["bias"].to(dev) if inp["bias"] is not None else None
    cin, cout = w.shape[2], w.shape[3]
    if f32:
        U = torch.empty((16, c["K"], c["N"]), device=dev)
        check(lib.runet_wino_weights(w.data_ptr(), U.data_ptr(), cin, cout, int(c["dgrad"]), stream))
    else:
        U = torch.empty(lib.runet_wino_x3_pack_elems(c["K"], c["N"]), device=dev, dtype=torch.bfloat16)
        check(lib.runet_wino_weights_x3(w.data_ptr(), U.data_ptr(), cin, cout, int(c["dgrad"]), stream))
    head = (x.data_ptr(), c["ldx"], U.data_ptr(), bias.data_ptr() if bias is not None else None, y.data_ptr(), c["ldy"],
            c["n"], c["h"], c["w"], c["K"], c["N"], int(c["accumulate"]))
    part = None
    if f32:
        assert not stats
        check(lib.runet_wino_conv(*head, stream))
    elif stats:
        part = torch.full((lib.runet_wino_conv_x3_stats_parts(c["n"], c["h"], c["w"]), c["N"], 3), -7.0, device=dev)
        check(lib.runet_wino_conv_x3_stats(*head, part.data_ptr(), stream))
    else:
        check(lib.runet_wino_conv_x3(*head, stream))
    torch.cuda.synchronize()
    return y.cpu(), (part.cpu() if part is not None else None)


def sha(t):
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


def chan_combine(part):
    """[parts, N, 3] (count, mean, M2) -> per-channel count, mean, M2 in float64, Chan-combined in part order."""
    part = part.double()
    cnt, mean, m2 = torch.zeros(part.shape[1], dtype=torch.float64), torch.zeros(part.shape[1], dtype=torch.float64), torch.zeros(part.shape[1], dtype=torch.float64)
    for p in part:
        nt = cnt + p[:, 0]
        safe = torch.where(nt > 0, nt, torch.ones_like(nt))
        d = p[:, 1] - mean
        m2 = m2 + p[:, 2] + d * d * (cnt * p[:, 0] / safe)
        mean = mean + d * (p[:, 0] / safe)
        cnt = nt
    return cnt, mean, m2


def figures(name, inp, y, y_stats, part, y_f32):
    """The quantities tests/test_gpu_wino_x3_epilogue.py bounds, as a dict of floats (see there for the bounds)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    R = importlib.import_module("x3_ref")
    c = CASES[name]
    xk = inp["x"][..., :c["K"]]
    ref = (R.conv3_dgrad_ref if c["dgrad"] else R.conv3_ref)(xk, inp["w"])
    if inp["bias"] is not None:
        ref = ref + inp["bias"].double()
    if c["accumulate"]:
        ref = ref + inp["y0"][..., :c["N"]].double()
    got = y[..., :c["N"]].double()
    out = dict(rms=float((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()), rms_tol=R.rms_tol(c["K"]),
               pad_untouched=bool(torch.equal(y[..., c["N"]:], inp["y0"][..., c["N"]:])), stats_same_y=bool(torch.equal(y, y_stats)))
    f = y_f32[..., :c["N"]].double()
    out["vs_f32"] = float(((got - f).abs() / (1.0 + f.abs())).max())
    cnt, mean, m2 = chan_combine(part)
    flat = got.reshape(-1, c["N"])
    rmean = flat.mean(0)
    out["count_ok"] = bool((cnt == flat.shape[0]).all())
    out["mean"] = float((mean - rmean).abs().max() / rmean.abs().max())
    rm2 = (flat - rmean).pow(2).sum(0)
    out["m2"] = float((m2 - rm2).abs().max() / rm2.abs().max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit RUNET_HIP_LIB was built from")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    if not os.environ.get("RUNET_HIP_LIB"):
        sys.exit("RUNET_HIP_LIB is unset: the record must come from the reference build's library, not from the code under test")
    sys.path.insert(0, ROOT)
    importlib.import_module("eusipco-2026-robust-unet_amd")
    ops = importlib.import_module("eusipco-2026-robust-unet_amd.ops")
    L = importlib.import_module("eusipco-2026-robust-unet_amd._lib")
    assert os.path.samefile(L.LIB_PATH, os.environ["RUNET_HIP_LIB"])
    rec = {"parent_commit": a.commit, "hash": "sha256 of the tensor's bytes (fp32, C order; y is the whole [n, h, w, ldy] destination)", "cases": {}}
    for name, c in CASES.items():
        inp = make_inputs(name)
        y, _ = run(L.lib, L.check, ops.stream(), name, inp, False)
        ys, part = run(L.lib, L.check, ops.stream(), name, inp, True)
        yf, _ = run(L.lib, L.check, ops.stream(), name, inp, False, f32=True)
        rec["cases"][name] = dict(shape=c, y=sha(y), y_with_stats=sha(ys), stats=sha(part), stats_shape=list(part.shape))
        print(name, json.dumps(figures(name, inp, y, ys, part, yf)), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
