"""Bit record of the RGB stem's forward kernel (csrc/conv_stem.hip: runet_stem_conv, runet_stem_conv_stats) as a REFERENCE build of the
library computes it: one SHA-256 per output tensor on seeded inputs, written to tests/golden/stem_parent_bits.json.
tests/test_gpu_stem_persistent.py imports the cases and the runner from here and holds the library under test to these hashes: the
persistent form of the kernel (blocks that walk several tiles, B built once per block, a double-buffered halo, the column tiles in two
passes) keeps every accumulator's k order and every combine of the BatchNorm partials, so every bit must stay.

The record must come from the build one compares against, never from the code under test: the script refuses to write unless RUNET_HIP_LIB
names that build's librunet_hip.so (see _lib.py), and it wants the commit that build was made from.  One fresh process:

  RUNET_HIP_LIB=/path/to/parent/librunet_hip.so python tools/stem_bits.py --commit <parent commit hash>

The binding declares every entry point of include/runet_hip.h, so a reference build that lacks an entry point of the current header is
recorded from a checkout of its own commit (this file copied into its tools/, --out pointing here).
"""
import argparse
import hashlib
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "stem_parent_bits.json")

# name: n, h, w, cin_w, cout, shortcut (the 1x1 filter rides along).  Tiles are 8 x 32 pixels.
CASES = {
    # one tile: fewer tiles than any grid has blocks
    "one_tile": dict(n=1, h=8, w=32, cin_w=3, cout=64, shortcut=False),
    "one_tile_shortcut": dict(n=1, h=8, w=32, cin_w=3, cout=64, shortcut=True),
    # 2 x 2 tiles per image, the second tile row with 2 of 8 rows (waves 1..3 idle there), the second tile column with 8 of 32 columns
    "ragged": dict(n=2, h=10, w=40, cin_w=3, cout=64, shortcut=False),
    "ragged_shortcut": dict(n=2, h=10, w=40, cin_w=3, cout=64, shortcut=True),
    # 3 x 3 tiles per image, 27 in all: a block of a small grid walks several and crosses an image boundary
    "walk": dict(n=3, h=24, w=96, cin_w=3, cout=64, shortcut=False),
    "walk_shortcut": dict(n=3, h=24, w=96, cin_w=3, cout=64, shortcut=True),
    # the one- and two-column-tile instances (other models' stems)
    "nt1_gray": dict(n=2, h=10, w=40, cin_w=1, cout=32, shortcut=False),
    "nt2_shortcut": dict(n=2, h=10, w=40, cin_w=3, cout=32, shortcut=True),
}


def make_inputs(name):
    """Seeded CPU tensors of a case: x [n, h, w, 4] (channels >= cin_w hold garbage the kernel must not read into the result),
    w3 HWIO [3, 3, cin_w, cout], w1 [1, 1, cin_w, cout] or None"""
    c = CASES[name]
    g = torch.Generator().manual_seed(2000 + list(CASES).index(name))
    x = torch.randn(c["n"], c["h"], c["w"], 4, generator=g)
    x[..., c["cin_w"]:] = 1e3
    w3 = torch.randn(3, 3, c["cin_w"], c["cout"], generator=g) * (2.0 / (9 * c["cin_w"])) ** 0.5
    w1 = torch.randn(1, 1, c["cin_w"], c["cout"], generator=g) if c["shortcut"] else None
    return dict(x=x, w3=w3, w1=w1)


def run(lib, check, stream, name, inp, stats):
    """One launch on cuda:0 -> dict of CPU tensors: y3, y1 (or absent), and with stats the partials stats3, stats1 [tiles, cout, 3]"""
    c = CASES[name]
    dev = torch.device("cuda:0")
    x, w3 = inp["x"].to(dev), inp["w3"].to(dev)
    w1 = inp["w1"].to(dev) if inp["w1"] is not None else None
    shape = (c["n"], c["h"], c["w"], c["cout"])
    y3 = torch.full(shape, -7.0, device=dev)
    y1 = torch.full(shape, -7.0, device=dev) if w1 is not None else None
    args = (x.data_ptr(), 4, w3.data_ptr(), w1.data_ptr() if w1 is not None else None, y3.data_ptr(), c["cout"],
            y1.data_ptr() if y1 is not None else None, c["cout"] if y1 is not None else 0, c["n"], c["h"], c["w"], c["cin_w"], c["cout"])
    res = {}
    if stats:
        parts = lib.runet_stem_conv_stats_parts(c["n"], c["h"], c["w"])
        s3 = torch.full((parts, c["cout"], 3), -7.0, device=dev)
        s1 = torch.full((parts, c["cout"], 3), -7.0, device=dev) if w1 is not None else None
        check(lib.runet_stem_conv_stats(*args, s3.data_ptr(), s1.data_ptr() if s1 is not None else None, stream))
        res["stats3"] = s3
        if s1 is not None:
            res["stats1"] = s1
    else:
        check(lib.runet_stem_conv(*args, stream))
    res["y3"] = y3
    if y1 is not None:
        res["y1"] = y1
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in res.items()}


def sha(t):
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


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
    rec = {"parent_commit": a.commit, "hash": "sha256 of the tensor's bytes (fp32, C order)", "cases": {}}
    for name, c in CASES.items():
        inp = make_inputs(name)
        plain = run(L.lib, L.check, ops.stream(), name, inp, False)
        full = run(L.lib, L.check, ops.stream(), name, inp, True)
        assert all(torch.equal(plain[k], full[k]) for k in plain), name
        rec["cases"][name] = dict(shape=c, **{k: sha(v) for k, v in sorted(full.items())}, stats_shape=list(full["stats3"].shape))
        print(name, {k: rec["cases"][name][k][:12] for k in sorted(full)}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
