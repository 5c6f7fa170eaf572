"""GPU: the persistent RGB stem kernel (csrc/conv_stem.hip stem_conv_kernel: blocks walk tiles b, b + grid, ...; B built once per block;
double-buffered halo; the column tiles in two passes) computes what the one-tile-per-block kernel before it computed.

  accuracy  y3 / y1 against torch.nn.functional.conv2d in float64 on the CPU, |err| <= 2e-4 (1 + |ref|): the bound of the stem cases of
            tests/test_gpu_conv.py (test_stem_kernels);
  bits      y3, y1 and the BatchNorm partials [tiles][cout][3] hash to what the PARENT build's library gave for the same seeded inputs
            (tests/golden/stem_parent_bits.json, written by tools/stem_bits.py from that build, never from the code under test).

Every case runs at the default grid (two blocks per CU: more blocks than these shapes have tiles, so one tile per block) and with
RUNET_STEM_CONV_BLOCKS = 1 and 4 (read at every launch): one block walks every tile / 27 tiles over 4 blocks, 7 + 7 + 7 + 6, each walk
crossing an image boundary (9 tiles per image) and ending at another parity of the halo buffer.  The partial of a tile lands at the tile's
index whichever block computes it.  Cases (tools/stem_bits.py CASES): one tile; ragged tile rows (2 of 8: idle waves) and columns
(8 of 32); 3 x 3 x 3 tiles; the one- and two-column-tile instances.  The float64 references are computed once per case."""
import functools
import importlib
import importlib.util
import json
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("stem_bits", os.path.join(ROOT, "tools", "stem_bits.py"))
B = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(B)

NAMES = list(B.CASES)
GRIDS = [None, 1, 4]
TOL = 2e-4


@functools.lru_cache(maxsize=None)
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "stem_parent_bits.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (inputs, y3 float64 NHWC, y1 float64 NHWC or None)"""
    c, inp = B.CASES[name], B.make_inputs(name)
    x = inp["x"][..., :c["cin_w"]].permute(0, 3, 1, 2).double()
    y3 = F.conv2d(x, inp["w3"].permute(3, 2, 0, 1).double(), padding=1).permute(0, 2, 3, 1)
    y1 = F.conv2d(x, inp["w1"].permute(3, 2, 0, 1).double()).permute(0, 2, 3, 1) if inp["w1"] is not None else None
    return inp, y3, y1


def test_the_record_covers_the_cases():
    g = golden()
    assert sorted(g["cases"]) == sorted(NAMES) and len(g["parent_commit"]) == 40
    for name in NAMES:
        assert g["cases"][name]["shape"] == B.CASES[name], name


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"blocks_{g or 'default'}")
@pytest.mark.parametrize("name", NAMES)
def test_stem_bits_and_accuracy(name, grid, monkeypatch):
    L = importlib.import_module(PKG_NAME + "._lib")
    ops = importlib.import_module(PKG_NAME + ".ops")
    if grid is None:
        monkeypatch.delenv("RUNET_STEM_CONV_BLOCKS", raising=False)
    else:
        monkeypatch.setenv("RUNET_STEM_CONV_BLOCKS", str(grid))
    c, rec = B.CASES[name], golden()["cases"][name]
    inp, y3, y1 = reference(name)
    tiles = c["n"] * -(-c["h"] // 8) * -(-c["w"] // 32)
    assert L.lib.runet_stem_conv_stats_parts(c["n"], c["h"], c["w"]) == tiles == rec["stats_shape"][0]
    for stats in (False, True):
        got = B.run(L.lib, L.check, ops.stream(), name, inp, stats)
        assert sorted(got) == sorted(k for k in ("y3", "y1", "stats3", "stats1") if (stats or k[0] == "y") and (c["shortcut"] or k[-1] == "3"))
        for k, ref in (("y3", y3), ("y1", y1)):
            if ref is None:
                continue
            err = (got[k].double() - ref).abs()
            worst = float((err / (1.0 + ref.abs())).max())
            print(f"{name} blocks={grid} stats={stats} {k}: max err / (1 + |ref|) = {worst:.2e}")
            assert worst <= TOL, (name, k, worst)
        for k, t in got.items():
            assert B.sha(t) == rec[k], f"{name}: {k} differs from the parent build's bits (blocks={grid}, stats={stats})"
        if stats:
            assert bool((got["stats3"][..., 0].sum(0) == c["n"] * c["h"] * c["w"]).all())      # every pixel counted once per channel
