"""The fused split-operand F(2x2) convolution (csrc/conv_winograd_x3.hip) after the re-cut of its epilogue: wave w owns Winograd column
j = w for all four rows, forms the first output-transform stage in registers and exchanges 2 x 4 planes through LDS once.  The re-cut
changes no summation order, so the check is mechanical:

  bits      y and the BatchNorm partials [parts][N][3] hash to what the PARENT build's library gave for the same seeded inputs
            (tests/golden/wino_x3_parent_bits.json, written by tools/wino_x3_bits.py from that build, never from the code under test);
  accuracy  the same outputs against float64 (tests/x3_ref.py conv3_ref / conv3_dgrad_ref) in rms, bound x3_ref.rms_tol(K), and against the
            f32-MFMA kernel runet_wino_conv within |err| <= 3e-4 (1 + |ref|), the bound of test_gpu_conv.py::test_winograd_fwd_and_dgrad
            for a Winograd F(2x2) result;
  stats     the partials, Chan-combined on the host in float64, against the count, mean and M2 of the stored y in float64: count
            exact, mean and M2 to 2e-6 of the largest reference value (the bound of
            test_gpu_conv.py::test_epilogue_statistics_equal_the_separate_pass).

Cases (tools/wino_x3_bits.py CASES): one partial patch with one K chunk and N = 6; one full patch at K = N = 64 with and without bias;
a second output chunk of 6 channels with patches partial in both directions; 18 patches (the remainder group of the block remap), three K
chunks, two output chunks, accumulate into a pre-filled destination with ldy = 160 from a source with ldx = 64; data-gradient weights.
Each with and without statistics.  Every launch is a handful of blocks; the float64 references are computed once per case.
"""
import functools
import importlib
import importlib.util
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import x3_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("wino_x3_bits", os.path.join(ROOT, "tools", "wino_x3_bits.py"))
B = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(B)

with open(os.path.join(ROOT, "tests", "golden", "wino_x3_parent_bits.json")) as _f:
    GOLDEN = json.load(_f)

NAMES = list(B.CASES)


def test_the_record_covers_the_cases():
    assert sorted(GOLDEN["cases"]) == sorted(NAMES) and len(GOLDEN["parent_commit"]) == 40
    for name in NAMES:
        assert GOLDEN["cases"][name]["shape"] == B.CASES[name], name


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return B.make_inputs(name)


@functools.lru_cache(maxsize=None)
def _got(name, stats):
    """(y, partials or None) of one launch of the library under test; computed once, compared by several tests"""
    importlib.import_module("eusipco-2026-robust-unet_amd")
    ops = importlib.import_module("eusipco-2026-robust-unet_amd.ops")
    L = importlib.import_module("eusipco-2026-robust-unet_amd._lib")
    return B.run(L.lib, L.check, ops.stream(), name, _inputs(name), stats)


@functools.lru_cache(maxsize=None)
def _f32(name):
    importlib.import_module("eusipco-2026-robust-unet_amd")
    ops = importlib.import_module("eusipco-2026-robust-unet_amd.ops")
    L = importlib.import_module("eusipco-2026-robust-unet_amd._lib")
    return B.run(L.lib, L.check, ops.stream(), name, _inputs(name), False, f32=True)[0]


@functools.lru_cache(maxsize=None)
def _ref64(name):
    """float64 reference of the first N channels of the destination after the call"""
    c, inp = B.CASES[name], _inputs(name)
    ref = (R.conv3_dgrad_ref if c["dgrad"] else R.conv3_ref)(inp["x"][..., :c["K"]], inp["w"])
    if inp["bias"] is not None:
        ref = ref + inp["bias"].double()
    if c["accumulate"]:
        ref = ref + inp["y0"][..., :c["N"]].double()
    return ref


@pytest.mark.parametrize("stats", [False, True], ids=["plain", "stats"])
@pytest.mark.parametrize("name", NAMES)
def test_bits_equal_the_parent_build(name, stats):
    y, part = _got(name, stats)
    rec = GOLDEN["cases"][name]
    assert B.sha(y) == rec["y_with_stats" if stats else "y"], f"{name}: y differs from the parent build's bits"
    if stats:
        assert list(part.shape) == rec["stats_shape"]
        assert B.sha(part) == rec["stats"], f"{name}: the statistics partials differ from the parent build's bits"


@pytest.mark.parametrize("stats", [False, True], ids=["plain", "stats"])
@pytest.mark.parametrize("name", NAMES)
def test_accuracy_against_float64_and_the_f32_kernel(name, stats):
    c, inp = B.CASES[name], _inputs(name)
    y, _ = _got(name, stats)
    assert torch.equal(y[..., c["N"]:], inp["y0"][..., c["N"]:]), f"{name}: channels beyond N of the destination were written"
    got, ref = y[..., :c["N"]].double(), _ref64(name)
    rms = float((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    print(f"{name} stats={stats}: rms error / rms reference {rms:.3e} (limit {R.rms_tol(c['K']):.3e})")
    assert rms <= R.rms_tol(c["K"]), (name, rms)
    f = _f32(name)[..., :c["N"]].double()
    worst = float(((got - f).abs() / (1.0 + f.abs())).max())
    print(f"{name} stats={stats}: against the f32-MFMA kernel, max |err| / (1 + |ref|) {worst:.3e} (limit 3e-4)")
    assert worst <= 3e-4, (name, worst)


@pytest.mark.parametrize("name", NAMES)
def test_partials_give_the_moments_of_y(name):
    c = B.CASES[name]
    y, part = _got(name, True)
    flat = y[..., :c["N"]].double().reshape(-1, c["N"])
    cnt, mean, m2 = B.chan_combine(part)
    assert bool((cnt == flat.shape[0]).all()), (name, cnt)
    rmean = flat.mean(0)
    rm2 = (flat - rmean).pow(2).sum(0)
    e_mean = float((mean - rmean).abs().max() / rmean.abs().max())
    e_m2 = float((m2 - rm2).abs().max() / rm2.abs().max())
    print(f"{name}: mean {e_mean:.3e}, M2 {e_m2:.3e} of the largest reference value (limit 2e-6)")
    assert e_mean <= 2e-6 and e_m2 <= 2e-6, (name, e_mean, e_m2)
