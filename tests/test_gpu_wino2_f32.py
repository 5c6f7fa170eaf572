"""The fp32 fused Winograd F(2x2, 3x3) kernels of csrc/conv_winograd.hip against float64 torch, called so that no route can move a case
to another kernel:

  forward / data gradient   runet_wino_conv with ops.USE_WINO_X3 off (the filter comes back as fp32 U, asserted), the shapes and
                            assertions of test_gpu_conv.py::test_winograd_fwd_and_dgrad (bias, accumulate into a channel slice, untouched
                            guard channels) plus two shapes with cout = 6 < 16 (masked filter columns): 3 patches (a lone tail group of
                            the XCD-aware block order) and 9 patches (one full group of 8 and a tail of 1).  A data gradient contracts
                            over cout, so it is taken where cout is a multiple of 16.
                            Bound: |err| <= 3e-4 (1 + |ref|), the project's bound for a Winograd F(2x2) result.
  weight gradient           lib.runet_wino_wgrad itself, in the three forms it can take: the zig-zag direct instance (tile rows AND tile
                            columns even), the row-major direct instance (any odd tile count) and the LDS form (w < 4).  One and two tile
                            ranges, one and two channel blocks along cin, channel counts ragged against 32, odd tile columns with two
                            ranges (where the zig-zag decode of a range's first tile would go wrong), x and dy as channel slices of wider
                            buffers.  Bound: 3e-4 max(1, sqrt(n h w / 256)) (1 + |ref|), the one test_gpu_conv.py uses for weight gradients.
                            RUNET_WINO_WGRAD_LDS and RUNET_WINO_WGRAD_ROWMAJOR are read once per process: the same cases run again in one
                            fresh child process each.

Every launch is a handful of blocks; the float64 references are computed once per case and shared."""
import functools
import importlib
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

prng = importlib.import_module("eusipco-2026-robust-unet_amd.portable_rng")


def _ops():
    return importlib.import_module("eusipco-2026-robust-unet_amd.ops")


def rnd(shape, seed, std=1.0):
    return torch.from_numpy(prng.normal_f32(shape, seed, std))


def worst(got, ref):
    """max |err| / (1 + |ref|) against a float64 reference"""
    got, ref = got.detach().cpu().double(), ref.detach().double()
    return float(((got - ref).abs() / (1.0 + ref.abs())).max())


FWD_CASES = [(2, 8, 8, 16, 32), (1, 12, 20, 64, 128), (3, 4, 4, 128, 256), (2, 16, 16, 32, 48), (2, 64, 64, 64, 64), (1, 32, 32, 256, 64),
             (5, 6, 10, 48, 32), (1, 4, 36, 16, 6), (1, 20, 36, 16, 6)]


@pytest.mark.parametrize("n,h,w,cin,cout", FWD_CASES)
def test_fwd_and_dgrad_on_the_f32_kernel(n, h, w, cin, cout, monkeypatch):
    ops = _ops()
    monkeypatch.setattr(ops, "USE_WINO_X3", False)
    dev = torch.device("cuda:0")
    x = rnd((n, cin, h, w), 21)
    wt = rnd((cout, cin, 3, 3), 22, std=(2.0 / (cin * 9)) ** 0.5)
    b = rnd((cout,), 23)
    gy = rnd((n, cout, h, w), 24)
    xr = x.double().requires_grad_(True)
    yr = F.conv2d(xr, wt.double(), b.double(), padding=1)
    yr.backward(gy.double())
    xg = x.permute(0, 2, 3, 1).contiguous().to(dev)
    wg = wt.permute(2, 3, 1, 0).contiguous().to(dev)
    gyg = gy.permute(0, 2, 3, 1).contiguous().to(dev)
    assert ops.wino_ok(h, w, cin, cout)
    U = ops.wino_weights(wg)
    assert U.dtype == torch.float32, "the split-operand kernel would be taken"
    e_fwd = worst(ops.wino_conv(xg, U, b.to(dev)).permute(0, 3, 1, 2), yr)
    print(f"{(n, h, w, cin, cout)}: forward max |err| / (1 + |ref|) {e_fwd:.3e} (limit 3e-4)")
    assert e_fwd <= 3e-4, e_fwd
    if not ops.wino_ok(h, w, cout, cin):
        return
    Ud = ops.wino_weights(wg, dgrad=True)
    assert Ud.dtype == torch.float32, "the split-operand kernel would be taken"
    buf = torch.full((n, h, w, cin + 8), 3.0, device=dev)
    ops.wino_conv(gyg, Ud, None, out=buf[..., 8:], accumulate=True)
    e_dx = worst(buf[..., 8:].permute(0, 3, 1, 2), xr.grad + 3.0)
    print(f"{(n, h, w, cin, cout)}: data gradient max |err| / (1 + |ref|) {e_dx:.3e} (limit 3e-4)")
    assert e_dx <= 3e-4, e_dx
    assert float(buf[..., :8].min()) == 3.0 and float(buf[..., :8].max()) == 3.0


# n, h, w, cin, cout, ldx, ldy
WGRAD_CASES = {
    "zigzag-1range-wci1": (1, 8, 8, 16, 16, 16, 16),
    "zigzag-2ranges-wci2-ragged": (2, 16, 12, 48, 80, 48, 80),
    "oddTX-2ranges-16x6": (4, 16, 6, 16, 16, 16, 16),
    "oddTX-2ranges-16x10": (2, 16, 10, 32, 48, 32, 48),
    "oddTY-rowmajor-2ranges": (5, 6, 10, 48, 32, 48, 32),
    "w2-lds-form": (3, 8, 2, 16, 32, 16, 32),
    "zigzag-2ranges-channel-slices": (2, 16, 12, 48, 80, 56, 96),
}


@functools.lru_cache(maxsize=None)
def _wgrad_case(name):
    """(x, dy) NHWC fp32 on the host and the float64 weight gradient [3][3][cin][cout]; computed once per case"""
    n, h, w, cin, cout, _, _ = WGRAD_CASES[name]
    x, dy = rnd((n, cin, h, w), 31), rnd((n, cout, h, w), 32)
    wr = torch.zeros((cout, cin, 3, 3), dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), wr, None, padding=1).backward(dy.double())
    return x.permute(0, 2, 3, 1).contiguous(), dy.permute(0, 2, 3, 1).contiguous(), wr.grad.permute(2, 3, 1, 0).contiguous()


@pytest.mark.parametrize("name", list(WGRAD_CASES))
def test_wgrad_against_float64(name):
    ops = _ops()
    L = importlib.import_module("eusipco-2026-robust-unet_amd._lib")
    lib, check = L.lib, L.check
    dev = torch.device("cuda:0")
    n, h, w, cin, cout, ldx, ldy = WGRAD_CASES[name]
    x, dy, ref = _wgrad_case(name)
    xb = torch.full((n, h, w, ldx), 5.0, device=dev)            # the channels around the slices must not matter
    yb = torch.full((n, h, w, ldy), -5.0, device=dev)
    xs, ys = xb[..., ldx - cin:], yb[..., ldy - cout:]
    xs.copy_(x)
    ys.copy_(dy)
    dw = torch.zeros((3, 3, cin, cout), device=dev)
    ws = torch.zeros(lib.runet_wino_wgrad_workspace_floats(n, h, w, cin, cout), device=dev)
    check(lib.runet_wino_wgrad(xs.data_ptr(), ldx, ys.data_ptr(), ldy, dw.data_ptr(), ws.data_ptr(), ws.numel(), n, h, w, cin, cout, ops.stream()))
    tol = 3e-4 * max(1.0, (n * h * w / 256.0) ** 0.5)
    err = worst(dw, ref)
    print(f"{name} {(n, h, w, cin, cout)}: max |err| / (1 + |ref|) {err:.3e} (limit {tol:.3e})")
    assert err <= tol, (name, err)


@pytest.mark.parametrize("knob", ["RUNET_WINO_WGRAD_LDS", "RUNET_WINO_WGRAD_ROWMAJOR"])
def test_wgrad_forms_behind_the_knobs_in_a_child_process(knob):
    """every weight-gradient case on the LDS form / the row-major direct instance: one fresh process per knob"""
    here = os.path.abspath(__file__)
    r = subprocess.run([sys.executable, "-m", "pytest", here, "-q", "-x", "-s", "-k", "test_wgrad_against_float64", "-p", "no:cacheprovider"],
                       env=dict(os.environ, **{knob: "1"}), capture_output=True, text=True, timeout=300, cwd=os.path.dirname(os.path.dirname(here)))
    print(r.stdout[-3000:])
    assert r.returncode == 0 and f"{len(WGRAD_CASES)} passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
