"""CPU: host side of the streaming 1x1 convolution (csrc/conv1x1_stream.hip) - what it supports, what it refuses before any launch, and
which calls ops.py routes to it."""
import ctypes
import importlib

import torch

FWD, DGRAD = 0, 1


def _ops():
    return importlib.import_module("eusipco-2026-robust-unet_amd.ops")


def test_supported_truth_table():
    lib = _ops().lib
    for mode in (FWD, DGRAD):
        for cin in (8, 16, 32, 128, 144):
            for cout in (2, 4, 36, 128, 132):
                want = cin in (16, 32, 128) and cout in (4, 36, 128)
                assert bool(lib.runet_conv1x1_stream_supported(cin, cout, mode)) == want, (cin, cout, mode)
    for mode in (2, 3, 4, 5, -1):      # the transposed modes and the pre-transposed data gradient are not this kernel's
        assert not lib.runet_conv1x1_stream_supported(64, 64, mode)


def test_refusals_before_any_launch():
    lib = _ops().lib
    P = ctypes.c_void_p
    good = dict(x=P(0x1000), ldx=64, w=P(0x2000), bias=None, y=P(0x3000), ldy=32, n=1, h=4, w_=4, cin=64, cout=32, mode=FWD, acc=0)

    def call(**kw):
        a = dict(good, **kw)
        return lib.runet_conv1x1_stream(a["x"], a["ldx"], a["w"], a["bias"], a["y"], a["ldy"], a["n"], a["h"], a["w_"], a["cin"], a["cout"], a["mode"],
                                        a["acc"], None)
    for kw, text in ((dict(x=None), b"null pointer"), (dict(w=None), b"null pointer"), (dict(y=None), b"null pointer"),
                     (dict(ldx=48), b"pixel strides"), (dict(ldy=28), b"pixel strides"), (dict(ldx=66), b"pixel strides"), (dict(ldy=34), b"pixel strides"),
                     (dict(x=P(0x1004)), b"16-byte aligned"), (dict(y=P(0x3008)), b"16-byte aligned"), (dict(w=P(0x2004)), b"16-byte aligned"),
                     (dict(cin=8), b"cin a multiple of 16"), (dict(cin=144, ldx=144), b"cin a multiple of 16"), (dict(cout=132, ldy=132), b"cin a multiple of 16"),
                     (dict(cout=30), b"cin a multiple of 16"), (dict(mode=2), b"mode FWD or DGRAD"), (dict(n=0), b"empty iteration space"),
                     (dict(h=0), b"empty iteration space")):
        assert call(**kw) == 1, kw      # RUNET_EINVAL: validation failed on the host, nothing was launched
        assert text in lib.runet_last_error(), (kw, lib.runet_last_error())


def test_block_count_knob(monkeypatch):
    lib = _ops().lib
    monkeypatch.setenv("RUNET_CONV1X1_STREAM_BLOCKS", "2")
    assert lib.runet_conv1x1_stream_blocks(16, 256, 256, 64, 128) == 2
    monkeypatch.delenv("RUNET_CONV1X1_STREAM_BLOCKS")
    assert lib.runet_conv1x1_stream_blocks(1, 5, 7, 64, 128) == 1            # 2 wave tiles: one block
    assert lib.runet_conv1x1_stream_blocks(1, 16, 16, 64, 128) == 2          # 8 wave tiles: two blocks
    assert lib.runet_conv1x1_stream_blocks(0, 16, 16, 64, 128) == 0
    assert lib.runet_conv1x1_stream_kernel_name(64, 128, 1) == b"conv1x1_stream_kernel<4, 4, true>"
    assert lib.runet_conv1x1_stream_kernel_name(128, 36, 0) == b"conv1x1_stream_kernel<8, 2, false>"


def _nhwc(n, h, w, c, ld=None, off=0):
    """An NHWC view without memory behind it: c channels at channel offset `off` of a buffer with pixel stride ld."""
    buf = torch.empty((n, h, w, ld or c), device="meta")
    return buf[..., off:off + c]


# the narrow 1x1 launches of the 16 x 256^2 step that go to the implicit GEMM today: (mode, channels read, channels written, image side, source ld, destination ld)
HEADLINE = [
    (DGRAD, 64, 128, 256, 64, 128),
    (FWD, 128, 64, 256, 128, 64),
    (FWD, 64, 32, 256, 64, 32),
    (FWD, 64, 32, 256, 128, 32),
    (DGRAD, 32, 64, 256, 32, 64),
    (DGRAD, 32, 64, 256, 32, 128),
    (FWD, 64, 128, 128, 64, 128),
    (FWD, 128, 64, 128, 128, 64),
    (FWD, 128, 64, 128, 256, 64),
    (DGRAD, 64, 128, 128, 64, 128),
    (DGRAD, 64, 128, 128, 64, 256),
    (DGRAD, 128, 64, 128, 128, 64),
]


def test_routing_takes_the_headline_calls_and_nothing_of_the_split_operand_kernels(monkeypatch):
    ops = _ops()
    monkeypatch.setattr(ops, "USE_CONV1X1_STREAM", True)
    monkeypatch.setattr(ops, "_PRECISION", "f32")
    for mode, cin, cout, side, ldx, ldy in HEADLINE:
        x = _nhwc(16, side, side, cin, ldx)
        out = _nhwc(16, side, side, cout, ldy)
        assert not ops._conv_x3_case(x, cin, cin, cout), (mode, cin, cout)
        assert ops._conv1x1_stream_case(mode, x, cin, cin, cout, 1, 1, out), (mode, cin, cout, side, ldx, ldy)
    # what the split-operand kernels take is never taken here, nor are 3x3 kernels, padded weights (the stem) or unsupported widths
    for cin, cout in ((128, 128), (256, 64), (256, 128), (512, 256)):
        x = _nhwc(16, 64, 64, cin)
        assert ops._conv_x3_case(x, cin, cin, cout) and not ops._conv1x1_stream_case(FWD, x, cin, cin, cout)
    x = _nhwc(2, 16, 16, 64)
    assert not ops._conv1x1_stream_case(FWD, x, 64, 64, 32, 3, 3)
    assert not ops._conv1x1_stream_case(FWD, _nhwc(2, 16, 16, 4), 4, 3, 64)
    assert not ops._conv1x1_stream_case(FWD, _nhwc(2, 16, 16, 16), 16, 12, 64)
    assert not ops._conv1x1_stream_case(FWD, _nhwc(2, 16, 16, 8), 8, 8, 64)
    assert not ops._conv1x1_stream_case(FWD, x, 64, 64, 30)
    assert not ops._conv1x1_stream_case(FWD, _nhwc(2, 16, 16, 64, 66, 2), 64, 64, 32)          # source neither 16-byte aligned nor ld % 4 == 0
    assert not ops._conv1x1_stream_case(FWD, x, 64, 64, 32, 1, 1, _nhwc(2, 16, 16, 32, 34))     # destination ld % 4 != 0
    monkeypatch.setattr(ops, "_PRECISION", "bf16")
    assert not ops._conv1x1_stream_case(FWD, x, 64, 64, 32)


def test_switch_restores_the_implicit_gemm(monkeypatch):
    ops = _ops()
    monkeypatch.setattr(ops, "_PRECISION", "f32")
    monkeypatch.setattr(ops, "USE_CONV1X1_STREAM", False)
    for mode, cin, cout, side, ldx, ldy in HEADLINE:
        assert not ops._conv1x1_stream_case(mode, _nhwc(16, side, side, cin, ldx), cin, cin, cout, 1, 1, _nhwc(16, side, side, cout, ldy))


def test_switch_is_read_from_the_environment():
    import os
    import subprocess
    import sys
    from conftest import ROOT
    code = ("import importlib; ops = importlib.import_module('eusipco-2026-robust-unet_amd.ops'); print(int(ops.USE_CONV1X1_STREAM))")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, RUNET_NO_CONV1X1_STREAM="1"), capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "0", r.stdout + r.stderr
    assert _ops().USE_CONV1X1_STREAM == (os.environ.get("RUNET_NO_CONV1X1_STREAM", "0") != "1")


# ------------------------------------------------------------------ the weight gradient (runet_conv1x1_wgrad_stream)
def test_wgrad_plan():
    lib = _ops().lib
    # one slab per 256 pixels (a block of four waves), at most 256
    for (n, h, w, cin, cout), slabs in (((16, 256, 256, 128, 64), 256),      # 1 048 576 pixels: 4096 blocks wanted, capped at 256
                                        ((3, 24, 24, 64, 32), 7),             # 1 728 pixels: ceil(1728 / 256)
                                        ((1, 5, 7, 32, 64), 1)):              # 35 pixels
        assert lib.runet_conv1x1_wgrad_stream_slabs(n, h, w) == slabs
        assert lib.runet_conv1x1_wgrad_stream_workspace_floats(n, h, w, cin, cout) == slabs * cin * cout
    assert lib.runet_conv1x1_wgrad_stream_slabs(0, 4, 4) == 0
    for cin in (16, 32, 64, 96, 128, 256):
        for cout in (16, 32, 64, 96, 128, 256):
            want = cin in (32, 64, 128) and cout in (32, 64, 128) and not (cin == 128 and cout == 128)
            assert bool(lib.runet_conv1x1_wgrad_stream_supported(cin, cout)) == want, (cin, cout)


def test_wgrad_refusals_before_any_launch():
    lib = _ops().lib
    P = ctypes.c_void_p
    good = dict(x=P(0x1000), ldx=64, dy=P(0x2000), ldy=32, dw=P(0x3000), ws=P(0x4000), wsf=64 * 32, n=1, h=4, w_=4, cin=64, cout=32)

    def call(**kw):
        a = dict(good, **kw)
        return lib.runet_conv1x1_wgrad_stream(a["x"], a["ldx"], a["dy"], a["ldy"], a["dw"], a["ws"], a["wsf"], a["n"], a["h"], a["w_"], a["cin"], a["cout"], None)
    for kw, text in ((dict(x=None), b"null pointer"), (dict(dy=None), b"null pointer"), (dict(dw=None), b"null pointer"), (dict(ws=None), b"null pointer"),
                     (dict(ldx=48), b"pixel strides"), (dict(ldy=28), b"pixel strides"), (dict(ldx=66), b"pixel strides"),
                     (dict(x=P(0x1004)), b"16-byte aligned"), (dict(dy=P(0x2008)), b"16-byte aligned"), (dict(dw=P(0x3004)), b"16-byte aligned"),
                     (dict(cin=48, ldx=48), b"32, 64 or 128"), (dict(cin=128, cout=128, ldx=128, ldy=128), b"32, 64 or 128"),
                     (dict(wsf=64 * 32 - 1), b"workspace too small"), (dict(n=0), b"empty iteration space")):
        assert call(**kw) == 1, kw
        assert text in lib.runet_last_error(), (kw, lib.runet_last_error())


# the narrow 1x1 weight gradients of the 16 x 256^2 step that go to wgrad_tile_kernel<1, ...> today: (cin, cout, image side)
HEADLINE_WGRAD = [(128, 64, 256), (64, 32, 256), (64, 32, 256), (128, 64, 128), (128, 64, 128), (64, 128, 128)]


def test_wgrad_routing_and_switch(monkeypatch):
    ops = _ops()
    monkeypatch.setattr(ops, "_PRECISION", "f32")
    monkeypatch.setattr(ops, "USE_CONV1X1_WGRAD_STREAM", True)
    for cin, cout, side in HEADLINE_WGRAD:
        assert ops._conv1x1_wgrad_stream_case(_nhwc(16, side, side, cin), _nhwc(16, side, side, cout), cin, cin, cout)
        assert ops._conv1x1_wgrad_stream_case(_nhwc(16, side, side, cin, 2 * cin, cin), _nhwc(16, side, side, cout, 2 * cout), cin, cin, cout)
    x, dy = _nhwc(2, 16, 16, 128), _nhwc(2, 16, 16, 128)
    assert not ops._conv1x1_wgrad_stream_case(x, dy, 128, 128, 128)                       # the TN GEMM's
    assert not ops._conv1x1_wgrad_stream_case(_nhwc(2, 16, 16, 256), dy, 256, 256, 128)
    assert not ops._conv1x1_wgrad_stream_case(_nhwc(2, 16, 16, 64), _nhwc(2, 16, 16, 32), 64, 64, 32, 3, 3)
    assert not ops._conv1x1_wgrad_stream_case(_nhwc(2, 16, 16, 4), _nhwc(2, 16, 16, 64), 4, 3, 64)      # the stem
    assert not ops._conv1x1_wgrad_stream_case(_nhwc(2, 16, 16, 64, 66, 2), _nhwc(2, 16, 16, 32), 64, 64, 32)
    monkeypatch.setattr(ops, "USE_CONV1X1_WGRAD_STREAM", False)
    for cin, cout, side in HEADLINE_WGRAD:
        assert not ops._conv1x1_wgrad_stream_case(_nhwc(16, side, side, cin), _nhwc(16, side, side, cout), cin, cin, cout)


def test_wgrad_stream_is_opt_in():
    import os
    ops = _ops()
    want = os.environ.get("RUNET_CONV1X1_WGRAD_STREAM", "0") == "1" and os.environ.get("RUNET_NO_CONV1X1_WGRAD_STREAM", "0") != "1"
    assert ops.USE_CONV1X1_WGRAD_STREAM == want
    if not want:      # the default: the step's weight gradients stay on wgrad_tile_kernel, so the step computes what it did before
        for cin, cout, side in HEADLINE_WGRAD:
            assert not ops._conv1x1_wgrad_stream_case(_nhwc(16, side, side, cin), _nhwc(16, side, side, cout), cin, cin, cout)
