"""GPU: the streaming weight-resident 1x1 convolution (csrc/conv1x1_stream.hip) against the implicit GEMM it replaces on the narrow layers.

Every case runs runet_conv1x1_stream and runet_conv_igemm through the C ABI on the same inputs in the same process and asks for
torch.equal outputs (the kernel forms the implicit GEMM's fp32 MFMA chain per element and stores acc + bias + old in its association),
and checks both against a float64 matmul with the implicit GEMM's bound of tests/test_gpu_conv.py, |err| <= 2e-4 * (1 + |ref|)."""
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

prng = importlib.import_module("eusipco-2026-robust-unet_amd.portable_rng")
FWD, DGRAD = 0, 1
PAIRS = [(16, 4), (32, 64), (64, 32), (64, 128), (128, 64), (128, 128), (48, 36)]
# 35: a single ragged tile; 128: whole tiles only; 1728: many tiles; 3: the one extra image of "1728 + 3", far fewer rows than a tile
PIXELS = [(1, 5, 7), (2, 8, 8), (3, 24, 24), (1, 1, 3)]
# mode, bias, accumulate
VARIANTS = [(FWD, True, False), (FWD, False, False), (FWD, True, True), (FWD, False, True), (DGRAD, False, False), (DGRAD, False, True)]


def _ops():
    return importlib.import_module("eusipco-2026-robust-unet_amd.ops")


def rnd(shape, seed, std=1.0):
    return torch.from_numpy(prng.normal_f32(shape, seed, std))


def _ld(t):
    return t.stride(2)


def _run(ops, which, mode, x, w, bias, y, cin, cout, acc):
    n, h, wd, _ = x.shape
    bp = bias.data_ptr() if bias is not None else None
    if which == "stream":
        ops.check(ops.lib.runet_conv1x1_stream(x.data_ptr(), _ld(x), w.data_ptr(), bp, y.data_ptr(), _ld(y), n, h, wd, cin, cout, mode, int(acc), ops.stream()))
    else:
        ops.check(ops.lib.runet_conv_igemm(x.data_ptr(), _ld(x), w.data_ptr(), bp, y.data_ptr(), _ld(y), n, h, wd, cin, cin, cout, 1, 1, 1, mode, int(acc),
                                           ops.stream()))


def _reference(mode, x, w, bias, y0, cin, cout, acc):
    """float64 on the CPU; w is the module's forward weight: FWD [cin][cout], DGRAD [cout][cin] read transposed."""
    a = x.double().reshape(-1, cin)
    m = w.double() if mode == FWD else w.double().t()
    r = a @ m
    if bias is not None:
        r = r + bias.double()
    if acc:
        r = r + y0.double().reshape(-1, cout)
    return r.reshape(*x.shape[:3], cout)


def _close(got, ref, what):
    err = (got.double().cpu() - ref).abs()
    lim = 2e-4 * (1.0 + ref.abs())
    assert bool((err <= lim).all()), f"{what}: max err {err.max().item():.3e} (ref max {ref.abs().max().item():.3e})"


def _inputs(cin, cout, shape, mode, sliced, seed):
    """-> x view, w, bias, y0 (start value of the destination view), make_y() -> (buffer, view).  sliced: source pixel stride 2 cin at
    channel offset cin, destination pixel stride 2 cout at channel offset cout, the rest of the destination buffer a sentinel."""
    dev = torch.device("cuda:0")
    n, h, wd = shape
    xs = rnd((n, h, wd, 2 * cin if sliced else cin), seed).to(dev)
    x = xs[..., cin:] if sliced else xs
    w = rnd((cin, cout) if mode == FWD else (cout, cin), seed + 1, std=(2.0 / cin) ** 0.5).to(dev)
    bias = rnd((cout,), seed + 2).to(dev)
    y0 = rnd((n, h, wd, cout), seed + 3).to(dev)

    def make_y():
        if not sliced:
            buf = y0.clone()
            return buf, buf
        buf = torch.full((n, h, wd, 2 * cout), 7.0, device=dev)
        buf[..., cout:] = y0
        return buf, buf[..., cout:]
    return x, w, bias, y0, make_y


def _check_case(ops, cin, cout, shape, mode, with_bias, acc, sliced=False, seed=11):
    x, w, bias, y0, make_y = _inputs(cin, cout, shape, mode, sliced, seed)
    b = bias if with_bias else None
    what = f"{cin}->{cout} {shape} mode {mode} bias {with_bias} acc {acc} sliced {sliced}"
    buf_s, y_s = make_y()
    buf_i, y_i = make_y()
    _run(ops, "stream", mode, x, w, b, y_s, cin, cout, acc)
    _run(ops, "igemm", mode, x, w, b, y_i, cin, cout, acc)
    torch.cuda.synchronize()
    assert torch.equal(y_s, y_i), f"{what}: {int((y_s != y_i).sum())} elements differ from the implicit GEMM, max {float((y_s - y_i).abs().max()):.3e}"
    ref = _reference(mode, x.cpu(), w.cpu(), b.cpu() if b is not None else None, y0.cpu(), cin, cout, acc)
    _close(y_s, ref, what + " (stream)")
    _close(y_i, ref, what + " (igemm)")
    if sliced:
        assert float(buf_s[..., :cout].min()) == 7.0 and float(buf_s[..., :cout].max()) == 7.0, what + ": wrote outside its channel slice"


@pytest.mark.parametrize("shape", PIXELS)
@pytest.mark.parametrize("cin,cout", PAIRS)
def test_stream_equals_implicit_gemm(cin, cout, shape):
    ops = _ops()
    assert ops.lib.runet_conv1x1_stream_supported(cin, cout, FWD) and ops.lib.runet_conv1x1_stream_supported(cin, cout, DGRAD)
    for mode, with_bias, acc in VARIANTS:
        _check_case(ops, cin, cout, shape, mode, with_bias, acc)


@pytest.mark.parametrize("shape", [(1, 5, 7), (3, 24, 24)])
@pytest.mark.parametrize("cin,cout", PAIRS)
def test_stream_on_channel_slices(cin, cout, shape):
    ops = _ops()
    for mode in (FWD, DGRAD):
        for acc in (False, True):
            _check_case(ops, cin, cout, shape, mode, mode == FWD, acc, sliced=True, seed=23)


@pytest.mark.parametrize("blocks,shape", [("2", (3, 24, 24)),      # 54 tiles on 8 waves: the persistent loop, its hand-over and the load past the end
                                          ("2", (3, 24, 25)),      # the same with a ragged last tile (1800 pixels)
                                          ("8", (1, 5, 7)),        # 2 tiles on 8 blocks: idle blocks and idle waves
                                          (None, (1, 5, 7))])      # the launcher's own count
def test_stream_block_counts(blocks, shape, monkeypatch):
    ops = _ops()
    if blocks is None:
        monkeypatch.delenv("RUNET_CONV1X1_STREAM_BLOCKS", raising=False)
    else:
        monkeypatch.setenv("RUNET_CONV1X1_STREAM_BLOCKS", blocks)
    n, h, w = shape
    want = int(blocks) if blocks is not None else 1
    assert ops.lib.runet_conv1x1_stream_blocks(n, h, w, 64, 128) == want
    for cin, cout in ((64, 128), (128, 64), (48, 36)):
        for mode, with_bias, acc in VARIANTS:
            _check_case(ops, cin, cout, shape, mode, with_bias, acc, seed=31)
        _check_case(ops, cin, cout, shape, FWD, True, True, sliced=True, seed=37)


def test_ops_route_and_switch(monkeypatch):
    """ops.conv_fwd / conv_dgrad take the stream kernel for the narrow layers, the implicit GEMM under the switch, with equal bits."""
    ops = _ops()
    dev = torch.device("cuda:0")
    calls = []
    real = ops.lib.runet_conv1x1_stream
    monkeypatch.setattr(ops.lib, "runet_conv1x1_stream", lambda *a: (calls.append(a[9:12]), real(*a))[1])
    x = rnd((2, 8, 8, 64), 5).to(dev)
    w = rnd((1, 1, 64, 32), 6, std=0.2).to(dev)
    b = rnd((32,), 7).to(dev)
    gy = rnd((2, 8, 8, 32), 8).to(dev)
    out = {}
    for on in (True, False):
        monkeypatch.setattr(ops, "USE_CONV1X1_STREAM", on)
        y = ops.conv_fwd(x, w, b)
        dx = torch.full((2, 8, 8, 64), 0.5, device=dev)
        ops.conv_dgrad(gy, w, out=dx, accumulate=True)
        out[on] = (y, dx)
    assert calls == [(64, 32, FWD), (32, 64, DGRAD)]
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])


def _train_step(pkg, ops, x, y, state):
    model = pkg.RobustUNet(3, 1, 64)
    model.load_state_dict(state)
    model = model.to(x.device).train()
    opt = pkg.FusedAdam(model.parameters(), lr=1e-3, weight_decay=1e-4)
    opt.zero_grad()
    prob = model(x)
    loss = pkg.bce_loss(prob, y)
    loss.backward()
    grads = [p.grad.detach().clone() for p in model.parameters()]
    opt.step()
    torch.cuda.synchronize()
    return loss.detach().clone(), grads, [p.detach().clone() for p in model.parameters()]


def test_train_step_is_bit_identical_with_and_without_the_stream_kernel(pkg, monkeypatch):
    ops = _ops()
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    state = {k: v.clone() for k, v in pkg.RobustUNet(3, 1, 64).state_dict().items()}
    x, y = pkg.synthetic_batch(2, 64, seed=4)
    x, y = x.to(dev), y.to(dev)
    calls = []
    real = ops.lib.runet_conv1x1_stream
    monkeypatch.setattr(ops.lib, "runet_conv1x1_stream", lambda *a: (calls.append(1), real(*a))[1])
    monkeypatch.setattr(ops, "USE_CONV1X1_STREAM", True)
    torch.manual_seed(9)
    loss_a, grads_a, params_a = _train_step(pkg, ops, x, y, state)
    assert len(calls) > 0, "the 2 x 64^2 step has narrow 1x1 layers: they should have taken the stream kernel"
    taken = len(calls)
    monkeypatch.setattr(ops, "USE_CONV1X1_STREAM", False)
    torch.manual_seed(9)
    loss_b, grads_b, params_b = _train_step(pkg, ops, x, y, state)
    assert len(calls) == taken, "the switch must restore the implicit-GEMM launches"
    assert torch.equal(loss_a, loss_b)
    for i, (a, b) in enumerate(zip(grads_a, grads_b)):
        assert torch.equal(a, b), f"gradient {i} differs"
    for i, (a, b) in enumerate(zip(params_a, params_b)):
        assert torch.equal(a, b), f"updated parameter {i} differs"


# ------------------------------------------------------------------ the weight gradient of the same layers (runet_conv1x1_wgrad_stream)
WG_PAIRS = [(64, 32), (128, 64), (64, 128), (32, 64)]
WG_RESULTS = {}      # (cin, cout, shape, sliced) -> (stream error, tile error), relative to max |dW|; printed by the tests that fill it


def _wgrad(ops, which, x, dy, dw, cin, cout):
    n, h, wd, _ = x.shape
    lib = ops.lib
    if which == "stream":
        ws = ops.workspace(lib.runet_conv1x1_wgrad_stream_workspace_floats(n, h, wd, cin, cout), x.device)
        ops.check(lib.runet_conv1x1_wgrad_stream(x.data_ptr(), _ld(x), dy.data_ptr(), _ld(dy), dw.data_ptr(), ws.data_ptr(), ws.numel(), n, h, wd, cin, cout,
                                                 ops.stream()))
    else:
        ws = ops.workspace(lib.runet_conv_wgrad_workspace_floats(n, h, wd, cin, cout, 1, 1), x.device)
        ops.check(lib.runet_conv_wgrad(x.data_ptr(), _ld(x), dy.data_ptr(), _ld(dy), dw.data_ptr(), ws.data_ptr(), ws.numel(), n, h, wd, cin, cin, cout,
                                       1, 1, 1, 0, ops.stream()))


def _wg_inputs(cin, cout, shape, sliced, seed=41):
    dev = torch.device("cuda:0")
    n, h, wd = shape
    xs = rnd((n, h, wd, 2 * cin if sliced else cin), seed).to(dev)
    ds = rnd((n, h, wd, 2 * cout if sliced else cout), seed + 1).to(dev)
    return (xs[..., cin:], ds[..., cout:]) if sliced else (xs, ds)


@pytest.mark.parametrize("sliced", [False, True])
@pytest.mark.parametrize("shape", PIXELS)
@pytest.mark.parametrize("cin,cout", WG_PAIRS)
def test_wgrad_stream_against_float64_and_the_tile_kernel(cin, cout, shape, sliced):
    ops = _ops()
    assert ops.lib.runet_conv1x1_wgrad_stream_supported(cin, cout)
    x, dy = _wg_inputs(cin, cout, shape, sliced)
    dev = x.device
    pixels = shape[0] * shape[1] * shape[2]
    ref = x.double().cpu().reshape(-1, cin).t() @ dy.double().cpu().reshape(-1, cout)
    bufs = {}
    for which in ("stream", "tile"):
        buf = torch.full((cin * cout + 64,), 7.0, device=dev)      # the gradient, then a sentinel that must stay
        _wgrad(ops, which, x, dy, buf[:cin * cout], cin, cout)
        torch.cuda.synchronize()
        assert float(buf[cin * cout:].min()) == 7.0 and float(buf[cin * cout:].max()) == 7.0, f"{which}: wrote past dw"
        bufs[which] = buf[:cin * cout].view(cin, cout)
    scale = float(ref.abs().max())
    err = {k: float((v.double().cpu() - ref).abs().max()) / scale for k, v in bufs.items()}
    WG_RESULTS[(cin, cout, shape, sliced)] = (err["stream"], err["tile"])
    print(f"wgrad {cin}->{cout} {shape} sliced={sliced}: max err / max|dW|  stream {err['stream']:.3e}  tile {err['tile']:.3e}")
    tol = 3e-4 * max(1.0, (pixels / 256.0) ** 0.5)      # tests/test_gpu_conv.py's bound for fp32 weight gradients
    for which, v in bufs.items():
        e = (v.double().cpu() - ref).abs()
        assert bool((e <= tol * (1.0 + ref.abs())).all()), f"{which}: max err {float(e.max()):.3e}"
    assert err["stream"] <= 1.25 * err["tile"], f"stream {err['stream']:.3e} vs tile {err['tile']:.3e} (relative to max |dW|)"
    # bitwise: a second run, and a graph replay of the same call
    again = torch.empty(cin * cout, device=dev)
    _wgrad(ops, "stream", x, dy, again, cin, cout)
    assert torch.equal(again.view(cin, cout), bufs["stream"]), "two runs differ"
    if shape == (3, 24, 24):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        captured = torch.zeros(cin * cout, device=dev)
        with torch.cuda.stream(side):
            _wgrad(ops, "stream", x, dy, captured, cin, cout)      # warm-up on the capture stream (workspace of that stream)
            captured.zero_()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                _wgrad(ops, "stream", x, dy, captured, cin, cout)
        torch.cuda.current_stream().wait_stream(side)
        captured.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured.view(cin, cout), bufs["stream"]), "graph replay differs from the eager call"


def test_wgrad_ops_route_and_switch(monkeypatch):
    ops = _ops()
    dev = torch.device("cuda:0")
    calls = []
    real = ops.lib.runet_conv1x1_wgrad_stream
    monkeypatch.setattr(ops.lib, "runet_conv1x1_wgrad_stream", lambda *a: (calls.append(a[10:12]), real(*a))[1])
    x = rnd((2, 8, 8, 64), 5).to(dev)
    gy = rnd((2, 8, 8, 32), 8).to(dev)
    out = {}
    for on in (True, False):
        monkeypatch.setattr(ops, "USE_CONV1X1_WGRAD_STREAM", on)
        out[on] = ops.conv_wgrad(x, gy, 1, 1)
    assert calls == [(64, 32)]
    ref = x.double().cpu().reshape(-1, 64).t() @ gy.double().cpu().reshape(-1, 32)
    for v in out.values():
        assert tuple(v.shape) == (1, 1, 64, 32)
        assert float((v.double().cpu().view(64, 32) - ref).abs().max()) <= 3e-4 * (1.0 + float(ref.abs().max()))


def test_train_step_with_and_without_the_stream_weight_gradient(pkg, monkeypatch):
    """One 2 x 64^2 step with the streaming weight gradient on against the same step with it off: the loss is the same number, every gradient
    within 1e-4 of its tensor's scale (the per-tensor bound tests/test_gpu_model.py applies against the oracle)."""
    ops = _ops()
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    state = {k: v.clone() for k, v in pkg.RobustUNet(3, 1, 64).state_dict().items()}
    x, y = pkg.synthetic_batch(2, 64, seed=4)
    x, y = x.to(dev), y.to(dev)
    calls = []
    real = ops.lib.runet_conv1x1_wgrad_stream
    monkeypatch.setattr(ops.lib, "runet_conv1x1_wgrad_stream", lambda *a: (calls.append(1), real(*a))[1])
    monkeypatch.setattr(ops, "USE_CONV1X1_WGRAD_STREAM", True)
    torch.manual_seed(9)
    loss_a, grads_a, _ = _train_step(pkg, ops, x, y, state)
    assert len(calls) > 0
    taken = len(calls)
    monkeypatch.setattr(ops, "USE_CONV1X1_WGRAD_STREAM", False)
    torch.manual_seed(9)
    loss_b, grads_b, _ = _train_step(pkg, ops, x, y, state)
    assert len(calls) == taken
    assert torch.equal(loss_a, loss_b)
    worst = 0.0
    for a, b in zip(grads_a, grads_b):
        worst = max(worst, float((a - b).abs().max()) / (float(b.abs().max()) + 1e-30))
    print(f"largest gradient difference, relative to its tensor's scale: {worst:.3e}")
    assert worst <= 1e-4
