"""Times the fused split-operand F(2x2) launches of the Robust U-Net step (csrc/conv_winograd_x3.hip) on one stream: the five
(K -> N @ size) shapes its eight launches per step have at 16 x 256^2, base 64.  Prints one line per shape: median and minimum of REPS event-timed
groups of ITERS launches, in microseconds per launch.  A/B of two builds: one fresh process per build, RUNET_HIP_LIB selects the library.

  python tools/wino_x3_time.py [label]
"""
import importlib
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

ops = importlib.import_module("eusipco-2026-robust-unet_amd.ops")
SHAPES = [(64, 64, 256), (64, 128, 256), (128, 64, 256), (64, 128, 128), (128, 64, 128)]      # K, N, size
N_IMG, ITERS, REPS = 16, 20, 7
label = sys.argv[1] if len(sys.argv) > 1 else "lib"
dev = torch.device("cuda:0")
for k, n, s in SHAPES:
    x = torch.randn((N_IMG, s, s, k), device=dev)
    U = ops.wino_weights(torch.randn((3, 3, k, n), device=dev) * 0.05)
    assert U.dtype == torch.bfloat16
    y = torch.empty((N_IMG, s, s, n), device=dev)
    for _ in range(3):
        ops.wino_conv(x, U, out=y)
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            ops.wino_conv(x, U, out=y)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / ITERS)
    print(f"{label:8s} {k:4d}->{n:4d} @ {N_IMG}x{s}^2: median {statistics.median(ts):7.1f} us  min {min(ts):7.1f} us", flush=True)
