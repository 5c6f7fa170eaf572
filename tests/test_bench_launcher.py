"""CPU: `python bench.py --gpus N` starts its own N ranks (the driver calls the plain form, not torch.distributed.run) and relays rank 0's
JSON line; the BASELINE.json configurations map to the documented per-GPU shards."""
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_self_launch_two_ranks_over_gloo():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--selftest-launch"], env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec == {"selftest": True, "world": 2, "sum": 3.0}


def test_config_presets_follow_baseline_json():
    bench = importlib.import_module("bench")
    with open(os.path.join(ROOT, "BASELINE.json")) as f:
        assert len(json.load(f)["configs"]) == len(bench.CONFIGS) == 5
    a = bench.parse_args([])
    assert (a.model, a.batch, a.size, a.dtype, a.gpus) == ("runet", 16, 256, "f32", 1)          # the headline configuration
    a = bench.parse_args(["--config", "3"])
    assert (a.batch, a.size, a.dtype) == (4, 512, "bf16")
    a = bench.parse_args(["--config", "5"])
    assert (a.batch, a.size, a.dtype, a.graph) == (1, 1024, "fp16", True)
    a = bench.parse_args(["--config", "4"])
    assert a.model == "deeplab"
    a = bench.parse_args(["--config", "1", "--batch", "8"])
    assert (a.batch, a.size) == (8, 64)


def test_plain_run_options_and_output_dump(tmp_path):
    """A plain run leaves the secondary measurements to --full; --dump-outputs writes float32 arrays, at most 64 MB, at fixed positions."""
    import numpy as np
    import torch
    bench = importlib.import_module("bench")
    a = bench.parse_args(["--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert bench.parse_args(["--full", "--dump-outputs", str(tmp_path)]).full
    model = importlib.import_module("eusipco-2026-robust-unet_amd").RobustUNet(3, 1, 64)      # 40.9 M parameters: sampled
    for i, p in enumerate(model.parameters()):
        p.grad = torch.full_like(p, float(i))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), model, 0.5)
    total = 0
    for name in ("loss", "params", "grads", "buffers"):
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert x.dtype == np.float32 and np.array_equal(x, y)
        total += x.nbytes
    assert total <= 64 << 20
    assert np.load(tmp_path / "a" / "loss.npy").tolist() == [0.5]
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).numpy()
    assert np.isin(np.load(tmp_path / "a" / "params.npy"), flat).all()
