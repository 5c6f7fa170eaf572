"""CPU: FastSCNN in the shell the single-node baselines share (baseline.FusedNet) - tests/test_baseline_scaffold.py's checks for this model:
the SyncBatchNorm guard, set_precision, the device check and the physical -> logical layout rule for every 4-D parameter (the depthwise
weights [c, 1, 3, 3] stored [3][3][1][c] included)."""
import importlib

import pytest
import torch

from conftest import PKG_NAME

HWIO = (3, 2, 0, 1)       # physical -> logical permute; its inverse is (2, 3, 1, 0)


@pytest.fixture(scope="module")
def net(pkg):
    torch.manual_seed(0)
    return pkg.FastSCNN()


def test_is_a_fused_net(net):
    assert isinstance(net, importlib.import_module(PKG_NAME + ".baseline").FusedNet)


def test_sync_bn_hook_is_refused(net):
    with pytest.raises(NotImplementedError, match="FastSCNN"):
        net.sync_bn_hook = object()
    net.sync_bn_hook = None
    assert net.sync_bn_hook is None


def test_set_precision(net):
    for mode in ("nonsense", "bf16", "fp16"):
        with pytest.raises(ValueError):
            net.set_precision(mode)
    assert net.set_precision("f32") is net and net.precision == "f32"


def test_cpu_input_is_refused(net):
    with pytest.raises(RuntimeError, match="no CPU path"):
        net(torch.zeros(2, 3, 32, 32))


def test_layout_rule_follows_the_owning_module(net):
    """A gradient in the physical shape the backward produces (the parameter's own storage order) comes out with exactly the parameter's shape
    and strides by the HWIO rule: the model owns no transposed convolution."""
    seen = {"depthwise": 0, "other": 0}
    for name, p in net.named_parameters():
        if p.dim() != 4:
            g = torch.zeros(p.shape)
            assert net.logical_grad(name, g) is g, name
            continue
        seen["depthwise" if name.endswith("depthwise.weight") else "other"] += 1
        phys = p.detach().permute(2, 3, 1, 0)
        assert phys.is_contiguous(), (name, "the parameter's storage is not HWIO")
        g = torch.arange(phys.numel(), dtype=torch.float32).view(phys.shape)
        out = net.logical_grad(name, g)
        assert out.shape == p.shape and out.stride() == p.stride(), (name, tuple(out.shape), tuple(p.shape))
        assert torch.equal(out, g.permute(HWIO)), name
    assert seen == {"depthwise": 13, "other": 1 + 13 + 4 + 2 + 1}
