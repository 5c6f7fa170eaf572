"""CPU: ENet in the shell the single-node baselines share (baseline.FusedNet) - tests/test_baseline_scaffold.py's checks for this model: the
SyncBatchNorm guard, set_precision, the device check and the physical -> logical layout rule for every 4-D parameter (the three transposed
convolutions [cin, cout, kh, kw] stored [kh][kw][cin][cout], the rectangular (5, 1) / (1, 5) kernels stored HWIO)."""
import importlib

import pytest
import torch

from conftest import PKG_NAME

HWIO = (3, 2, 0, 1)       # physical -> logical permute; its inverse is (2, 3, 1, 0)
TRANSPOSED = (2, 3, 0, 1)  # [kh, kw, cin, cout] -> [cin, cout, kh, kw]; its own inverse


@pytest.fixture(scope="module")
def net(pkg):
    torch.manual_seed(0)
    return pkg.ENet()


def test_is_a_fused_net(net):
    assert isinstance(net, importlib.import_module(PKG_NAME + ".baseline").FusedNet)


def test_sync_bn_hook_is_refused(net):
    with pytest.raises(NotImplementedError, match="ENet"):
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
    and strides: [kh, kw, cin, cout] -> [cin, cout, kh, kw] for the decoder's three transposed convolutions (the type of the owning module
    decides), HWIO -> OIHW for everything else."""
    seen = {"transposed": 0, "rect": 0, "other": 0}
    for name, p in net.named_parameters():
        if p.dim() != 4:
            g = torch.zeros(p.shape)
            assert net.logical_grad(name, g) is g, name
            continue
        transposed = name in ("decoder.0.weight", "decoder.3.weight", "decoder.6.weight")
        rect = p.shape[2] != p.shape[3]
        seen["transposed" if transposed else "rect" if rect else "other"] += 1
        phys = p.detach().permute(2, 3, 0, 1) if transposed else p.detach().permute(2, 3, 1, 0)
        assert phys.is_contiguous(), (name, "the parameter's storage is not [kh][kw][in][out]")
        g = torch.arange(phys.numel(), dtype=torch.float32).view(phys.shape)
        out = net.logical_grad(name, g)
        assert out.shape == p.shape and out.stride() == p.stride(), (name, tuple(out.shape), tuple(p.shape))
        assert torch.equal(out, g.permute(TRANSPOSED if transposed else HWIO)), name
    # initial 1; per block conv1, conv2, conv3 (13 x 3), conv_down (2), the second kernel of the 2 asymmetric blocks counted under rect
    assert seen == {"transposed": 3, "rect": 4, "other": 1 + 13 * 3 - 2 + 2}
