"""CPU: the shell the eight single-node baselines share (baseline.FusedNet): the SyncBatchNorm guard, set_precision, the device check and the
physical -> logical layout rule for every 4-D parameter of every model."""
import importlib

import pytest
import torch

from conftest import PKG_NAME

MODELS = ("DeepLabV3Plus", "UNet", "SegNet", "YOLOSeg", "SegFormerLite", "HRNetWater", "WaterNet", "MSWNet")
LOW_PRECISION = ("UNet", "SegNet")          # the others run in fp32 only
HWIO, TRANSPOSED = (3, 2, 0, 1), (2, 3, 0, 1)       # physical -> logical permutes; the second is its own inverse, the first's is (2, 3, 1, 0)


@pytest.fixture(scope="module", params=MODELS)
def net(request, pkg):
    torch.manual_seed(0)
    return getattr(pkg, request.param)()


def test_is_a_fused_net(net):
    assert isinstance(net, importlib.import_module(PKG_NAME + ".baseline").FusedNet)


def test_sync_bn_hook_is_refused(net):
    with pytest.raises(NotImplementedError, match=type(net).__name__):
        net.sync_bn_hook = object()
    net.sync_bn_hook = None
    assert net.sync_bn_hook is None


def test_set_precision(net):
    with pytest.raises(ValueError):
        net.set_precision("nonsense")
    assert net.precision == "f32"
    if type(net).__name__ in LOW_PRECISION:
        assert net.set_precision("bf16") is net and net.precision == "bf16"
    else:
        with pytest.raises(ValueError):
            net.set_precision("bf16")
    assert net.set_precision("f32") is net and net.precision == "f32"


def test_cpu_input_is_refused(net):
    with pytest.raises(RuntimeError, match="no CPU path"):
        net(torch.zeros(1, 3, 32, 32))


def test_layout_rule_follows_the_owning_module(net):
    """A gradient in the physical shape a backward produces (the parameter's own storage order) must come out with exactly the parameter's
    shape: by the transposed rule for every weight owned by a transposed convolution, by the HWIO rule for every other 4-D parameter."""
    model = importlib.import_module(PKG_NAME + ".model")
    deeplab = importlib.import_module(PKG_NAME + ".deeplab")
    transposed = (model.ConvTranspose2d, deeplab.ConvTranspose2dK4)
    seen = {True: 0, False: 0}
    for name, p in net.named_parameters():
        if p.dim() != 4:
            g = torch.zeros(p.shape)
            assert net.logical_grad(name, g) is g, name
            continue
        owner = net.get_submodule(name.rpartition(".")[0])
        t = isinstance(owner, transposed)
        seen[t] += 1
        phys = p.detach().permute(TRANSPOSED if t else (2, 3, 1, 0))
        assert phys.is_contiguous(), (name, "the parameter's storage is not in the physical order its owner's type implies")
        g = torch.arange(phys.numel(), dtype=torch.float32).view(phys.shape)
        out = net.logical_grad(name, g)
        assert out.shape == p.shape and out.stride() == p.stride(), (name, tuple(out.shape), tuple(p.shape))
        assert torch.equal(out, g.permute(TRANSPOSED if t else HWIO)), name
    assert seen[False] > 0
    assert (seen[True] > 0) == (type(net).__name__ in ("DeepLabV3Plus", "UNet", "YOLOSeg", "WaterNet", "MSWNet"))
