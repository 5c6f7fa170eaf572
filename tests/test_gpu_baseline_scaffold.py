"""GPU: the autograd node the seven single-node baselines share (baseline._FusedFn) at 2 x 3 x 32 x 32, the smallest size all of them take
(SegFormerLite needs multiples of 32; MSWNet's bridge is 2 x 2 there): gradient accumulation through ops.deliver_grads, the fixed gradient
addresses graph capture relies on, and the refusal of a second backward."""
import pytest
import torch

pytestmark = pytest.mark.gpu

MODELS = ("UNet", "SegNet", "YOLOSeg", "SegFormerLite", "HRNetWater", "WaterNet", "MSWNet")


@pytest.mark.parametrize("name", MODELS)
def test_accumulation_addresses_and_second_backward(pkg, name):
    dev = torch.device("cuda")
    torch.manual_seed(11)
    net = getattr(pkg, name)().to(dev).train()
    x = torch.randn(2, 3, 32, 32).to(dev)
    w = torch.randn(2, net.n_classes, 32, 32).to(dev)          # a fixed, non-uniform output gradient
    params = list(net.named_parameters())

    def step(**kw):
        out = net(x)
        assert out.shape == w.shape
        (out * w).sum().backward(**kw)
        return out

    step()
    torch.cuda.synchronize()
    g1 = {k: p.grad.clone() for k, p in params}
    ptr = {k: p.grad.data_ptr() for k, p in params}
    assert all(g.shape == p.shape and bool(torch.isfinite(g).all()) for (k, p), g in zip(params, g1.values()))
    assert any(bool(g.abs().max() > 0) for g in g1.values())
    # a second step on top of the first one's gradients: the steps are bit-deterministic (each model's own test file asserts it) and x + x is
    # exact in fp32, so the accumulated gradient is exactly twice the first
    step()
    torch.cuda.synchronize()
    for k, p in params:
        assert torch.equal(p.grad, 2 * g1[k]), k
    # from cleared gradients: delivered to the addresses of the first step
    for _, p in params:
        p.grad = None
    out = step(retain_graph=True)
    torch.cuda.synchronize()
    for k, p in params:
        assert p.grad.data_ptr() == ptr[k], k
        assert torch.equal(p.grad, g1[k]), k
    with pytest.raises(RuntimeError, match="called twice"):
        (out * w).sum().backward()
