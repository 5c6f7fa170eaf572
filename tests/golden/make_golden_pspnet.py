#!/usr/bin/env python3
"""Generate the PSPNet golden vectors (tests/golden/pspnet_*.{json,npz}) from the REFERENCE itself.

Runs only where the reference checkout is present (never on the GPU box).  Like make_golden_enet.py it imports the reference's second
comparison script, comne.py, in-process with empty `torchvision` stub modules (the file imports torchvision.transforms at the top; the
model never touches it), fills `comne.PSPNet` from the portable generator (tests/pspnet_ref.init_state: torch's default-init distributions,
jittered BatchNorm affine parameters), replaces final_conv's Dropout2d (`final_conv[3]`) by a module that multiplies with an injected
keep-mask (tests/pspnet_ref.dropout_masks), runs one train step (nn.BCELoss + Adam 1e-4, weight decay 1e-4, comne.py:650-651) and an eval
forward on portable inputs, and stores inputs-by-seed + outputs in Fast-SCNN's sampling scheme (sampled gradients and Adam results with
`/meta`).  Nothing from the reference's source is copied: the fixtures are data (tensors, scalars, key lists).

Usage:  python tests/golden/make_golden_pspnet.py [path/to/reference checkout]   (or REFERENCE_DIR=...)
"""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

for name in ("torchvision", "torchvision.transforms"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
import matplotlib  # noqa: E402

matplotlib.use("Agg")
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE_DIR", os.path.join(os.path.dirname(ROOT), "reference"))   # default: a sibling checkout
sys.path.insert(0, REF)
comne = importlib.import_module("comne")

pref = importlib.import_module("pspnet_ref")
pkg_data = importlib.import_module("eusipco-2026-robust-unet_amd.data")

torch.set_num_threads(8)
torch.manual_seed(0)


class InjectedDropout2d(torch.nn.Module):
    """Stands in for the reference's nn.Dropout2d so the Bernoulli draw is reproducible."""

    def __init__(self, mask):
        super().__init__()
        self.mask = mask

    def forward(self, x):
        return x * self.mask[:, :, None, None] if self.training else x


def put(out, key, t, full=False, nsample=1024):
    t = t.detach()
    if full:
        out[key] = t.float().numpy()
        return
    flat = t.double().reshape(-1)
    stride = max(1, flat.numel() // nsample)
    out[key + "/sample"] = flat[::stride][:nsample].float().numpy()
    out[key + "/meta"] = np.array([stride, flat.numel(), nsample], dtype=np.int64)


def pspnet_case(n, size, seed, tag):
    out = {}
    model = comne.PSPNet(n_classes=1)
    st = pref.init_state(seed=seed, perturb_bn=True)
    res = model.load_state_dict(st, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    masks = pref.dropout_masks(n, seed)
    dropped = int((masks["final_conv.3"] == 0).sum())
    assert dropped > 0, "the fixture's mask must drop at least one channel"
    model.final_conv[3] = InjectedDropout2d(masks["final_conv.3"])
    x, y = pkg_data.synthetic_batch(n, size, seed=seed)
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-4, weight_decay=1e-4)
    opt.zero_grad()
    prob = model(x)
    loss = torch.nn.BCELoss()(prob, y)
    loss.backward()
    put(out, "prob", prob, full=size <= 64)
    out["loss"] = np.array(loss.item(), dtype=np.float64)
    names = [k for k, _ in model.named_parameters()]
    out["grad_norm"] = np.array([p.grad.double().norm().item() for _, p in model.named_parameters()])
    for k, p in model.named_parameters():
        put(out, "grad/" + k, p.grad, full=p.numel() <= 1024)
    for k, b in model.named_buffers():
        if not k.endswith("num_batches_tracked"):
            put(out, "buf/" + k, b, full=True)
    opt.step()
    out["param_delta_abs_sum"] = np.array([(p.detach().double() - st[k].double()).abs().sum().item() for k, p in model.named_parameters()])
    for k, p in model.named_parameters():
        put(out, "adam/" + k, p, full=p.numel() <= 1024, nsample=256)
    model.eval()
    with torch.no_grad():
        pe = model(x)
    put(out, "eval_prob", pe, full=size <= 64)
    np.savez_compressed(os.path.join(HERE, f"pspnet_{tag}.npz"), **out)
    with open(os.path.join(HERE, f"pspnet_{tag}.json"), "w") as f:
        json.dump({"n": n, "size": size, "seed": seed, "param_names": names, "n_params": sum(p.numel() for p in model.parameters()),
                   "dropped": dropped}, f, indent=1)
    print("pspnet", tag, "loss", loss.item(), "dropped", dropped, "bytes", os.path.getsize(os.path.join(HERE, f"pspnet_{tag}.npz")))


def state_dict_case():
    model = comne.PSPNet(1)
    with open(os.path.join(HERE, "pspnet_state_dict.json"), "w") as f:
        json.dump({"state_dict": [[k, list(v.shape), str(v.dtype)] for k, v in model.state_dict().items()],
                   "n_params": sum(p.numel() for p in model.parameters())}, f, indent=0)


if __name__ == "__main__":
    state_dict_case()
    pspnet_case(n=2, size=64, seed=17, tag="n2_s64")       # H/16 map 4 x 4: the 6-bin branch is resized DOWN, the 3-bin windows overlap
    pspnet_case(n=3, size=96, seed=19, tag="n3_s96")       # 6 x 6, three images: the 6-bin pool is the identity, the 3-bin windows are 2 x 2
