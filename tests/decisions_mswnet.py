"""Decision bookkeeping for the MSWNet tests (test infrastructure): the 3x3 stride-1 pool's winner bytes against ATen's flat indices, and the HIP
step's decisions collected in tests/mswnet_ref.py's DECISION_SITES order for tests/decisions_seq.py's two-part check.  A 3x3-pool winner on which
the two sides differ is judged by the same rule as a 2x2 one (decisions.NEAR_TIE through decisions_seq.assert_near_ties)."""
import torch

from decisions_seq import pool_flat_2x2


def pool_flat_3s1(code, w_in):
    """HIP MaxPool2d(3, 1, 1) winner byte (dy * 3 + dx) [n, c, h, w] -> ATen flat index into the input plane"""
    n, c, h, w = code.shape
    oh = torch.arange(h).view(1, 1, -1, 1)
    ow = torch.arange(w).view(1, 1, 1, -1)
    return (oh - 1 + code // 3) * w_in + ow - 1 + code % 3


def pool_code_3s1(flat, w_in):
    """ATen flat index [n, c, h, w] of a MaxPool2d(3, 1, 1) -> window position dy * 3 + dx"""
    n, c, h, w = flat.shape
    oh = torch.arange(h).view(1, 1, -1, 1)
    ow = torch.arange(w).view(1, 1, 1, -1)
    return (flat // w_in - oh + 1) * 3 + (flat % w_in - ow + 1)


def hip_decisions(B, C, mref):
    """C: the context mswnet_forward saved.  -> the step's decisions in mref.DECISION_SITES order (bool masks / ATen flat pool indices, CPU).
    An encoder level's four ReLU masks are read off its activation (the skip half of the decoder's concat buffer: e > 0 exactly where the
    BatchNorm output was); the bridge's and the decoder's come from the saved BatchNorm inputs and coefficients with bn_apply's arithmetic."""
    dec = []
    for lvl in (1, 2, 3, 4):
        cat = C[f"dec{lvl}.0"]["x"]
        ch = cat.shape[3] // 2
        q = ch // 4
        act = (cat[..., ch:] > 0).permute(0, 3, 1, 2).cpu()
        w_in = cat.shape[2]
        for b in range(4):
            if b == 3 and lvl > 1:
                dec.append(pool_flat_3s1(C["encs"][lvl]["idx"].permute(0, 3, 1, 2).cpu().long(), w_in))
            dec.append(act[:, b * q:(b + 1) * q].contiguous())
        dec.append(pool_flat_2x2(C["pools"][lvl].permute(0, 3, 1, 2).cpu().long(), w_in))
    for k in ("bridge.0", "bridge.3", "dec4.0", "dec3.0", "dec2.0", "dec1.0"):
        dec.append((B.bn_apply(C[k]["t"], C[k]["s"], C[k]["h"], None, relu=True) > 0).permute(0, 3, 1, 2).cpu())
    return dec
