"""Decision bookkeeping for the Fast-SCNN tests (test infrastructure): the HIP step's decisions collected in tests/fastscnn_ref.py's
DECISION_SITES order for tests/decisions_seq.py's two-part check.  Every decision is a ReLU mask."""


def hip_decisions(B, C, fref):
    """C: the context fastscnn_forward saved.  -> the step's ReLU masks in fref.DECISION_SITES order (bool [n, c, h, w], CPU).  The masks
    behind a BatchNorm come from the saved BatchNorm inputs and coefficients with bn_apply's arithmetic, the fusion's from its output (y > 0
    exactly where the sum was)."""
    def mask(cx):
        return (B.bn_apply(cx["t"], cx["s"], cx["h"], None, relu=True) > 0).permute(0, 3, 1, 2).cpu()
    sep = C["sep"]
    dec = [mask(C["stem"])]
    dec += [mask(sep[name]) for name, _, _, _ in fref.SEP_HEAD + fref.SEP_TRUNK]
    dec += [mask(b) for b in C["ppm"]["br"]]
    dec.append((C["y"] > 0).permute(0, 3, 1, 2).cpu())
    dec += [mask(sep[name]) for name, _, _, _ in fref.SEP_TAIL]
    assert len(dec) == len(fref.DECISION_SITES)
    return dec
