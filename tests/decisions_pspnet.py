"""Decision bookkeeping for the PSPNet tests (test infrastructure): the HIP step's decisions collected in tests/pspnet_ref.py's DECISION_SITES
order for tests/decisions_seq.py's two-part check.  Every decision is a ReLU mask."""


def hip_decisions(B, C, pref):
    """C: the context pspnet_forward saved.  -> the step's ReLU masks in pref.DECISION_SITES order (bool [n, c, h, w], CPU), each from the
    saved BatchNorm input and coefficients with bn_apply's arithmetic (the head kernels evaluate the same bn_pre expression)."""
    def mask(cx):
        return (B.bn_apply(cx["t"], cx["s"], cx["h"], None, relu=True) > 0).permute(0, 3, 1, 2).cpu()
    dec = [mask(C[name]) for name, _, _ in pref.BACKBONE]
    dec += [mask(b) for b in C["ppm"]["br"]]
    dec.append(mask(C["fin"]))
    assert len(dec) == len(pref.DECISION_SITES)
    return dec
