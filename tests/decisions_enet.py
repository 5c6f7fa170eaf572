"""Decision bookkeeping for the ENet tests (test infrastructure): the HIP step's decisions collected in tests/enet_ref.py's DECISION_SITES
order for tests/decisions_seq.py's two-part check.  Every decision is a ReLU mask."""


def hip_decisions(B, C, eref):
    """C: the context enet_forward saved.  -> the step's ReLU masks in eref.DECISION_SITES order (bool [n, c, h, w], CPU).  The masks behind a
    BatchNorm come from the saved BatchNorm inputs and coefficients with bn_apply's arithmetic, a bottleneck's last one from its output
    (out > 0 exactly where the sum was)."""
    def mask(cx):
        return (B.bn_apply(cx["t"], cx["s"], cx["h"], None, relu=True) > 0).permute(0, 3, 1, 2).cpu()
    dec = [mask(C["initial"])]
    for name, _, _, _, asym, _, _ in eref.BLOCKS:
        cx = C["blocks"][name]
        assert len(cx["stages"]) == (3 if asym else 2)
        dec += [mask(st) for st in cx["stages"]]
        dec.append((cx["out"] > 0).permute(0, 3, 1, 2).cpu())
    dec += [mask(C["d0"]), mask(C["d3"])]
    assert len(dec) == len(eref.DECISION_SITES)
    return dec
