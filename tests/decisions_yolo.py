"""Decision-aware gradient parity for YOLOSeg (tests/yolo_ref.py): tests/decisions_seq.py's recorder, extended to `F.leaky_relu`.  A
LeakyReLU branch is logged as the mask z > 0 (kind "relu", so decisions_seq.differing / assert_near_ties treat it like a ReLU mask: a
differing branch must be a near-tie |z| <= NEAR_TIE); forced, the factor is 1 where the mask holds and the slope elsewhere.  Pool winners
are decisions_seq's.  Test infrastructure; the oracle is the checker."""
import torch
import torch.nn.functional as F

from decisions_seq import SeqRecorder


class LeakyRecorder(SeqRecorder):
    def leaky_relu(self, x, negative_slope=0.01, inplace=False):
        f = self._f()
        self.log.append(("relu", (x > 0).detach().clone(), x.detach().clone()))
        if f is None:
            return F.leaky_relu(x, negative_slope)
        return x * torch.where(f, torch.ones((), dtype=x.dtype), torch.full((), negative_slope, dtype=x.dtype))


def run_oracle(mod, step, forced=None):
    """step(rec) -> (loss_fn, prob, logit); -> (recorder log, prob detached)"""
    rec = LeakyRecorder(forced)
    real = mod.F
    mod.F = rec
    try:
        loss_fn, prob, _ = step(rec)
        loss_fn(prob).backward()
    finally:
        mod.F = real
    return rec.log, prob.detach().clone()
