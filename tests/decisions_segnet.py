"""Decision-aware gradient parity for SegNet (tests/segnet_ref.py): tests/decisions_seq.py's recorder, extended to
`F.max_pool2d(..., return_indices=True)` so that a forced pool winner also drives the `F.max_unpool2d` that consumes the indices.
Test infrastructure; the oracle is the checker."""
import torch
import torch.nn.functional as F

from decisions_seq import SeqRecorder


class PoolIndexRecorder(SeqRecorder):
    def max_pool2d(self, x, kernel_size, stride=None, padding=0, return_indices=False):
        if not return_indices:
            return super().max_pool2d(x, kernel_size, stride, padding)
        f = self._f()
        y, idx = F.max_pool2d(x, kernel_size, stride, padding, return_indices=True)
        self.log.append(("pool", idx.detach().clone(), x.detach().clone()))
        if f is not None:        # f: flat index h * W + w into the input plane, [n, c, ho, wo]
            n, c, h, w = x.shape
            idx = f.to(idx.dtype).reshape(idx.shape)
            y = torch.gather(x.reshape(n, c, h * w), 2, idx.reshape(n, c, -1)).reshape(y.shape)
        return y, idx


def run_oracle(mod, step, forced=None):
    """decisions_seq.run_oracle with the index-aware recorder.  step(rec) -> (loss_fn, prob, logit); -> (recorder log, prob detached)"""
    rec = PoolIndexRecorder(forced)
    real = mod.F
    mod.F = rec
    try:
        loss_fn, prob, _ = step(rec)
        loss_fn(prob).backward()
    finally:
        mod.F = real
    return rec.log, prob.detach().clone()
