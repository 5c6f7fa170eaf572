"""The C-ABI calls behind the Robust U-Net's block functions, in order: per call the entry point's name, which of its pointer arguments are
given (1) or NULL (0), and its integer arguments.  Prints one line per configuration - the number of calls and a SHA-256 over their lines -
or, with --calls, every call.  Wraps the bound `lib.runet_*` functions (as tools/enet_step.py --launches
does) around
  rb_forward + rb_backward          64 -> 128 (convolution shortcut) and 128 -> 128 (identity) at 2 x 16 x 16, for every combination of
                                    train / eval, pool, need_dx, FUSED_RB_EDGES, FUSED_SHORTCUT_BN_SUMS and a single-process SyncBN stub
  upgate_forward + upgate_backward  128 -> 64 on a 2 x 16 x 16 skip, train / eval, FUSED_GATE_BN_SUMS, the stub
  ca_forward / ca_backward, sa_forward / sa_backward   once each
It uses only public functions of blocks.py, so the same file run in a checkout of another commit shows whether a change of the glue or of
the host launchers moved the call sequence: the two printouts must be equal (profiles/block_launches_*.txt).

runet_rb_out / runet_rb_out_ex and runet_rb_bwd1 / runet_rb_bwd1_ex are printed in one form each ("runet_rb_out*", "runet_rb_bwd1*": the
optional pointers, the strides, pixels, pixels per image, channels): with its optional arguments NULL the _ex entry point is the plain one,
and which of the two the glue calls for that case is not a property of the sequence.
  python tools/block_launches.py [--calls] [--out FILE]
"""
import argparse
import ctypes
import hashlib
import importlib
import itertools
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
importlib.import_module("eusipco-2026-robust-unet_amd")
B = importlib.import_module("eusipco-2026-robust-unet_amd.blocks")
L = importlib.import_module("eusipco-2026-robust-unet_amd._lib")
DEV = torch.device("cuda:0")
N, H, W = 2, 16, 16
LOG = []


def _given(a):
    return "1" if a else "0"


def _plain(name, a):
    types = L.PROTOS[name][1]
    ptrs = "".join(_given(v) for v, t in zip(a, types) if t in (ctypes.c_void_p, ctypes.c_char_p))
    ints = [int(v) for v, t in zip(a, types) if t in (ctypes.c_int, ctypes.c_long)]
    return f"{name} ptrs={ptrs} ints={ints}"


# (rs, relu_bits, pooled | ld, ldr, ldo, ldp | pixels, hw, c)  and  (dpool, out, relu_bits | lddo, ldp, ldo, ld, lddv | pixels, hw, c)
CANON = {
    "runet_rb_out": lambda a: ("runet_rb_out*", (a[7], None, None), (a[1], a[6], a[10], 0), (a[11], a[12], a[13])),
    "runet_rb_out_ex": lambda a: ("runet_rb_out*", (a[7], a[11], a[12]), (a[1], a[6], a[10], a[13]), (a[15] * a[16] * a[17], a[16] * a[17], a[18])),
    "runet_rb_bwd1": lambda a: ("runet_rb_bwd1*", (None, a[2], None), (a[1], 0, a[3], a[5], a[10]), (a[12], a[13], a[14])),
    "runet_rb_bwd1_ex": lambda a: ("runet_rb_bwd1*", (a[2], a[5], a[7]), (a[1], a[3], a[6], a[9], a[14]), (a[16] * a[17] * a[18], a[17] * a[18], a[19])),
}


def _wrap(name, fn):
    def call(*a):
        if name in CANON:
            label, opt, lds, shape = CANON[name](a)
            LOG.append(f"{label} opt={''.join(_given(v) for v in opt)} ld={[int(v) for v in lds]} ints={[int(v) for v in shape]}")
        else:
            LOG.append(_plain(name, a))
        return fn(*a)
    return call


class SyncStub:
    """Single-process stand-in for the SyncBN hook: every collective returns its inputs with the local counts."""

    def gather_stats(self, mean_nc, m2_nc, n, c):
        LOG.append("sync.gather_stats")
        return mean_nc, m2_nc, n

    def gather_stats_many(self, local):
        LOG.append(f"sync.gather_stats_many {len(local)}")
        return [(m, m2, n) for m, m2, n, _ in local]

    def reduce_sums(self, sums, count):
        LOG.append(f"sync.reduce_sums {count}")
        return sums, count

    def reduce_sums_many(self, sums, counts):
        LOG.append(f"sync.reduce_sums_many {list(counts)}")
        return list(zip(sums, counts))


def rnd(*shape, scale=1.0):
    g = torch.Generator().manual_seed(sum(shape) + len(shape))
    return (scale * torch.randn(shape, generator=g)).to(DEV)


def bn(c):
    return B.BNState(1 + 0.1 * rnd(c), 0.1 * rnd(c), 0.1 * rnd(c), 1 + 0.1 * rnd(c).abs(), torch.zeros((), dtype=torch.int64, device=DEV))


def rb_params(cin, c):
    cr = max(c // 16, 1)
    return B.RBParams(rnd(3, 3, cin, c, scale=0.05), bn(c), rnd(3, 3, c, c, scale=0.05), bn(c), rnd(1, 1, c, cr, scale=0.1), rnd(1, 1, cr, c, scale=0.1),
                      rnd(7, 7, 2, 1, scale=0.1), rnd(1, 1, cin, c, scale=0.1) if cin != c else None, bn(c) if cin != c else None)


def upgate_params(cin, c):
    f = c // 2
    return B.UpGateParams(rnd(2, 2, cin, c, scale=0.05), 0.1 * rnd(c), rnd(1, 1, c, f, scale=0.1), 0.1 * rnd(f), bn(f), rnd(1, 1, c, f, scale=0.1),
                          0.1 * rnd(f), bn(f), rnd(1, 1, f, 1, scale=0.1), 0.1 * rnd(1), bn(1))


def section(title, fn):
    LOG.append(f"== {title}")
    fn()
    torch.cuda.synchronize()


def trace_rb():
    flags = ("train", "pool", "need_dx", "edges", "sc_sums", "sync")
    for cin, c in ((64, 128), (128, 128)):
        p = rb_params(cin, c)
        x, dout, dpool = rnd(N, H, W, cin), rnd(N, H, W, c), rnd(N, H // 2, W // 2, c)
        for cfg in itertools.product((True, False), repeat=len(flags)):
            train, pool, need_dx, edges, sc_sums, sync = cfg
            if sync and not train:
                continue
            B.FUSED_RB_EDGES, B.FUSED_SHORTCUT_BN_SUMS = edges, sc_sums

            def run():
                res = B.rb_forward(x, p, train, stats_hook=SyncStub() if sync else None, pool=pool)
                if pool:
                    B.rb_backward(res[1], dout.clone(), B.DictSink(DEV), need_dx=need_dx, dpool=dpool, pool_idx=res[3])
                else:
                    B.rb_backward(res[1], dout.clone(), B.DictSink(DEV), need_dx=need_dx)
            section(f"rb {cin}->{c} " + " ".join(f"{k}={int(v)}" for k, v in zip(flags, cfg)), run)


def trace_upgate():
    cin, c = 128, 64
    p = upgate_params(cin, c)
    y, skip, dcat = rnd(N, H // 2, W // 2, cin), rnd(N, H, W, c), rnd(N, H, W, 2 * c)
    for train, gate_sums, sync in itertools.product((True, False), repeat=3):
        if sync and not train:
            continue
        B.FUSED_GATE_BN_SUMS = gate_sums

        def run():
            _, ctx = B.upgate_forward(y, skip, p, train, stats_hook=SyncStub() if sync else None)
            B.upgate_backward(ctx, dcat.clone(), B.DictSink(DEV), "att.", "up.")
        section(f"upgate {cin}->{c} train={int(train)} gate_sums={int(gate_sums)} sync={int(sync)}", run)


def trace_attention():
    c = 64
    x, dy = rnd(N, H, W, c), rnd(N, H, W, c)
    w0p, w2p, wsa = rnd(1, 1, c, 4, scale=0.1), rnd(1, 1, 4, c, scale=0.1), rnd(7, 7, 2, 1, scale=0.1)

    def ca():
        _, ctx = B.ca_forward(x, w0p, w2p)
        B.ca_backward(ctx, dy, B.DictSink(DEV))

    def sa():
        _, ctx = B.sa_forward(x, wsa)
        B.sa_backward(ctx, dy, B.DictSink(DEV))
    section("ca_forward + ca_backward", ca)
    section("sa_forward + sa_backward", sa)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--calls", action="store_true", help="print every call instead of one fingerprint per configuration")
    args = ap.parse_args()
    saved = (B.FUSED_RB_EDGES, B.FUSED_SHORTCUT_BN_SUMS, B.FUSED_GATE_BN_SUMS)
    real = {name: getattr(L.lib, name) for name in L.PROTOS}
    for name, fn in real.items():
        if name != "runet_last_error":
            setattr(L.lib, name, _wrap(name, fn))
    try:
        trace_rb()
        trace_upgate()
        trace_attention()
    finally:
        for name, fn in real.items():
            setattr(L.lib, name, fn)
        B.FUSED_RB_EDGES, B.FUSED_SHORTCUT_BN_SUMS, B.FUSED_GATE_BN_SUMS = saved
    lines = LOG
    if not args.calls:
        lines, heads = [], [i for i, l in enumerate(LOG) if l.startswith("== ")] + [len(LOG)]
        for a, b in zip(heads, heads[1:]):
            lines.append(f"{LOG[a]}  calls={b - a - 1} sha256={hashlib.sha256(chr(10).join(LOG[a + 1:b]).encode()).hexdigest()}")
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text, end="")
    print(f"{sum(1 for l in LOG if l.startswith('== '))} configurations, {sum(1 for l in LOG if not l.startswith('== '))} calls", file=sys.stderr)


if __name__ == "__main__":
    main()
