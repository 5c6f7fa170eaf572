"""Writes tests/golden/attention_host.json: the host-side decisions of csrc/attention.hip (workspace sizes, refusal messages) as one build of
the library makes them.  Nothing here launches a kernel - every recorded call is refused by a RUNET_REQUIRE - so it runs without a GPU, and
must: the refusal calls pass made-up pointers.

    RUNET_HIP_LIB=<librunet_hip.so of the commit to record> python tests/golden/make_golden_attention_host.py

tests/test_attention_host.py imports the grids and the collectors below, so the golden and the test cannot drift apart."""
import ctypes
import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "attention_host.json")
PKG = "eusipco-2026-robust-unet_amd"

# (n, h, w, c): the shapes of tools/abi_bits.py's attention cases and tests/attention_ref.py, then the training shapes of the network and the caps
SHAPES = ((2, 20, 36, 64), (2, 8, 8, 48), (1, 2, 2, 1024), (3, 6, 10, 16), (1, 4, 4, 256), (1, 1, 1, 4), (2, 16, 16, 128), (16, 256, 256, 64),
          (16, 128, 128, 128), (16, 64, 64, 256), (16, 32, 32, 512), (16, 16, 16, 1024), (2, 64, 64, 64), (1, 1024, 1024, 64), (1, 2048, 2048, 1024),
          (3, 17, 33, 12), (1, 1, 300, 8))
CR = (1, 3, 4, 16, 64)
GATE_F = (4, 8, 12, 32, 64, 128, 256, 512, 1024)


def load():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module(PKG + "._lib")


# ------------------------------------------------------------------------------------------------ workspaces
def ws_cases():
    return {"runet_sa_conv7_bwd_workspace_floats": [(n, h, w) for n, h, w, _ in SHAPES],
            "runet_rb_bwd2_bn_workspace_floats": [(n, h * w, c) for n, h, w, c in SHAPES],
            "runet_ca_bwd_workspace_floats": [(n, c, cr) for n, _, _, c in SHAPES for cr in CR if cr <= c],
            "runet_ag_bwd2_bn_workspace_floats": [(n * h * w, f) for n, h, w, _ in SHAPES for f in GATE_F]}


def sizes(lib):
    return {fn: [getattr(lib, fn)(*c) for c in cases] for fn, cases in ws_cases().items()}


# ------------------------------------------------------------------------------------------------ refusals
# Dummy 16-byte aligned addresses: every call below is refused by a RUNET_REQUIRE before anything is launched.
P = 0x1000
C4 = "channels must be a multiple of 4"


def _ptrs(*names):
    return [(k, P + 0x100 * i) for i, k in enumerate(names)]


_TAIL = _ptrs("t2") + [("ld", 64)] + _ptrs("A", "B", "sa", "r") + [("ldr", 64)] + _ptrs("rs", "rh", "out") + [("ldo", 64)]
_OUT = _TAIL + [("pixels", 32), ("hw", 16), ("c", 64), ("st", 0)]
_OUT_EX = _TAIL + _ptrs("bits", "pooled") + [("ldp", 64)] + _ptrs("pidx") + [("n", 2), ("h", 4), ("w", 4), ("c", 64), ("st", 0)]
_B1_TAIL = _ptrs("t2") + [("ld", 64)] + _ptrs("A", "B", "sa", "dv") + [("lddv", 64)] + _ptrs("dq")
_BWD1 = _ptrs("dout") + [("lddo", 64)] + _ptrs("out") + [("ldo", 64)] + _B1_TAIL + [("pixels", 32), ("hw", 16), ("c", 64), ("st", 0)]
_BWD1_EX = (_ptrs("dout") + [("lddo", 64)] + _ptrs("dpool") + [("ldp", 64)] + _ptrs("pidx", "out") + [("ldo", 64)] + _ptrs("bits") + _B1_TAIL
            + [("n", 2), ("h", 4), ("w", 4), ("c", 64), ("st", 0)])
_B2_HEAD = _ptrs("dv") + [("lddv", 64)] + _ptrs("t2") + [("ld", 64)] + _ptrs("sa", "dsm", "amax")
_BWD2 = _B2_HEAD + [("n", 2), ("hw", 16), ("c", 64)] + _ptrs("ws", "sdu", "sdut") + [("st", 0)]
_BWD2_BN = (_B2_HEAD + _ptrs("r") + [("ldr", 64)] + _ptrs("mean_s", "invstd_s") + [("n", 2), ("hw", 16), ("c", 64)] + _ptrs("ws") + [("wsf", 1 << 20)]
            + _ptrs("sdu", "sdut", "sums_s") + [("st", 0)])
_B3_HEAD = _B2_HEAD + _ptrs("ca", "davg", "dmx", "idx", "mean2", "invstd2", "s2", "sums2", "dt2") + [("lddt", 64)]
_B3_TAIL = [("pixels", 32), ("hw", 16), ("c", 64), ("m_total", 0), ("st", 0)]
_BWD3 = _B3_HEAD + _B3_TAIL
_BWD3_SC = _B3_HEAD + _ptrs("r") + [("ldr", 64)] + _ptrs("mean_s", "invstd_s", "scale_s", "sums_s") + [("m_total_s", 0)] + _B3_TAIL
_CA_COEFF = (_ptrs("mean_nc", "max_nc", "min_nc", "imax", "imin", "s2", "h2", "w0p", "w2p") + [("n", 2), ("c", 64), ("cr", 4)]
             + _ptrs("A", "B", "ca", "avg", "mx", "idx", "tval") + [("st", 0)])
_CA_BWD = (_ptrs("sdu", "sdut", "s2", "h2", "ca", "avg", "mx", "w0p", "w2p", "mean_nc", "tval", "mean2", "invstd2") + [("n", 2), ("c", 64), ("cr", 4)]
           + _ptrs("ws", "davg", "dmx", "sums2", "dw0p", "dw2p") + [("st", 0)])
_AG_HEAD = _ptrs("g1") + [("ldg", 64)] + _ptrs("x1") + [("ldx", 64)] + _ptrs("sg", "hg", "sx", "hx", "wpsi")
_AG_BWD2 = _ptrs("ds") + _AG_HEAD + _ptrs("dpre") + [("ldp", 64)] + _ptrs("ws", "dw") + [("pixels", 32), ("f", 64), ("st", 0)]
_AG_BWD2_BN = (_ptrs("ds") + _AG_HEAD + _ptrs("mean_g", "invstd_g", "mean_x", "invstd_x", "dpre") + [("ldp", 64)] + _ptrs("ws") + [("wsf", 1 << 20)]
               + _ptrs("dw", "sums_g", "sums_x") + [("pixels", 32), ("f", 64), ("st", 0)])

# (function, [(argument, good value)...], [(overrides, the RUNET_REQUIRE message it must hit)...]).  At least one call per RUNET_REQUIRE line of
# the entry point, in the order of the source.
REFUSALS = [
    ("runet_ca_coeff", _CA_COEFF,
     [(dict(mean_nc=0), "null pointer"), (dict(B=0), "null pointer"), (dict(c=66), C4), (dict(c=2048), C4), (dict(cr=0), "bad hidden width"),
      (dict(cr=65), "bad hidden width"), (dict(mx=0), "save buffers must come together"), (dict(tval=0), "save buffers must come together")]),
    ("runet_sa_reduce", _ptrs("t2") + [("ld", 64)] + _ptrs("A", "B") + [("pixels", 32), ("hw", 16), ("c", 64)] + _ptrs("smap", "amax") + [("st", 0)],
     [(dict(t2=0), "null pointer"), (dict(amax=0), "null pointer"), (dict(c=0), C4)]),
    ("runet_sa_conv7", _ptrs("smap", "wp", "sa") + [("n", 2), ("h", 4), ("w", 4), ("st", 0)], [(dict(smap=0), "null pointer"), (dict(sa=0), "null pointer")]),
    ("runet_rb_out", _OUT,
     [(dict(t2=0), "null pointer"), (dict(out=0), "null pointer"), (dict(c=6), C4), (dict(pixels=33), "pixels must be a whole number of images")]),
    ("runet_rb_bwd1", _BWD1, [(dict(dout=0), "null pointer"), (dict(dq=0), "null pointer"), (dict(c=1028), C4)]),
    ("runet_rb_out_ex", _OUT_EX,
     [(dict(r=0), "null pointer"), (dict(c=2), C4), (dict(n=0), "bad shape"), (dict(w=0), "bad shape"), (dict(pidx=0), "pooled and pool_idx come together"),
      (dict(pooled=0), "pooled and pool_idx come together"), (dict(h=65536, w=32768), "image too large"), (dict(h=3), "h and w must be even"),
      (dict(w=6, h=5), "h and w must be even"), (dict(ldp=60), "bad pooled stride"), (dict(ldp=66), "bad pooled stride")]),
    ("runet_rb_bwd1_ex", _BWD1_EX,
     [(dict(sa=0), "null pointer"), (dict(c=0), C4), (dict(h=0), "bad shape"), (dict(h=65536, w=32768), "bad shape"),
      (dict(pidx=0), "dpool and pool_idx come together"), (dict(dpool=0), "dpool and pool_idx come together"), (dict(w=5), "pooled gradient"),
      (dict(ldp=32), "pooled gradient"), (dict(ldp=70), "pooled gradient")]),
    ("runet_sa_conv7_bwd", _ptrs("smap", "dq", "wp", "dsm", "dwp", "ws") + [("n", 2), ("h", 4), ("w", 4), ("st", 0)],
     [(dict(dq=0), "null pointer"), (dict(ws=0), "null pointer")]),
    ("runet_rb_bwd2", _BWD2, [(dict(dv=0), "null pointer"), (dict(sdut=0), "null pointer"), (dict(c=10), C4)]),
    ("runet_rb_bwd2_bn", _BWD2_BN,
     [(dict(r=0), "null pointer"), (dict(sums_s=0), "null pointer"), (dict(c=10), C4), (dict(ldr=32), "bad stride / workspace too small"),
      (dict(ldr=66), "bad stride / workspace too small"), (dict(wsf=64), "bad stride / workspace too small")]),
    ("runet_ca_bwd", _CA_BWD, [(dict(sdu=0), "null pointer"), (dict(dw2p=0), "null pointer"), (dict(c=3), C4)]),
    ("runet_rb_bwd3", _BWD3, [(dict(idx=0), "null pointer"), (dict(dt2=0), "null pointer"), (dict(c=1030), C4), (dict(pixels=31), "pixels must be a whole number of images")]),
    ("runet_rb_bwd3_sc", _BWD3_SC,
     [(dict(dv=0), "null pointer"), (dict(r=0), "null pointer (shortcut BatchNorm)"), (dict(sums_s=0), "null pointer (shortcut BatchNorm)"), (dict(c=6), C4),
      (dict(pixels=40), "pixels must be a whole number of images"), (dict(ldr=32), "bad stride"), (dict(ldr=70), "bad stride")]),
    ("runet_ag_psi", _AG_HEAD + _ptrs("bpsi", "s") + [("pixels", 32), ("f", 64), ("st", 0)], [(dict(x1=0), "null pointer"), (dict(s=0), "null pointer"), (dict(f=6), C4)]),
    ("runet_ag_out", _ptrs("xs") + [("ldx", 64)] + _ptrs("s", "sp", "hp", "out") + [("ldo", 64), ("pixels", 32), ("c", 64), ("st", 0)],
     [(dict(xs=0), "null pointer"), (dict(out=0), "null pointer"), (dict(c=0), C4)]),
    ("runet_ag_bwd1", _ptrs("datt") + [("ldd", 64)] + _ptrs("xs") + [("ldx", 64)] + _ptrs("s", "sp", "hp", "dxs") + [("lddx", 64)] + _ptrs("dsbn")
     + [("pixels", 32), ("c", 64), ("st", 0)], [(dict(datt=0), "null pointer"), (dict(dsbn=0), "null pointer"), (dict(c=2), C4)]),
    ("runet_ag_bwd2", _AG_BWD2, [(dict(ds=0), "null pointer"), (dict(dw=0), "null pointer"), (dict(f=2), C4)]),
    ("runet_ag_bwd2_bn", _AG_BWD2_BN,
     [(dict(mean_x=0), "null pointer"), (dict(sums_x=0), "null pointer"), (dict(f=1026), C4), (dict(wsf=64), "workspace too small (runet_ag_bwd2_bn_workspace_floats)")]),
    ("runet_outc_fwd", _ptrs("x") + [("ld", 64)] + _ptrs("w", "b", "logit", "prob") + [("pixels", 32), ("c", 64), ("st", 0)],
     [(dict(x=0), "null pointer"), (dict(prob=0), "null pointer"), (dict(c=6), C4)]),
    ("runet_outc_bwd", _ptrs("dprob", "prob", "x") + [("ld", 64)] + _ptrs("w", "dx") + [("lddx", 64)] + _ptrs("ws", "dw_db") + [("pixels", 32), ("c", 64), ("st", 0)],
     [(dict(dprob=0), "null pointer"), (dict(dw_db=0), "null pointer"), (dict(c=6), C4)]),
]

# RUNET_REQUIRE lines without a call above, and why
SKIPPED = {
    "runet_rb_bwd2_bn / runet_ag_bwd2_bn: \"LDS budget\"":
        "unreachable behind the channel check: 256 / (c / 4) row groups of 4 c (4 f + 1) floats stay below 17 KiB for every accepted width",
}

# The one refusal the library gained after the recording: runet_rb_bwd1 now asks for whole images, in the words of runet_rb_out.
RB_BWD1_PIXELS = ("runet_rb_bwd1", dict(pixels=33), "runet_rb_out")


def call(mod, fn, over):
    """-> (return code, runet_last_error()) of one call of fn with its good arguments and the overrides"""
    good = next(g for f, g, _ in REFUSALS if f == fn)
    argtypes = mod.PROTOS[fn][1]
    assert len(argtypes) == len(good), fn
    assert set(over) <= {k for k, _ in good}, (fn, over)
    vals = [over.get(k, v) for k, v in good]
    args = [ctypes.c_void_p(v) if t is ctypes.c_void_p else v for t, v in zip(argtypes, vals)]
    mod.lib.runet_set_error(b"")
    rc = getattr(mod.lib, fn)(*args)
    return rc, mod.lib.runet_last_error().decode()


def refusals(mod):
    """-> [[function, overrides as text, return code, runet_last_error()]]; asserts that the call hit the RUNET_REQUIRE it was written for"""
    out = []
    for fn, _, cases in REFUSALS:
        for over, text in cases:
            rc, msg = call(mod, fn, over)
            assert rc == 1 and msg.startswith(fn + ": ") and text in msg, (fn, over, rc, msg)
            out.append([fn, json.dumps(over, sort_keys=True), rc, msg])
    return out


def dump(gold):
    """one line per refusal and per workspace function"""
    d = lambda v: json.dumps(v, sort_keys=True)
    rows = ",\n".join(d(r) for r in gold["refusals"])
    wss = ",\n".join(f"{d(k)}: {d(v)}" for k, v in sorted(gold["workspaces"].items()))
    return (f'{{"library": {d(gold["library"])},\n"refusals": [\n{rows}\n],\n"skipped": {d(gold["skipped"])},\n"workspaces": {{\n{wss}\n}}}}\n')


def gpu_visible():
    import torch
    return torch.cuda.is_available()


def main():
    assert not gpu_visible(), "record on a machine without a GPU: a refusal lost in the recorded library would launch on made-up pointers"
    mod = load()
    gold = {"library": "recorded from the parent of the commit that added this file; regenerate only against a library whose host decisions are the reference",
            "workspaces": sizes(mod.lib), "refusals": refusals(mod), "skipped": SKIPPED}
    with open(GOLDEN, "w") as f:
        f.write(dump(gold))
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes;", len(gold["refusals"]), "refusals;", sum(len(v) for v in gold["workspaces"].values()), "workspace sizes")


if __name__ == "__main__":
    main()
