"""Writes tests/golden/igemm_host.json: the host-side decisions of csrc/conv_igemm.hip (kernel names, workspace sizes, statistics parts,
refusal messages) as one build of the library makes them.  Nothing here launches a kernel, so it runs without a GPU.

    RUNET_HIP_LIB=<librunet_hip.so of the commit to record> python tests/golden/make_golden_igemm_host.py

tests/test_igemm_host.py imports the grids and the collectors below, so the golden and the test cannot drift apart.  The two environment
knobs are read once per process by the library: every knob setting is collected in a child process of its own (`--child`)."""
import base64
import ctypes
import importlib
import json
import os
import subprocess
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "igemm_host.json")
PKG = "eusipco-2026-robust-unet_amd"

FWD, DGRAD, CONVT_FWD, CONVT_DGRAD, DGRAD_T, CONVT_DGRAD_T = range(6)
KNOBS = ("RUNET_IGEMM_GENERAL", "RUNET_IGEMM_OLD_TILES")      # each collected alone, set to "1"
SHAPES = ((1, 4, 4), (3, 9, 11), (2, 32, 32), (16, 64, 64), (16, 128, 128), (16, 256, 256))
MODE_KH = ((FWD, 1), (FWD, 3), (DGRAD, 1), (DGRAD, 3), (DGRAD_T, 1), (DGRAD_T, 3), (CONVT_FWD, 2), (CONVT_DGRAD, 2), (CONVT_DGRAD_T, 2))
NAME_CIN = (4, 8, 16, 20, 32, 48, 64, 128, 256, 512)
NAME_COUT = (4, 8, 32, 36, 64, 68, 128, 132, 256, 512)
FORCED = (-1, 0, 1, 2, 3, 4)
GEMM_BATCH, GEMM_ROWS = (1, 4, 36), (16, 77, 100, 256, 1024, 4096, 16384)
GEMM_K, GEMM_N = (4, 16, 20, 32, 64, 128), (4, 8, 32, 36, 64, 96, 100, 128, 256)
WS_CH = (4, 16, 64, 128, 512)
WS_KHKW = ((1, 1), (3, 3), (5, 1), (1, 5), (7, 7), (8, 8), (4, 4))
WS_BAD = ((0, 16, 16, 3, 3), (64, 0, 16, 3, 3), (64, 16, 0, 3, 3), (64, 16, 16, 0, 3), (64, 16, 16, 9, 3), (64, 16, 16, 3, 0), (64, 16, 16, 3, 9))


def load():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module(PKG + "._lib")


def pack(values):
    """a long list with few distinct values -> {"table": the distinct values, "idx": base64(zlib(uint16 indices))}"""
    table = sorted(set(values))
    pos = {v: i for i, v in enumerate(table)}
    assert len(table) < 65536
    raw = b"".join(pos[v].to_bytes(2, "little") for v in values)
    return {"table": table, "n": len(values), "idx": base64.b64encode(zlib.compress(raw, 9)).decode("ascii")}


def unpack(p):
    raw = zlib.decompress(base64.b64decode(p["idx"]))
    assert len(raw) == 2 * p["n"]
    return [p["table"][int.from_bytes(raw[i:i + 2], "little")] for i in range(0, len(raw), 2)]


# ------------------------------------------------------------------------------------------------ names
def conv_name_cases():
    return [(f, n, h, w, cin, cout, kh, mode) for f in FORCED for mode, kh in MODE_KH for n, h, w in SHAPES for cin in NAME_CIN for cout in NAME_COUT]


def conv_names(lib):
    out = []
    try:
        last = None
        for f, n, h, w, cin, cout, kh, mode in conv_name_cases():
            if f != last:
                assert lib.runet_igemm_force_variant(f) == 0
                last = f
            out.append(lib.runet_conv_igemm_kernel_name(n, h, w, cin, cout, kh, mode).decode())
    finally:
        lib.runet_igemm_force_variant(-1)
    return out


def gemm_name_cases():
    return [(b, r, k, n) for b in GEMM_BATCH for r in GEMM_ROWS for k in GEMM_K for n in GEMM_N]


def gemm_names(lib):
    return [lib.runet_gemm_batched_kernel_name(*c).decode() for c in gemm_name_cases()]


# ------------------------------------------------------------------------------------------------ workspaces and parts
def wgrad_ws_cases():
    return [(n, h, w, ci, co, k, k) for k in (1, 2, 3) for n, h, w in SHAPES for ci in WS_CH for co in WS_CH]


def pixel_ws_cases():
    good = [(n * h * w, ci, co, kh, kw) for kh, kw in WS_KHKW for n, h, w in SHAPES for ci in WS_CH for co in WS_CH]
    return good + list(WS_BAD)      # rect answers -1 to these; general has no argument check (recorded as it answers)


def parts_cases():
    return [(n, h, w, co) for n, h, w in SHAPES + ((0, 4, 4),) for co in NAME_COUT + (0,)]


def sizes(lib):
    return {"wgrad": [lib.runet_conv_wgrad_workspace_floats(*c) for c in wgrad_ws_cases()],
            "general": [lib.runet_conv_wgrad_general_workspace_floats(*c) for c in pixel_ws_cases() if c not in WS_BAD],
            "rect": [lib.runet_conv_wgrad_rect_workspace_floats(*c) for c in pixel_ws_cases()],
            "parts": [lib.runet_convt4_igemm_stats_parts(*c) for c in parts_cases()]}


def collect(lib):
    """every grid in this process's environment, packed"""
    out = {"conv_names": pack(conv_names(lib)), "gemm_names": pack(gemm_names(lib))}
    out.update({k: pack(v) for k, v in sizes(lib).items()})
    return out


def collect_child(knob):
    """collect() in a fresh process with one knob set to 1 (None: with both unset)"""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    if knob:
        env[knob] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


# ------------------------------------------------------------------------------------------------ refusals
# Dummy 16-byte aligned addresses: every call below is refused by a RUNET_REQUIRE before anything is launched.
X, W, Y, DW, WS, ST, ODD = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x1004

# (function, [(argument, good value)...], [(overrides, the RUNET_REQUIRE message it must hit)...]).  One call per RUNET_REQUIRE line of the entry
# point, in the order of the source.
_IG = [("x", X), ("ldx", 16), ("w", W), ("bias", 0), ("y", Y), ("ldy", 16), ("n", 1), ("h", 4), ("w_", 4), ("cin", 16), ("cin_w", 16), ("cout", 16),
       ("kh", 1), ("kw", 1), ("dil", 1), ("mode", FWD), ("acc", 0), ("st", 0)]
_WG = [("x", X), ("ldx", 16), ("dy", Y), ("ldy", 16), ("dw", DW), ("ws", WS), ("wsf", 1 << 20), ("n", 1), ("h", 4), ("w_", 4), ("cin", 16), ("cin_w", 16),
       ("cout", 16), ("kh", 1), ("kw", 1), ("dil", 1), ("tr", 0), ("st", 0)]
_GEN = [("x", X), ("ldx", 16), ("w", W), ("bias", 0), ("y", Y), ("ldy", 16), ("n", 1), ("hin", 8), ("win", 8), ("cin", 16), ("cin_w", 16), ("cout", 16),
        ("kh", 3), ("kw", 3), ("stride", 1), ("pad", 1), ("dil", 1), ("mode", FWD), ("acc", 0), ("st", 0)]
_RECT = _GEN[:15] + [("pad_h", 1), ("pad_w", 1), ("dil_h", 1), ("dil_w", 1), ("mode", FWD), ("acc", 0), ("st", 0)]
_T4 = [("x", X), ("ldx", 16), ("w", W), ("bias", 0), ("y", Y), ("ldy", 16), ("n", 1), ("h", 4), ("w_", 4), ("cin", 16), ("cout", 16), ("mode", CONVT_FWD),
       ("acc", 0), ("st", 0)]
_T4S = _T4[:11] + [("stats", ST), ("st", 0)]
_WGG = [("x", X), ("ldx", 16), ("dy", Y), ("ldy", 16), ("dw", DW), ("ws", WS), ("wsf", 1 << 20), ("n", 1), ("hin", 8), ("win", 8), ("cin", 16), ("cin_w", 16),
        ("cout", 16), ("kh", 3), ("kw", 3), ("stride", 1), ("pad", 1), ("dil", 1), ("tr4", 0), ("st", 0)]
_WGR = _WGG[:16] + [("pad_h", 1), ("pad_w", 1), ("dil_h", 1), ("dil_w", 1), ("st", 0)]
_T3 = [("x", X), ("ldx", 16), ("wq", W), ("bias", 0), ("y", Y), ("ldy", 16), ("n", 1), ("h", 4), ("w_", 4), ("cin", 16), ("cout", 16), ("st", 0)]
_GB = [("a", X), ("lda", 16), ("sa", 64), ("b", W), ("sb", 256), ("c", Y), ("ldc", 16), ("sc", 64), ("batch", 1), ("rows", 4), ("k", 16), ("n", 16), ("st", 0)]
_GT = [("a", X), ("lda", 16), ("sa", 64), ("b", W), ("ldb", 16), ("sb", 64), ("c", Y), ("batch", 1), ("rows", 64), ("k", 16), ("n", 16), ("rps", 16), ("st", 0)]
_K2 = dict(kh=2, kw=2)

REFUSALS = [
    ("runet_transpose_taps", [("w", W), ("wt", Y), ("taps", 9), ("cin", 16), ("cout", 16), ("st", 0)],
     [(dict(w=0), "bad arguments"), (dict(wt=0), "bad arguments"), (dict(taps=0), "bad arguments"), (dict(cin=0), "bad arguments")]),
    ("runet_igemm_force_variant", [("v", -1)], [(dict(v=5), "variant: -1"), (dict(v=-2), "variant: -1")]),
    ("runet_igemm_lowp_force_variant", [("v", -1)], [(dict(v=3), "variant: -1"), (dict(v=-2), "variant: -1")]),
    ("runet_conv_igemm", _IG,
     [(dict(x=0), "null pointer"), (dict(w=0), "null pointer"), (dict(y=0), "null pointer"),
      (dict(cin=18, cin_w=18, ldx=20), "cin (channels read from x)"), (dict(cin_w=0), "cin_w (rows present"), (dict(cin_w=20), "cin_w (rows present"),
      (dict(cout=18), "cout must be"), (dict(ldx=12), "pixel strides"), (dict(ldy=18), "pixel strides"),
      (dict(x=ODD), "16-byte aligned"), (dict(w=W + 8), "16-byte aligned"), (dict(y=Y + 4), "16-byte aligned"),
      (dict(n=0), "empty iteration space"), (dict(kh=5, kw=5), "kernel must be"), (dict(kh=3, kw=1), "kernel must be"),
      (dict(_K2), "2x2 kernels are transposed-conv only"), (dict(ldy=12), "ldy < cout"),
      (dict(_K2, mode=DGRAD), "use RUNET_CONVT_DGRAD for 2x2"), (dict(mode=DGRAD, cin_w=12), "dgrad reads every output channel"),
      (dict(_K2, mode=DGRAD_T), "dgrad reads every output channel; use"), (dict(mode=DGRAD_T, cin_w=12), "dgrad reads every output channel; use"),
      (dict(mode=CONVT_DGRAD_T), "transposed conv is 2x2 stride 2"), (dict(_K2, mode=CONVT_DGRAD_T, cin_w=12), "transposed conv is 2x2 stride 2"),
      (dict(mode=CONVT_FWD, kh=3, kw=3), "transposed conv is 2x2 stride 2"), (dict(_K2, mode=CONVT_FWD, cin_w=12), "transposed conv is 2x2 stride 2"),
      (dict(mode=CONVT_DGRAD), "transposed conv is 2x2 stride 2"), (dict(mode=6), "unknown mode"), (dict(mode=-1), "unknown mode")]),
    ("runet_conv_wgrad", _WG,
     [(dict(x=0), "null pointer"), (dict(dy=0), "null pointer"), (dict(dw=0), "null pointer"),
      (dict(cin=18, ldx=20), "cin must be a multiple of 4"), (dict(cin_w=20), "cin must be a multiple of 4"), (dict(cout=18), "cout must be"),
      (dict(ldx=12), "bad pixel strides"), (dict(ldy=12), "bad pixel strides"), (dict(ldy=18), "bad pixel strides"),
      (dict(x=ODD), "16-byte aligned"), (dict(dw=DW + 8), "16-byte aligned"),
      (dict(_K2), "unsupported kernel size"), (dict(kh=5, kw=5), "unsupported kernel size"),
      (dict(kh=3, kw=3, cin=4, cin_w=3, ldx=4, ws=0), "workspace too small for the stem"), (dict(kh=3, kw=3, cin=4, cin_w=3, ldx=4, wsf=8), "workspace too small for the stem"),
      (dict(n=16, h=64, w_=64, cin=128, cin_w=128, cout=128, ldx=128, ldy=128, ws=0), "workspace too small (runet_conv_wgrad_workspace_floats)"),
      (dict(n=16, h=64, w_=64, cin=128, cin_w=128, cout=128, ldx=128, ldy=128, wsf=128 * 128), "workspace too small (runet_conv_wgrad_workspace_floats)")]),
    ("runet_conv2d_general", _GEN,
     [(dict(x=0), "null pointer"), (dict(y=0), "null pointer"), (dict(cin=18, cin_w=18), "channel counts"), (dict(cin_w=20), "channel counts"),
      (dict(cout=18), "channel counts"), (dict(kh=9), "unsupported geometry"), (dict(stride=0), "unsupported geometry"), (dict(stride=9), "unsupported geometry"),
      (dict(pad=-1), "unsupported geometry"), (dict(dil=0), "unsupported geometry"), (dict(ldx=18), "alignment"), (dict(w=W + 4), "alignment"),
      (dict(hin=1, pad=0), "empty output"), (dict(ldx=12), "bad pixel strides"), (dict(ldy=12), "bad pixel strides"),
      (dict(mode=DGRAD, kh=2, kw=2, stride=2, pad=0, cin_w=12), "bad arguments for the data gradient"),      # the live-tap form's line
      (dict(mode=DGRAD, cin_w=12), "bad arguments for the data gradient"), (dict(mode=DGRAD, ldy=12), "bad arguments for the data gradient"),
      (dict(mode=CONVT_FWD), "mode must be"), (dict(mode=DGRAD_T), "mode must be")]),
    ("runet_convt4_igemm", _T4,
     [(dict(x=0), "bad arguments"), (dict(w=0), "bad arguments"), (dict(cin=18), "bad arguments"), (dict(cout=0), "bad arguments"),
      (dict(ldx=18), "alignment"), (dict(y=Y + 4), "alignment"), (dict(mode=FWD), "mode must be"), (dict(mode=CONVT_DGRAD_T), "mode must be")]),
    ("runet_convt4_igemm_stats", _T4S,
     [(dict(x=0), "null pointer"), (dict(stats=0), "null pointer"), (dict(cin=18), "cin and cout"), (dict(cout=0), "cin and cout"),
      (dict(n=0), "bad shape"), (dict(ldx=12), "bad shape"), (dict(ldy=12), "bad shape"), (dict(ldx=18), "alignment"), (dict(w=W + 4), "alignment")]),
    ("runet_conv_wgrad_general", _WGG,
     [(dict(x=0), "null pointer"), (dict(dw=0), "null pointer"), (dict(cin=18), "channel counts / strides"), (dict(cin_w=0), "channel counts / strides"),
      (dict(cout=18), "channel counts / strides"), (dict(ldy=18), "channel counts / strides"), (dict(kh=9), "unsupported geometry"),
      (dict(stride=0), "unsupported geometry"), (dict(dil=0), "unsupported geometry"), (dict(tr4=1), "transposed4 is the k4-s2-p1")]),
    ("runet_conv2d_rect", _RECT,
     [(dict(x=0), "null pointer"), (dict(w=0), "null pointer"), (dict(cin=18, cin_w=18), "channel counts"), (dict(cout=0), "channel counts"),
      (dict(kw=9), "unsupported geometry"), (dict(pad_w=-1), "unsupported geometry"), (dict(dil_h=0), "unsupported geometry"), (dict(n=0), "empty shape"),
      (dict(win=0), "empty shape"), (dict(ldy=18), "alignment"), (dict(x=ODD), "alignment"), (dict(hin=1, pad_h=0), "empty output"),
      (dict(win=2, pad_w=0), "empty output"), (dict(ldx=12), "bad pixel strides"), (dict(ldy=12), "bad pixel strides"),
      (dict(mode=DGRAD, kh=2, kw=2, stride=2, pad_h=0, pad_w=0, cin_w=12), "bad arguments for the data gradient"),
      (dict(mode=DGRAD, cin_w=12), "bad arguments for the data gradient"), (dict(mode=DGRAD, ldx=12), "bad arguments for the data gradient"),
      (dict(mode=CONVT_FWD), "mode must be"), (dict(mode=-1), "mode must be")]),
    ("runet_convt3_pack", [("w", W), ("wq", Y), ("cin", 16), ("cout", 16), ("st", 0)],
     [(dict(w=0), "null pointer"), (dict(wq=0), "null pointer"), (dict(cin=18), "channel counts"), (dict(cout=0), "channel counts"),
      (dict(w=W + 4), "alignment"), (dict(wq=W), "wq must not be w")]),
    ("runet_convt3_fwd", _T3,
     [(dict(x=0), "null pointer"), (dict(wq=0), "null pointer"), (dict(cin=18), "channel counts"), (dict(cout=0), "channel counts"), (dict(h=0), "empty shape"),
      (dict(ldx=12), "bad pixel strides"), (dict(ldy=12), "bad pixel strides"), (dict(ldx=18), "alignment"), (dict(y=Y + 4), "alignment")]),
    ("runet_conv_wgrad_rect", _WGR,
     [(dict(x=0), "null pointer"), (dict(dy=0), "null pointer"), (dict(cin=18), "channel counts / strides"), (dict(cin_w=20), "channel counts / strides"),
      (dict(cout=0), "channel counts / strides"), (dict(ldx=18), "channel counts / strides"), (dict(ldx=12), "channel counts / strides"),
      (dict(ldy=12), "channel counts / strides"), (dict(kh=0), "unsupported geometry"), (dict(stride=9), "unsupported geometry"),
      (dict(pad_h=-1), "unsupported geometry"), (dict(dil_w=0), "unsupported geometry"), (dict(n=0), "empty shape"), (dict(hin=0), "empty shape"),
      (dict(x=ODD), "alignment"), (dict(dw=DW + 4), "alignment"), (dict(ws=WS + 8), "alignment"), (dict(hin=1, pad_h=0), "empty output"),
      (dict(win=2, pad_w=0), "empty output")]),
    ("runet_gemm_batched", _GB,
     [(dict(a=0), "bad arguments"), (dict(c=0), "bad arguments"), (dict(batch=0), "bad arguments"), (dict(batch=65536), "bad arguments"),
      (dict(rows=0), "bad arguments"), (dict(k=18, lda=20), "k, n and the row strides"), (dict(n=18, ldc=20), "k, n and the row strides"),
      (dict(lda=12), "k, n and the row strides"), (dict(ldc=18), "k, n and the row strides"), (dict(a=ODD), "alignment"), (dict(sb=254), "alignment"),
      (dict(sc=66), "alignment")]),
    ("runet_gemm_tn_batched", _GT,
     [(dict(a=0), "bad arguments (rows_per_split"), (dict(batch=65536), "bad arguments (rows_per_split"), (dict(rps=0), "bad arguments (rows_per_split"),
      (dict(rps=24), "bad arguments (rows_per_split"), (dict(rows=16 * 65536), "too many splits"), (dict(k=18, lda=20), "k, n and the row strides"),
      (dict(ldb=12), "k, n and the row strides"), (dict(b=W + 4), "alignment"), (dict(sa=66), "alignment")]),
]

# RUNET_REQUIRE lines without a call above, and why
SKIPPED = {
    "runet_conv_igemm: \"empty iteration space\" for h, w_": "the same condition as n = 0, one call per line",
    "runet_conv2d_general / runet_conv2d_rect: the second half of \"empty output\" (ho > 0 && wo > 0)":
        "ho <= 0 implies the first half of the condition where the entry point has one; the line is covered by hin = 1",
}


def refusals(mod):
    """-> [[function, overrides as text, return code, runet_last_error()]]; asserts that the call hit the RUNET_REQUIRE it was written for"""
    lib, out = mod.lib, []
    for fn, good, cases in REFUSALS:
        argtypes = mod.PROTOS[fn][1]
        assert len(argtypes) == len(good), fn
        for over, text in cases:
            assert set(over) <= {k for k, _ in good}, (fn, over)
            vals = [over.get(k, v) for k, v in good]
            args = [ctypes.c_void_p(v) if t is ctypes.c_void_p else v for t, v in zip(argtypes, vals)]
            lib.runet_set_error(b"")
            rc = getattr(lib, fn)(*args)
            msg = lib.runet_last_error().decode()
            assert rc == 1 and msg.startswith(fn + ": ") and text in msg, (fn, over, rc, msg)
            out.append([fn, json.dumps(over, sort_keys=True), rc, msg])
    return out


def main():
    if sys.argv[1:] == ["--child"]:
        print(json.dumps(collect(load().lib)))
        return
    mod = load()
    gold = {"library": "recorded from the parent of the commit that added this file; regenerate only against a library whose host decisions are the reference",
            "default": collect_child(None), "refusals": refusals(mod), "skipped": SKIPPED}
    for knob in KNOBS:
        gold[knob] = collect_child(knob)
    with open(GOLDEN, "w") as f:
        json.dump(gold, f, indent=0, sort_keys=True)
        f.write("\n")
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes;", len(gold["refusals"]), "refusals;", len(conv_name_cases()), "+", len(gemm_name_cases()), "names per setting")


if __name__ == "__main__":
    main()
