"""Writes tests/golden/ops_routes.json: what the convolution wrappers of ops.py hand to the C ABI, call by call, as one version of ops.py does
it.  Nothing launches and nothing reads tensor memory, so it runs without a GPU:

    python tests/golden/make_golden_ops_routes.py          (on the commit whose dispatch is the reference)

`ops.lib` is replaced by a proxy that forwards the host queries (names ending in HOST) to the real library and records every other entry
point as (name, arguments) - integers and floats as they are, pointers as "0" (null), "a" (16-byte aligned) or "u" - and answers 0.
`ops.stream` is a constant and torch.cuda.Event a dummy, so the profiled paths run as well.  The public functions are then called on
torch.empty CPU tensors over cases(); one record per case: the launches in order, the keys keep_v / keep_z / stats received, the profile
entries, the value of a predicate, or the exception.  Most knobs are read at import: every setting is collected in a child process.
The file holds every record's outline and digests of the full records (see "the file" below).

tests/test_ops_routes_host.py imports the grid and the collectors below, so the golden and the test cannot drift apart."""
import base64
import ctypes
import hashlib
import importlib
import json
import os
import subprocess
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "ops_routes.json")
PKG = "eusipco-2026-robust-unet_amd"

KNOBS = ("RUNET_NO_WINOGRAD", "RUNET_NO_WINOGRAD4", "RUNET_NO_WINOGRAD4_DILATED", "RUNET_NO_X3", "RUNET_NO_WINO_X3", "RUNET_NO_CONV_X3",
         "RUNET_NO_CONVT_X3_NARROW", "RUNET_NO_CONV1X1_STREAM", "RUNET_CONV1X1_WGRAD_STREAM", "RUNET_NO_STEM_KERNELS", "RUNET_NO_W4_ADJOINT",
         "RUNET_NO_FUSED_BN_INPUT", "RUNET_NO_EPILOGUE_STATS", "RUNET_TRANSPOSED_DGRAD")      # each collected alone, set to "1"
OTHER_KNOBS = ("RUNET_NO_CONV1X1_WGRAD_STREAM", "RUNET_WINO4_MIN_WIDE", "RUNET_WINO4_MIN_NARROW", "RUNET_WINO4_MAX_PIXELS", "RUNET_CONV_X3_MIN_K",
               "RUNET_CONV_X3_WIDE_N", "RUNET_HIP_LIB")      # cleared for the children: the grid assumes their defaults
HOST = ("_supported", "_fits", "_parts", "_elems", "_workspace_floats", "_rows_per_split", "_kernel_name")
STREAM = 0x5000
FWD, DGRAD, CONVT_FWD, CONVT_DGRAD = 0, 1, 2, 3

NS = (1, 2)
HW_N1 = ((128, 128), (16, 16), (6, 10))                        # a single image: at these sizes only
HW = ((128, 128), (64, 64), (32, 32), (16, 16), (8, 8), (6, 10), (7, 7))
CH = ((4, 3, 64), (8, 8, 8), (24, 24, 40), (64, 64, 64), (64, 64, 128), (128, 128, 64), (128, 128, 128), (256, 256, 128), (512, 512, 256),
      (512, 512, 512), (1024, 1024, 512))                      # (cin, cin_w, cout)
K_DIL = ((1, 1), (3, 1), (3, 2), (3, 4))
FORMS = ("dense", "wide", "off2")                               # the tensor itself / left half of a buffer twice as wide / the same from channel 2 on
MODES = (("f32", 0), ("f32", 1), ("bf16", 0), ("bf16", 1), ("fp16", 0), ("fp16", 1))      # (ops.precision, conv profile on)
MAX_ELEMS = 24 << 20                                             # n h w (cin + cout): keeps every tensor and workspace below 256 MB
# ops._wino_case on plain integers: (h, w, kh, dil, k, n, cin_w, n_img, ldx, ldy) around the fused F(2x2) kernel's 32-bit offset limit
WINO_INTS = ((512, 512, 3, 1, 64, 64, 64, 16, 64, 64), (512, 512, 3, 1, 64, 64, 64, 32, 64, 64), (512, 512, 3, 1, 64, 64, 64, 16, 128, 64),
             (512, 512, 3, 1, 64, 64, 64, 16, 64, 128), (512, 512, 3, 1, 64, 64, 64, 16, 127, 64), (1024, 1024, 3, 1, 32, 32, 32, 16, 0, 0),
             (1024, 1024, 3, 1, 32, 16, 32, 16, 0, 0), (16, 16, 3, 1, 4096, 2048, 4096, 1, 0, 0), (16, 16, 3, 1, 4096, 4096, 4096, 1, 0, 0),
             (16, 16, 3, 2, 64, 64, 64, 1, 0, 0), (16, 16, 1, 1, 64, 64, 64, 1, 0, 0), (16, 16, 3, 1, 64, 64, 48, 1, 0, 0), (15, 16, 3, 1, 64, 64, 64, 1, 0, 0))


# ------------------------------------------------------------------------------------------------ the grid
def _shapes(convt=False):
    for n in NS:
        for h, w in HW if n > 1 else HW_N1:
            for cin, cin_w, cout in CH:
                if n * h * w * (cin + (8 if convt else 1) * cout) <= MAX_ELEMS and not (convt and cin_w != cin):
                    yield n, h, w, cin, cin_w, cout


def cases():
    """-> [(function, n, h, w, cin, cin_w, cout, k, dil, source form, second form / destination, accumulate, feature, precision, profile)]"""
    out = []

    def add(fn, shape, k=1, dil=1, src="dense", dst="", acc=0, feat="", mode=MODES[0]):
        out.append((fn,) + tuple(shape) + (k, dil, src, dst, acc, feat) + tuple(mode))

    for shape in _shapes():
        stem = shape[3] != shape[4]
        for k, dil in K_DIL:
            for src in FORMS:                                    # layouts, f32, no profile
                for dst in ("", "slice"):
                    for acc in (0, 1):
                        add("conv_fwd", shape, k, dil, src, dst, acc)
                        if not stem:
                            add("conv_dgrad", shape, k, dil, src, dst, acc)
            for src, dst in (("dense", "dense"), ("wide", "wide"), ("off2", "dense"), ("dense", "off2")):
                for feat in ("", "out"):
                    add("conv_wgrad", shape, k, dil, src, dst, feat=feat)
            for feat in ("stats", "keep_v", "keep_v+stats", "pre", "pre+fac+keep_v+stats"):
                add("conv_fwd", shape, k, dil, feat=feat)
            for feat in ("v", "z", "v+z+out"):
                add("conv_wgrad", shape, k, dil, feat=feat)
            if not stem:
                for feat in ("keep_z", "bn", "bn+mask", "bn+nokeep"):
                    add("conv_dgrad", shape, k, dil, feat=feat)
            for mode in MODES[1:]:
                for src, dst, acc in (("dense", "", 0), ("wide", "slice", 1)):
                    add("conv_fwd", shape, k, dil, src, dst, acc, mode=mode)
                    if not stem:
                        add("conv_dgrad", shape, k, dil, src, dst, acc, mode=mode)
                add("conv_fwd", shape, k, dil, feat="keep_v+stats", mode=mode)
                add("conv_wgrad", shape, k, dil, mode=mode)
                add("conv_wgrad", shape, k, dil, feat="v+z+out", mode=mode)
                if not stem:
                    add("conv_dgrad", shape, k, dil, feat="keep_z", mode=mode)
        for k in (1, 3):
            add("fuses_act_input", shape, k)
            if not stem:
                add("fuses_bn_bwd_input", shape, k)
    for shape in _shapes(convt=True):
        for mode in MODES:
            for src in FORMS if mode == MODES[0] else FORMS[:2]:
                for dst in ("", "slice"):
                    add("convt_fwd", shape, 2, 1, src, dst, mode=mode)
                    for acc in (0, 1):
                        add("convt_dgrad", shape, 2, 1, src, dst, acc, mode=mode)
            for src, feat in (("dense", ""), ("wide", "out")):
                add("convt_wgrad", shape, 2, 1, src, src, feat=feat, mode=mode)
    for n in NS:
        for h, w in HW if n > 1 else HW_N1:
            for cout in (32, 64):
                for feat in ("", "w1", "stats3", "w1+stats3", "w1+stats3+stats1"):
                    add("stem_conv", (n, h, w, 4, 3, cout), 3, feat=feat)
    for c in WINO_INTS:
        out.append(("_wino_case",) + c)
    return out


# ------------------------------------------------------------------------------------------------ the recording proxy
class Recorder:
    def __init__(self, real, protos):
        self._real, self._protos, self.calls = real, protos, []

    def __getattr__(self, name):
        real = getattr(self._real, name)
        if name.endswith(HOST):
            return real
        types = self._protos[name][1]

        def record(*args):
            assert len(args) == len(types), (name, len(args), len(types))
            self.calls.append([name] + [_enc(a, t in (ctypes.c_void_p, ctypes.c_char_p)) for a, t in zip(args, types)])
            return 0
        return record


def _enc(a, pointer):
    if pointer:
        return "0" if not a else ("a" if a % 16 == 0 else "u")
    assert isinstance(a, (int, float)), a
    return int(a) if isinstance(a, bool) else a


class Event:
    def __init__(self, **kw):
        pass

    def record(self, *a):
        pass


def load_ops():
    """ops.py of the working tree with the library, the stream getter and the HIP events replaced (this process only: use a child)"""
    import torch
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    ops, lm = importlib.import_module(PKG + ".ops"), importlib.import_module(PKG + "._lib")
    ops.lib = Recorder(lm.lib, lm.PROTOS)
    ops.stream = lambda: STREAM
    torch.cuda.Event = Event
    return ops


# ------------------------------------------------------------------------------------------------ one case
def _nhwc(torch, n, h, w, c, form):
    if form == "dense":
        return torch.empty((n, h, w, c))
    buf = torch.empty((n, h, w, 2 * c))
    return buf[..., :c] if form == "wide" else (buf[..., c:] if form == "slice" else buf[..., 2:2 + c])


def launched_route(fn, calls):
    """the route a record's (or an outline's) launches show, under the names of ops.conv_route / wgrad_route / convt_route"""
    names = {c if isinstance(c, str) else c[0] for c in calls}
    if fn in ("conv_wgrad", "convt_wgrad"):
        table = (("lowp", ("runet_conv_wgrad_bf16", "runet_conv_wgrad_fp16")), ("wino4", ("runet_wino4_wgrad", "runet_wino4_wgrad_output")),
                 ("stem", ("runet_stem_wgrad",)), ("wino2", ("runet_wino_wgrad",)), ("stream1x1", ("runet_conv1x1_wgrad_stream",)),
                 ("igemm", ("runet_conv_wgrad",)))
    else:
        table = (("lowp", ("runet_conv_igemm_bf16", "runet_conv_igemm_fp16")), ("wino4_adj", ("runet_wino4_output_adj",)),
                 ("wino4", ("runet_wino4_conv", "runet_wino4_conv_x3", "runet_wino4_output", "runet_wino4_output_stats")),
                 ("wino2", ("runet_wino_conv", "runet_wino_conv_x3", "runet_wino_conv_x3_stats")), ("x3", ("runet_conv_x3", "runet_conv_x3_stats")),
                 ("stream1x1", ("runet_conv1x1_stream",)), ("igemm", ("runet_conv_igemm",)))
    hit = [route for route, fns in table if names & set(fns)]
    assert len(hit) == 1, (fn, sorted(names))
    return hit[0]


def run_case(ops, case):
    """-> the record of one case, a dict with the non-empty ones of: c launches, k keys received, p profile entries, r value, e exception"""
    import torch
    if case[0] == "_wino_case":
        return {"r": bool(ops._wino_case(*case[1:]))}
    fn, n, h, w, cin, cin_w, cout, k, dil, src, dst, acc, feat, prec, prof = case
    feats = set(feat.split("+")) if feat else set()
    E = torch.empty
    ops._derived.clear()
    ops.lib.calls = []
    got = {name: {} for name in ("keep_v", "keep_z", "stats", "stats3", "stats1") if name in feats}
    wt = E((k, k, cin_w, cout))
    bias = None if acc else E(cout)
    t = n * (h // 4) * (w // 4)
    route = None                                                  # (route function, its arguments) where the case has one
    if fn == "conv_fwd":
        x, out = _nhwc(torch, n, h, w, cin, src), _nhwc(torch, n, h, w, cout, dst) if dst else None
        kw = {}
        if "pre" in feats:
            kw["pre"] = (E(cin), E(cin), E(n * cin) if "fac" in feats else None)
        call = lambda: ops.conv_fwd(x, wt, bias, out=out, dil=dil, accumulate=bool(acc), keep_v=got.get("keep_v"), stats=got.get("stats"), **kw)
        route = ("conv_route", (FWD, x, wt, out, dil))
    elif fn == "conv_dgrad":
        dy, out = _nhwc(torch, n, h, w, cout, src), _nhwc(torch, n, h, w, cin, dst) if dst else None
        kw = {}
        if "bn" in feats:
            kw["bn"] = dict(x=E((n, h, w, cout)), mean=E(cout), invstd=E(cout), scale=E(cout), shift=E(cout), sums=E(2 * cout), m_total=n * h * w,
                            mask=E(n * cout) if "mask" in feats else None)
            if "nokeep" not in feats:
                got["keep_z"] = {}
        call = lambda: ops.conv_dgrad(dy, wt, out=out, dil=dil, accumulate=bool(acc), keep_z=got.get("keep_z"), **kw)
        route = ("conv_route", (DGRAD, dy, wt, out, dil))
    elif fn == "conv_wgrad":
        x, dy = _nhwc(torch, n, h, w, cin, src), _nhwc(torch, n, h, w, cout, dst)
        out = E((k, k, cin_w, cout)) if "out" in feats else None
        v, z = E(36 * t * cin) if "v" in feats else None, E(36 * t * cout) if "z" in feats else None
        call = lambda: ops.conv_wgrad(x, dy, k, k, cin_w=cin_w, dil=dil, out=out, v=v, z=z)
        route = ("wgrad_route", (x, dy, k, k, cin_w, dil, out if out is not None else E((k, k, cin_w, cout))))
    elif fn == "convt_fwd":
        x, out = _nhwc(torch, n, h, w, cin, src), _nhwc(torch, n, 2 * h, 2 * w, cout, dst) if dst else None
        call = lambda: ops.convt_fwd(x, wt, bias, out=out)
        route = ("convt_route", (CONVT_FWD, x, wt))
    elif fn == "convt_dgrad":
        dy, out = _nhwc(torch, n, 2 * h, 2 * w, cout, src), _nhwc(torch, n, h, w, cin, dst) if dst else None
        call = lambda: ops.convt_dgrad(dy, wt, out=out, accumulate=bool(acc))
        route = ("convt_route", (CONVT_DGRAD, dy, wt))
    elif fn == "convt_wgrad":
        x, dy = _nhwc(torch, n, h, w, cin, src), _nhwc(torch, n, 2 * h, 2 * w, cout, dst)
        call = lambda: ops.convt_wgrad(x, dy, out=E((2, 2, cin, cout)) if "out" in feats else None)
    elif fn == "stem_conv":
        x = E((n, h, w, 4))
        call = lambda: ops.stem_conv(x, wt, E((1, 1, cin_w, cout)) if "w1" in feats else None, got.get("stats3"), got.get("stats1"))
    else:
        x = E((n, h, w, cin if fn == "fuses_act_input" else cout))
        call = lambda: bool(getattr(ops, fn)(x, wt))
    rec = {}
    with ops.precision(prec):
        if prof:
            ops.start_conv_profile()
        try:
            r = call()
            if isinstance(r, bool):
                rec["r"] = r
        except AssertionError:
            rec["e"] = "AssertionError"
        finally:
            entries, ops._PROFILE = ops._PROFILE, None
        if ops.lib.calls:
            rec["c"] = ops.lib.calls
        keys = {name: sorted(d) for name, d in got.items() if d}
        if keys:
            rec["k"] = keys
        if entries:
            rec["p"] = [[e[0], e[1], e[2], e[5] if len(e) > 5 else None] for e in entries]
        if route is not None and "e" not in rec and hasattr(ops, route[0]):
            # a tree that has the route functions: they must name the kernels that were launched
            assert getattr(ops, route[0])(*route[1]) == launched_route(fn, rec["c"]), (case, getattr(ops, route[0])(*route[1]), rec["c"])
    return rec


def collect(ops):
    return [json.dumps(run_case(ops, c), sort_keys=True, separators=(",", ":")) for c in cases()]


def collect_child(knob):
    """collect() in a fresh process with one knob set to 1 (None: with all of them unset) -> the records, as JSON text each"""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS + OTHER_KNOBS}
    if knob:
        env[knob] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return unpack(r.stdout.strip().splitlines()[-1])


# ------------------------------------------------------------------------------------------------ the file
# Full records of every setting would take megabytes.  The file keeps, per setting, (1) the outline of every record - the names of the
# launches in order, the keys received, the profile's kernel names, the value or exception: few distinct ones, stored as a shared table plus
# one index per case - and (2) a digest of the full records (every argument, FLOP and byte count) per CHUNK consecutive cases.
CHUNK, DIGEST = 32, 4


def pack(obj):
    return base64.b64encode(zlib.compress(json.dumps(obj, separators=(",", ":")).encode(), 9)).decode("ascii")


def unpack(text):
    return json.loads(zlib.decompress(base64.b64decode(text)))


def outline(record):
    r = json.loads(record)
    for key in ("c", "p"):
        if key in r:
            r[key] = [entry[0] for entry in r[key]]
    return json.dumps(r, sort_keys=True, separators=(",", ":"))


def digests(records):
    return [hashlib.blake2b("\n".join(records[i:i + CHUNK]).encode(), digest_size=DIGEST).hexdigest() for i in range(0, len(records), CHUNK)]


def _b64(raw):
    return base64.b64encode(zlib.compress(raw, 9)).decode("ascii")


def encode(settings):
    """{setting: records} -> the file's content; the settings other than "default" are stored as differences from it"""
    table = sorted({outline(r) for recs in settings.values() for r in recs})
    pos = {o: i for i, o in enumerate(table)}
    assert len(table) < 65536
    idx = {k: [pos[outline(r)] for r in recs] for k, recs in settings.items()}
    dig = {k: bytes.fromhex("".join(digests(recs))) for k, recs in settings.items()}
    out = {"cases": len(settings["default"]), "chunk": CHUNK, "table": table}
    for k in settings:
        i = [(a - b) % 65536 for a, b in zip(idx[k], idx["default"])] if k != "default" else idx[k]
        d = bytes(a ^ b for a, b in zip(dig[k], dig["default"])) if k != "default" else dig[k]
        out[k] = {"outline": _b64(b"".join(v.to_bytes(2, "little") for v in i)), "digest": _b64(d)}
    return out


def decode(gold):
    """-> {setting: (outlines, one per case; digests, one per CHUNK cases)}"""
    def raw(k, part):
        return zlib.decompress(base64.b64decode(gold[k][part]))
    out = {}
    for k in ["default"] + [k for k in gold if isinstance(gold[k], dict) and k != "default"]:
        o, d = raw(k, "outline"), raw(k, "digest")
        i = [int.from_bytes(o[j:j + 2], "little") for j in range(0, 2 * gold["cases"], 2)]
        if k != "default":
            i = [(a + b) % 65536 for a, b in zip(i, base_i)]
            d = bytes(a ^ b for a, b in zip(d, base_d))
        else:
            base_i, base_d = i, d
        out[k] = ([gold["table"][j] for j in i], [d[j:j + DIGEST].hex() for j in range(0, len(d), DIGEST)])
    return out


def main():
    if sys.argv[1:] == ["--child"]:
        print(pack(collect(load_ops())))
        return
    settings = {"default": collect_child(None)}
    for knob in KNOBS:
        settings[knob] = collect_child(knob)
        print(knob, sum(a != b for a, b in zip(settings[knob], settings["default"])), "records differ")
    gold = encode(settings)
    gold["source"] = "recorded from ops.py as it was in the parent of the commit that added this file; regenerate only from a dispatch that is the reference"
    with open(GOLDEN, "w") as f:
        json.dump(gold, f, indent=0, sort_keys=True)
        f.write("\n")
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes;", gold["cases"], "cases per setting;", len(gold["table"]), "outlines")


if __name__ == "__main__":
    main()
