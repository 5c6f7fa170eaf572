"""CPU: what ops.py's convolution wrappers hand to the C ABI, call by call, against tests/golden/ops_routes.json, recorded by
tests/golden/make_golden_ops_routes.py from ops.py as it was before its dispatch was gathered into conv_route / wgrad_route / convt_route:
the launches in order with every integer argument, null / aligned / unaligned pointers, the keys keep_v / keep_z / stats receive, the conv
profile's (name, flops, executed flops, bytes), under the default settings, each dispatch knob alone, and ops.precision.  Nothing launches.
The golden holds the outline of every record (launch names in order, keys, profile names, value or exception), compared case by case, and a
digest of the full records per gen.CHUNK consecutive cases, compared chunk by chunk.
In a tree that has the route functions the generator also asserts, case by case, that they name the kernel that was launched."""
import concurrent.futures
import importlib.util
import json
import os

import pytest

from conftest import ROOT

_spec = importlib.util.spec_from_file_location("make_golden_ops_routes", os.path.join(ROOT, "tests", "golden", "make_golden_ops_routes.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

CASES = gen.cases()
CONV, WGRAD, CONVT = ("conv_fwd", "conv_dgrad"), ("conv_wgrad",), ("convt_fwd", "convt_dgrad")
ROUTES = {CONV: {"lowp", "wino4", "wino4_adj", "wino2", "x3", "stream1x1", "igemm"}, WGRAD: {"lowp", "wino4", "stem", "wino2", "stream1x1", "igemm"},
          CONVT: {"lowp", "x3", "igemm"}}


@pytest.fixture(scope="module")
def gold():
    """{setting: (outlines, digests)}, the default setting under the key None"""
    with open(gen.GOLDEN) as f:
        g = json.load(f)
    assert g["cases"] == len(CASES) and g["chunk"] == gen.CHUNK
    out = gen.decode(g)
    out[None] = out.pop("default")
    assert sorted(k for k in out if k) == sorted(gen.KNOBS)
    return out


@pytest.fixture(scope="module")
def traces():
    """a fresh process per setting (most knobs are read at import), a few at a time"""
    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as pool:
        yield {knob: pool.submit(gen.collect_child, knob) for knob in (None,) + gen.KNOBS}


@pytest.mark.parametrize("knob", (None,) + gen.KNOBS)
def test_launch_trace_is_the_recorded_one(gold, traces, knob):
    got, (want, want_digests) = traces[knob].result(), gold[knob]
    assert len(got) == len(want) == len(CASES)
    bad = [(c, g, w) for c, g, w in zip(CASES, got, want) if gen.outline(g) != w]
    assert not bad, (knob, len(bad), bad[:3])
    bad = [i for i, (g, w) in enumerate(zip(gen.digests(got), want_digests)) if g != w]      # an argument, a pointer class or a FLOP count moved
    assert not bad, (knob, len(bad), [(c, g) for c, g in zip(CASES, got)][bad[0] * gen.CHUNK:(bad[0] + 1) * gen.CHUNK])


def _routes(records, fns, lowp=None, dilated=None):
    """the routes the launches of `records` show for the cases of functions `fns` (lowp / dilated: only such cases, or only the others)"""
    seen = set()
    for c, r in zip(CASES, records):
        rec = json.loads(r)
        if c[0] in fns and "c" in rec and lowp in (None, c[13] != "f32") and dilated in (None, c[8] > 1):
            seen.add(gen.launched_route(c[0], rec["c"]))
    return seen


def test_the_golden_reaches_every_route_and_every_knob(gold):
    """the conditions the recorded grid must meet, asserted on the golden itself so that a thin grid cannot pass silently"""
    base = gold[None][0]
    for fns, names in ROUTES.items():
        # "lowp" needs ops.precision; the streaming weight gradient is off by default (RUNET_CONV1X1_WGRAD_STREAM=1 turns it on at import)
        want = names - {"lowp"} - ({"stream1x1"} if fns == WGRAD else set())
        assert _routes(base, fns, lowp=False) == want, fns
        assert "lowp" in _routes(base, fns, lowp=True), fns
    assert "stream1x1" in _routes(gold["RUNET_CONV1X1_WGRAD_STREAM"][0], WGRAD, lowp=False)
    for knob in gen.KNOBS:
        assert gold[knob][1] != gold[None][1], knob
    for fn in ("fuses_act_input", "fuses_bn_bwd_input"):
        assert {json.loads(r)["r"] for c, r in zip(CASES, base) if c[0] == fn} == {True, False}, fn
    assert {"wino4", "wino4_adj"} <= _routes(base, CONV, lowp=False, dilated=True)
    # a 3x3, dilation 1 convolution with every weight row present that the fused F(2x2) kernel refuses (odd size, narrow) -> implicit GEMM
    assert any(c[0] == "conv_fwd" and (c[7], c[8], c[13]) == (3, 1, "f32") and c[4] == c[5] and gen.launched_route(c[0], json.loads(r)["c"]) == "igemm"
               for c, r in zip(CASES, base))
    fits = [json.loads(r)["r"] for c, r in zip(CASES, base) if c[0] == "_wino_case"]
    assert fits[0] is True and fits[1] is False and len(fits) == len(gen.WINO_INTS)      # 16 x 512^2 x 64 fits the 32-bit offsets, 32 images do not


def test_fused_inputs_are_legal_exactly_where_the_predicates_say(traces):
    """conv_fwd(pre=...) / conv_dgrad(bn=...) launch the fused input transform wherever fuses_act_input / fuses_bn_bwd_input answer yes
    (at dilation 1, and for bn with keep_z), and raise AssertionError everywhere else: the predicates cannot disagree with the dispatch"""
    recs = [json.loads(r) for r in traces[None].result()]
    says = {(c[0],) + c[1:8]: r["r"] for c, r in zip(CASES, recs) if c[0].startswith("fuses_")}
    seen = {("pre", True): 0, ("pre", False): 0, ("bn", True): 0, ("bn", False): 0}
    for c, r in zip(CASES, recs):
        feats = set(c[12].split("+")) if len(c) > 12 and isinstance(c[12], str) else set()
        kind = "pre" if (c[0] == "conv_fwd" and "pre" in feats) else "bn" if (c[0] == "conv_dgrad" and "bn" in feats) else None
        if kind is None:
            continue
        legal = says[("fuses_act_input" if kind == "pre" else "fuses_bn_bwd_input",) + c[1:8]] and c[8] == 1 and "nokeep" not in feats
        seen[(kind, legal)] += 1
        if legal:
            want = "runet_wino4_input_act" if kind == "pre" else "runet_wino4_input_bn_bwd"
            assert "e" not in r and want in [call[0] for call in r["c"]], (c, r)
            assert gen.launched_route(c[0], r["c"]) == ("wino4" if kind == "pre" else "wino4_adj")
        else:
            assert r.get("e") == "AssertionError" and "c" not in r, (c, r)
    assert all(seen.values()), seen
