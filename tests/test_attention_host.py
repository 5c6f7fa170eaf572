"""CPU: the host-side decisions of csrc/attention.hip against tests/golden/attention_host.json, recorded by
tests/golden/make_golden_attention_host.py from the library as it was before its launchers were folded: the workspace sizes (the chunk plans
show in them) and the full runet_last_error() text - entry point, message, quoted condition - of refused calls for every reachable
RUNET_REQUIRE line of every entry point.  Nothing launches."""
import importlib.util
import json
import os

import pytest

from conftest import ROOT

_spec = importlib.util.spec_from_file_location("make_golden_attention_host", os.path.join(ROOT, "tests", "golden", "make_golden_attention_host.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

# The refusal calls pass made-up pointers: a check lost in a regression would launch on them, which only a machine without a GPU turns away.
no_gpu = pytest.mark.skipif(gen.gpu_visible(), reason="the refused calls pass made-up pointers: they run only where no GPU is visible")


@pytest.fixture(scope="module")
def gold():
    with open(gen.GOLDEN) as f:
        return json.load(f)


def test_workspace_sizes(gold):
    got, cases = gen.sizes(gen.load().lib), gen.ws_cases()
    assert sorted(got) == sorted(gold["workspaces"]) == sorted(cases)
    for fn, want in gold["workspaces"].items():
        assert len(want) == len(cases[fn]) and all(v > 0 for v in want), fn
        bad = [(c, a, b) for c, a, b in zip(cases[fn], got[fn], want) if a != b]
        assert not bad, (fn, len(bad), bad[:5])


def test_every_recorded_call_was_refused(gold):
    assert len(gold["refusals"]) == sum(len(c) for _, _, c in gen.REFUSALS)
    assert all(rc != 0 and msg.startswith(fn + ": ") for fn, _, rc, msg in gold["refusals"])
    assert {fn for fn, _, _ in gen.REFUSALS} == {w[0] for w in gold["refusals"]}


@no_gpu
def test_refusals_keep_function_message_and_condition(gold):
    got = gen.refusals(gen.load())
    assert len(got) == len(gold["refusals"])
    for g, w in zip(got, gold["refusals"]):
        assert g == w


@no_gpu
def test_rb_bwd1_asks_for_whole_images(gold):
    """the one refusal added since the recording, in the words of runet_rb_out's"""
    fn, over, like = gen.RB_BWD1_PIXELS
    want = next(msg for f, _, _, msg in gold["refusals"] if f == like and "whole number of images" in msg)
    assert gen.call(gen.load(), fn, over) == (1, want.replace(like + ": ", fn + ": ", 1))
