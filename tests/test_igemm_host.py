"""CPU: the host-side decisions of csrc/conv_igemm.hip against tests/golden/igemm_host.json, recorded by tests/golden/make_golden_igemm_host.py
from the library as it was before the launchers were restructured: which kernel a shape takes (runet_conv_igemm_kernel_name at automatic
selection and with each tile variant forced, runet_gemm_batched_kernel_name), the workspace sizes, the statistics parts, and the full
runet_last_error() text of one refused call per RUNET_REQUIRE line of every entry point.  Nothing launches."""
import importlib.util
import json
import os

import pytest

from conftest import ROOT

_spec = importlib.util.spec_from_file_location("make_golden_igemm_host", os.path.join(ROOT, "tests", "golden", "make_golden_igemm_host.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

GRIDS = {"conv_names": gen.conv_name_cases, "gemm_names": gen.gemm_name_cases, "wgrad": gen.wgrad_ws_cases,
         "general": lambda: [c for c in gen.pixel_ws_cases() if c not in gen.WS_BAD], "rect": gen.pixel_ws_cases, "parts": gen.parts_cases}


@pytest.fixture(scope="module")
def gold():
    with open(gen.GOLDEN) as f:
        return json.load(f)


def _compare(got, want):
    assert sorted(got) == sorted(want) == sorted(GRIDS)
    for key, cases in GRIDS.items():
        g, w, cases = gen.unpack(got[key]), gen.unpack(want[key]), cases()
        assert len(g) == len(w) == len(cases), key
        bad = [(c, a, b) for c, a, b in zip(cases, g, w) if a != b]
        assert not bad, (key, len(bad), bad[:5])


@pytest.mark.parametrize("knob", (None,) + gen.KNOBS)
def test_names_workspaces_and_parts(gold, knob):
    """a fresh process per setting: the library reads each knob once"""
    _compare(gen.collect_child(knob), gold[knob or "default"])


def test_the_grids_reach_every_name(gold):
    names = set(gold["default"]["conv_names"]["table"]) | set(gold["RUNET_IGEMM_GENERAL"]["conv_names"]["table"])
    assert len(names) == 20 and all(n.startswith("igemm_kernel<") for n in names)            # 5 tiles x 2 weight layouts x 2 loaders
    assert any(n.startswith("gemm_nn_kernel<") for n in gold["default"]["gemm_names"]["table"])
    assert -1 in gold["default"]["rect"]["table"]


def test_refusals_keep_function_message_and_condition(gold):
    got = gen.refusals(gen.load())
    assert len(got) == len(gold["refusals"]) == sum(len(c) for _, _, c in gen.REFUSALS)
    for g, w in zip(got, gold["refusals"]):
        assert g == w
    assert {fn for fn, _, _ in gen.REFUSALS} == {w[0] for w in gold["refusals"]}
