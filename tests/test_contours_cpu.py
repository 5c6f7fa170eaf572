"""CPU: the parallel border-following formulation behind the device contour tracer (contours_ref.py) against the host tracer on every mask
the GPU test runs, and the C ABI of the new entry points with their host-side validation."""
import ctypes
import importlib
import os

import numpy as np
import pytest

import contours_ref as CR
from conftest import ROOT

ENTRIES = ("runet_contours_workspace_bytes", "runet_contours_state_workspace_bytes", "runet_contours_count", "runet_contours_trace")
P16 = ctypes.c_void_p(4096)          # a non-null, 16-byte aligned "pointer": validation must fail before anything would touch it
CASES = CR.cases()


def _predict():
    return importlib.import_module("eusipco-2026-robust-unet_amd.predict")


def _lib():
    return importlib.import_module("eusipco-2026-robust-unet_amd._lib")


def _same(got, want):
    return len(got) == len(want) and all(a.dtype == np.int32 and a.shape == b.shape and np.array_equal(a, b) for a, b in zip(got, want))


def test_case_list_covers_what_it_names():
    names = [n for n, _ in CASES]
    assert len(set(names)) == len(names)
    by = dict(CASES)
    P = _predict()
    assert len(P.trace_external_contours(by["all_ones"])) == 1 and len(P.trace_external_contours(by["all_ones"])[0]) == 4
    assert len(P.trace_external_contours(by["squares_touching_at_a_corner"])) == 1
    assert len(P.trace_external_contours(by["diagonal_ring_with_dot"])) == 1
    assert len(P.trace_external_contours(by["dot_in_ring_in_ring"])) == 1
    assert len(P.trace_external_contours(by["two_rings_with_islands"])) == 2
    assert len(P.trace_external_contours(by["hole_and_frame_bay"])) == 3
    assert len(P.trace_external_contours(by["spiral_64"])) == 1 and len(P.trace_external_contours(by["serpentine_128"])) == 1
    assert CR.successor_map(by["serpentine_128"])["succ"].size > 16384
    assert by["values_2_and_255"].max() == 255 and 2 in by["values_2_and_255"]
    assert len(P.trace_external_contours(by["coastline_band_256"])) >= 3


@pytest.mark.parametrize("name,mask", CASES, ids=[n for n, _ in CASES])
def test_formulation_equals_the_host_tracer(name, mask):
    want = _predict().trace_external_contours(mask)
    assert _same(CR.trace(mask), want)
    assert _same(CR.trace(mask, 10), [c for c in want if len(c) > 10])


@pytest.mark.parametrize("name,mask", CASES, ids=[n for n, _ in CASES])
def test_successor_map_is_a_bijection_on_the_valid_states(name, mask):
    sm = CR.successor_map(mask, candidates_only=False)
    n = sm["succ"].size
    assert np.array_equal(np.sort(sm["succ"]), np.arange(n))
    # on the candidate pixels alone: a state is its own successor or maps to a state of its successor pixel that points back at it
    cm = CR.successor_map(mask)
    moved = np.flatnonzero(cm["succ"] != np.arange(cm["succ"].size))
    w = mask.shape[1]
    q = cm["spix"][cm["succ"][moved]]
    back = cm["sdir"][cm["succ"][moved]]
    assert np.array_equal(q + np.array(CR.DI)[back] * w + np.array(CR.DJ)[back], cm["spix"][moved])
    assert np.unique(cm["succ"][moved]).size == moved.size


def test_new_entry_points_are_declared_exported_and_cite_the_reference():
    lm = _lib()
    protos = lm.parse_header(os.path.join(ROOT, "include", "runet_hip.h"))
    raw = ctypes.CDLL(lm.LIB_PATH)
    for name in ENTRIES:
        assert name in protos, f"{name} not declared in include/runet_hip.h"
        assert hasattr(raw, name), f"{name} not exported by librunet_hip.so"
    assert len(protos["runet_contours_count"][1]) == 7 and len(protos["runet_contours_trace"][1]) == 9
    assert "predict_coastline.py:605-608" in open(os.path.join(ROOT, "include", "runet_hip.h")).read()
    pkg = importlib.import_module("eusipco-2026-robust-unet_amd")
    assert "trace_external_contours_device" in pkg.__all__
    assert pkg.trace_external_contours_device is _predict().trace_external_contours_device


def test_workspace_sizes():
    lib = _lib().lib
    assert lib.runet_contours_workspace_bytes(0, 5) == -1 and lib.runet_contours_workspace_bytes(5, -1) == -1
    assert lib.runet_contours_workspace_bytes(65536, 32768) == -1                      # h * w = 2^31
    a, b = lib.runet_contours_workspace_bytes(512, 512), lib.runet_contours_workspace_bytes(2048, 2048)
    assert a >= 512 * 512 * 10 and 15 * a < b < 17 * a
    assert lib.runet_contours_state_workspace_bytes(0) == -1 and lib.runet_contours_state_workspace_bytes(1 << 31) == -1
    s = lib.runet_contours_state_workspace_bytes(1000)
    assert s >= 1000 * 4 * 15 and lib.runet_contours_state_workspace_bytes(100000) > 50 * s


def test_host_side_validation_without_a_gpu():
    lib = _lib().lib
    err = lib.runet_last_error
    big = 1 << 40
    assert lib.runet_contours_count(None, 8, 8, P16, big, P16, None) != 0 and b"null pointer" in err()
    assert lib.runet_contours_count(P16, 8, 8, None, big, P16, None) != 0 and b"null pointer" in err()
    assert lib.runet_contours_count(P16, 8, 8, P16, big, None, None) != 0 and b"null pointer" in err()
    assert lib.runet_contours_count(P16, 0, 8, P16, big, P16, None) != 0 and b"bad shape" in err()
    assert lib.runet_contours_count(P16, 8, 8, ctypes.c_void_p(4104), big, P16, None) != 0 and b"aligned" in err()
    assert lib.runet_contours_count(P16, 8, 8, P16, big, ctypes.c_void_p(4100), None) != 0 and b"aligned" in err()
    assert lib.runet_contours_count(P16, 65536, 32768, P16, big, P16, None) != 0 and b"2^31" in err()
    need = lib.runet_contours_workspace_bytes(8, 8)
    assert lib.runet_contours_count(P16, 8, 8, P16, need - 1, P16, None) != 0 and b"workspace too small" in err()

    sneed = lib.runet_contours_state_workspace_bytes(20)
    assert lib.runet_contours_trace(8, 8, None, need, 20, 0, P16, sneed, None) != 0 and b"null pointer" in err()
    assert lib.runet_contours_trace(8, 8, P16, need, 20, 0, None, sneed, None) != 0 and b"null pointer" in err()
    assert lib.runet_contours_trace(8, 8, P16, need, 20, 0, ctypes.c_void_p(4104), sneed, None) != 0 and b"aligned" in err()
    assert lib.runet_contours_trace(65536, 32768, P16, big, 20, 0, P16, big, None) != 0 and b"2^31" in err()
    assert lib.runet_contours_trace(32768, 32768, P16, big, 1 << 31, 0, P16, big, None) != 0 and b"does not fit int32" in err()
    assert lib.runet_contours_trace(8, 8, P16, need, 0, 0, P16, sneed, None) != 0 and b"state count" in err()
    assert lib.runet_contours_trace(8, 8, P16, need, 20, -1, P16, sneed, None) != 0 and b"min_points" in err()
    assert lib.runet_contours_trace(8, 8, P16, need, 8 * 64 + 1, 0, P16, big, None) != 0 and b"8 per pixel" in err()
    assert lib.runet_contours_trace(8, 8, P16, need - 1, 20, 0, P16, sneed, None) != 0 and b"workspace too small" in err()
    assert lib.runet_contours_trace(8, 8, P16, need, 20, 0, P16, sneed - 1, None) != 0 and b"state workspace too small" in err()
    P = _predict()
    with pytest.raises(ValueError):
        P.trace_external_contours_device(np.zeros((4, 4), np.uint8))                  # a host array: the host tracer is the function for it
