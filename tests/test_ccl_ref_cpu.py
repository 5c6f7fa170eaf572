"""CPU: the numpy restatement of connected-component labelling (components.label_components_host) against the flood fill and scipy, and
the named mistakes against the cases.  No tolerance anywhere: labels, areas and boxes are integers."""
import importlib

import numpy as np
import pytest

import ccl_ref as R


def _components():
    return importlib.import_module("eusipco-2026-robust-unet_amd.components")


def test_host_restatement_equals_the_flood_fill():
    C = _components()
    for name, m, connectivity, invert in R.cases():
        got = C.label_components_host(m, connectivity=connectivity, invert=invert)
        assert got.dtype == np.int32 and got.shape == m.shape and np.array_equal(got, R.truth(name, m, connectivity, invert)), name
    batch = R.batch()
    got = C.label_components_host(batch, connectivity=4)
    assert got.shape == batch.shape and all(np.array_equal(got[i], R.flood_labels(batch[i], 4)) for i in range(3))
    assert np.array_equal(C.label_components_host(batch != 0, connectivity=4), got)
    with pytest.raises(ValueError):
        C.label_components_host(batch, connectivity=6)


def test_the_definition_on_hand_checked_masks():
    m = np.array([[1, 0, 0, 1],
                  [0, 1, 0, 1],
                  [0, 0, 0, 0],
                  [1, 1, 0, 1]], np.uint8)
    assert np.array_equal(R.flood_labels(m, 8), [[1, 0, 0, 4], [0, 1, 0, 4], [0, 0, 0, 0], [13, 13, 0, 16]])
    assert np.array_equal(R.flood_labels(m, 4), [[1, 0, 0, 4], [0, 6, 0, 4], [0, 0, 0, 0], [13, 13, 0, 16]])
    assert np.array_equal(R.flood_labels(m, 4, invert=True), [[0, 2, 2, 0], [2, 0, 2, 0], [2, 2, 2, 2], [0, 0, 2, 0]])
    assert np.array_equal(R.flood_labels(m[:2], 4, invert=True), [[0, 2, 2, 0], [5, 0, 2, 0]])
    checker = R.contents(6, 7)["checkerboard"]
    assert len(np.unique(R.flood_labels(checker, 8))) == 2 and len(np.unique(R.flood_labels(checker, 4))) == 1 + int(checker.sum())
    for name in ("serpentine", "spiral", "u", "comb"):
        m = R.contents(*R.RAGGED)[name]
        for connectivity in (4, 8):
            assert set(np.unique(R.flood_labels(m, connectivity))) == {0, 1}, name
    rows = R.table(R.flood_labels(R.contents(20, 22)["ring and island"], 4))
    assert rows.tolist() == [[2 * 22 + 2 + 1, 120, 2, 2, 19, 17, 0, 0], [6 * 22 + 6 + 1, 80, 6, 6, 15, 13, 0, 0]]
    assert R.table(R.flood_labels(R.specks(), 8))[:, 1].tolist() == [5, 1, 2, 393, 6, 45]
    assert R.table(R.flood_labels(R.specks(), 8))[:, 6].tolist() == [1, 0, 0, 0, 0, 2 | 4]


def test_dense_labels_equal_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    C = _components()
    structures = {4: ndimage.generate_binary_structure(2, 1), 8: ndimage.generate_binary_structure(2, 2)}
    for name, m, connectivity, invert in R.cases():
        want, count = ndimage.label(R.features(m, invert), structure=structures[connectivity])
        got = C.dense_labels(C.label_components_host(m, connectivity=connectivity, invert=invert))
        assert got.dtype == np.int32 and int(got.max()) == count and np.array_equal(got, want), name


def test_dense_labels_without_scipy():
    C = _components()
    lab = np.array([[7, 0, 3], [7, 0, 3], [0, 9, 0]], np.int32)
    assert np.array_equal(C.dense_labels(lab), [[2, 0, 1], [2, 0, 1], [0, 3, 0]])
    assert np.array_equal(C.dense_labels(np.stack([lab, np.zeros_like(lab)])), np.stack([C.dense_labels(lab), np.zeros_like(lab)]))


@pytest.mark.parametrize("name,kind,fn", R.mistakes(), ids=[m[0] for m in R.mistakes()])
def test_the_cases_reject_each_mistake(name, kind, fn):
    if kind == "labels":
        # the big shapes first: most of these mistakes need more than one tile
        for case, m, connectivity, invert in sorted(R.cases(), key=lambda c: -c[1].size):
            if not np.array_equal(fn(m, connectivity, invert), R.truth(case, m, connectivity, invert)):
                return
    elif kind == "frame":
        for case, m, connectivity, invert in R.cases():
            labels = R.truth(case, m, connectivity, invert)
            if not all(np.array_equal(a, b) for a, b in zip(fn(labels), R.areas_frame(labels))):
                return
    else:
        for case, m, min_water, min_land, connectivity, keep in R.clean_cases():
            got, want = fn(m, min_water, min_land, connectivity, keep), R.clean(m, min_water, min_land, connectivity, keep)
            if not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])):
                return
    pytest.fail(f"no case tells '{name}' from the truth")


def test_host_clean_and_bodies_equal_the_restatement(monkeypatch):
    monkeypatch.setenv("RUNET_NO_DEVICE_CCL", "1")       # read at call time
    C = _components()
    for case, m, min_water, min_land, connectivity, keep in R.clean_cases():
        got, info = C.clean_water_mask(m, min_water, min_land, connectivity=connectivity, keep_frame=keep)
        want, counts = R.clean(m, min_water, min_land, connectivity, keep)
        assert got.dtype == np.uint8 and np.array_equal(got, want) and [info[k] for k in C.INFO_KEYS] == counts.tolist(), case
    for connectivity in (4, 8):
        bodies = C.water_bodies(R.specks(), connectivity=connectivity, pixel_size=10.0)
        rows = R.table(R.flood_labels(R.specks(), connectivity))
        assert [b["label"] for b in bodies] == rows[:, 0].tolist() and [b["area"] for b in bodies] == rows[:, 1].tolist()
        assert [b["bbox"] for b in bodies] == [tuple(r[2:6]) for r in rows.tolist()]
        assert [b["area_units"] for b in bodies] == [100.0 * a for a in rows[:, 1].tolist()]
        assert [sum(on << bit for bit, on in enumerate(b["touches_frame"].values())) for b in bodies] == rows[:, 6].tolist()
