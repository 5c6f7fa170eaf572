"""CPU: what of the connected-component calls can be checked without a GPU - the exported names, the host-side refusals of the C ABI
(every one returns before any device work), clean_water_mask's argument rules and its numpy route, and the extractor's signature."""
import ctypes
import importlib
import inspect

import numpy as np
import pytest

import ccl_ref as R

NAMES = ("label_components", "label_components_host", "dense_labels", "water_bodies", "clean_water_mask")
ENTRY_POINTS = ("runet_ccl_workspace_bytes", "runet_ccl_label_u8", "runet_ccl_areas", "runet_ccl_filter_u8", "runet_ccl_table")


def _components():
    return importlib.import_module("eusipco-2026-robust-unet_amd.components")


def test_the_new_symbols_are_exported(pkg):
    L = importlib.import_module("eusipco-2026-robust-unet_amd._lib")
    for name in NAMES:
        assert name in pkg.__all__ and callable(getattr(pkg, name)), name
    for name in ENTRY_POINTS:
        assert name in L.PROTOS and hasattr(L.lib, name), name


def test_refusals_return_error_codes_without_a_gpu():
    lib = importlib.import_module("eusipco-2026-robust-unet_amd._lib").lib
    p = ctypes.c_void_p(64)                              # never dereferenced: every call below is refused on the host
    big = 1 << 50
    assert lib.runet_ccl_workspace_bytes(1, 64, 64) > 0 and lib.runet_ccl_workspace_bytes(1, 64, 64) % 8 == 0
    assert lib.runet_ccl_workspace_bytes(1, 32768, 32768) > 0 and lib.runet_ccl_workspace_bytes(3, 1, 1) > 0
    for n, h, w in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (1, 32769, 4), (1, 4, 32769), (-1, 4, 4), (2 ** 31 - 1, 64, 64), (1025, 32768, 32768)):
        assert lib.runet_ccl_workspace_bytes(n, h, w) < 0, (n, h, w)
    short = lib.runet_ccl_workspace_bytes(1, 4, 4) - 1
    # runet_ccl_label_u8(mask, n, h, w, row_stride, image_stride, invert, connectivity, labels, workspace, workspace_bytes, stream)
    for args, word in (((None, 1, 4, 4, 4, 16, 0, 8, p, p, big, None), b"null pointer"),
                       ((p, 1, 4, 4, 4, 16, 0, 8, None, p, big, None), b"null pointer"),
                       ((p, 1, 4, 4, 4, 16, 0, 8, p, None, big, None), b"null pointer"),
                       ((p, 1, 4, 4, 4, 16, 0, 6, p, p, big, None), b"connectivity must be 4 or 8"),
                       ((p, 1, 4, 4, 4, 16, 0, 0, p, p, big, None), b"connectivity must be 4 or 8"),
                       ((p, 0, 4, 4, 4, 16, 0, 4, p, p, big, None), b"bad shape"),
                       ((p, 1, 32769, 4, 4, 16, 0, 8, p, p, big, None), b"h and w must not exceed 32768"),
                       ((p, 1, 4, 32769, 32769, 16, 0, 8, p, p, big, None), b"h and w must not exceed 32768"),
                       ((p, 2 ** 31 - 1, 64, 64, 64, 4096, 0, 8, p, p, big, None), b"batch too large"),
                       ((p, 1, 4, 4, 3, 16, 0, 8, p, p, big, None), b"row stride"),
                       ((p, 2, 4, 4, 4, 15, 0, 8, p, p, big, None), b"image stride"),
                       ((p, 1, 4, 4, 4, 16, 0, 8, p, p, short, None), b"workspace too small"),
                       ((p, 1, 4, 4, 4, 16, 0, 8, ctypes.c_void_p(66), p, big, None), b"misaligned")):
        assert lib.runet_ccl_label_u8(*args) != 0 and word in lib.runet_last_error(), (args, lib.runet_last_error())
    # runet_ccl_areas(labels, n, h, w, areas, frame, stream)
    for args, word in (((None, 1, 4, 4, p, p, None), b"null pointer"), ((p, 1, 4, 4, None, p, None), b"null pointer"),
                       ((p, 1, 4, 4, p, None, None), b"null pointer"), ((p, 1, 32769, 4, p, p, None), b"32768"),
                       ((p, 1, 4, 0, p, p, None), b"bad shape")):
        assert lib.runet_ccl_areas(*args) != 0 and word in lib.runet_last_error(), (args, lib.runet_last_error())
    # runet_ccl_filter_u8(labels, areas, frame, n, h, w, min_area, keep_frame, value, mask_out, counts, stream)
    for args, word in (((None, p, p, 1, 4, 4, 1, 1, 0, p, p, None), b"null pointer"), ((p, p, p, 1, 4, 4, 1, 1, 0, None, p, None), b"null pointer"),
                       ((p, p, p, 1, 4, 4, 1, 1, 0, p, None, None), b"null pointer"), ((p, p, p, 1, 4, 32769, 1, 1, 0, p, p, None), b"32768"),
                       ((p, p, p, 1, 4, 4, -1, 1, 0, p, p, None), b"min_area"), ((p, p, p, 1, 4, 4, 1, 1, 256, p, p, None), b"byte")):
        assert lib.runet_ccl_filter_u8(*args) != 0 and word in lib.runet_last_error(), (args, lib.runet_last_error())
    # runet_ccl_table(labels, areas, frame, n, h, w, capacity, n_components, table, workspace, workspace_bytes, stream)
    for args, word in (((None, p, p, 1, 4, 4, 1, p, p, p, big, None), b"null pointer"), ((p, p, p, 1, 4, 4, 1, None, p, p, big, None), b"null pointer"),
                       ((p, p, p, 1, 4, 4, 1, p, None, p, big, None), b"null pointer"), ((p, p, p, 1, 4, 4, 1, p, p, None, big, None), b"null pointer"),
                       ((p, p, p, 1, 4, 4, -1, p, p, p, big, None), b"capacity"), ((p, p, p, 1, 32769, 4, 1, p, p, p, big, None), b"32768"),
                       ((p, p, p, 1, 4, 4, 1, p, p, p, short, None), b"workspace too small")):
        assert lib.runet_ccl_table(*args) != 0 and word in lib.runet_last_error(), (args, lib.runet_last_error())


def test_clean_water_mask_with_both_thresholds_at_zero_returns_the_input_bytes():
    C = _components()
    m = (np.random.default_rng(0).integers(0, 3, (9, 11)) * 100).astype(np.uint8)
    out, info = C.clean_water_mask(m, device="cuda:0")   # no step runs, so no device is touched
    assert out is not m and out.dtype == np.uint8 and np.array_equal(out, m) and info == dict.fromkeys(C.INFO_KEYS, 0)
    out, info = C.clean_water_mask(np.stack([m, m]) != 0)
    assert out.shape == (2, 9, 11) and np.array_equal(out, np.stack([m, m]) != 0) and info == (dict.fromkeys(C.INFO_KEYS, 0),) * 2


def test_clean_water_mask_on_the_numpy_route(monkeypatch):
    monkeypatch.setenv("RUNET_NO_DEVICE_CCL", "1")       # read at call time
    C = _components()
    m = R.specks()
    for min_water, min_land, connectivity, keep in ((7, 0, 8, True), (0, 5, 8, True), (7, 5, 4, False), (2000, 2000, 8, False), (46, 4, 4, True)):
        got, info = C.clean_water_mask(m, min_water, min_land, connectivity=connectivity, keep_frame=keep, device="cuda:0")
        want, counts = R.clean(m, min_water, min_land, connectivity, keep)
        assert np.array_equal(got, want) and [info[k] for k in C.INFO_KEYS] == counts.tolist(), (min_water, min_land, connectivity, keep)
    # everything below 7 pixels inland goes, the lake's holes are filled, and what touches the frame stays
    got, info = C.clean_water_mask(m, 7, 5, connectivity=8)
    assert info == {"removed_water_components": 3, "removed_water_pixels": 9, "filled_land_components": 4, "filled_land_pixels": 7}
    assert got[10:30, 10:30].all() and got[0, 38:43].all() and not got[39, 4:7].any() and got.sum() == 400 + 5 + 45
    labels = C.label_components(m, connectivity=4, invert=True, device="cuda:0")
    assert np.array_equal(labels, R.flood_labels(m, 4, invert=True))
    assert np.array_equal(C.label_components(m, as_tensor=True).numpy(), R.flood_labels(m, 8))


def test_bad_arguments_raise():
    C = _components()
    m = np.zeros((4, 5), np.uint8)
    for kwargs in ({"min_water_area": -1}, {"min_land_area": -1}, {"min_water_area": 2.0}, {"min_land_area": 1.5}, {"min_water_area": True},
                   {"min_water_area": "3"}, {"min_water_area": None}, {"connectivity": 6}, {"connectivity": True}):
        with pytest.raises(ValueError):
            C.clean_water_mask(m, **kwargs)
    for bad in (np.zeros((4, 5), np.int32), np.zeros(5, np.uint8), np.zeros((1, 2, 3, 4), np.uint8), np.zeros((0, 5), np.uint8),
                np.zeros((1, 32769), np.uint8)):
        with pytest.raises(ValueError):
            C.clean_water_mask(bad, 1, 1)
        with pytest.raises(ValueError):
            C.label_components_host(bad)
    with pytest.raises(ValueError):
        C.label_components(m, connectivity=5)
    with pytest.raises(ValueError):
        C.water_bodies(m, connectivity=0)


def test_the_extractor_takes_the_cleanup_arguments(pkg):
    for method in (pkg.CoastlineExtractor.extract_coastline_from_image, pkg.CoastlineExtractor.extract_coastline_contours):
        params = inspect.signature(method).parameters
        assert [params[k].default for k in ("min_water_area", "min_land_area", "connectivity")] == [0, 0, 8]
