"""GPU: the scene ingestion (scene.py, csrc/scene_bands.hip).  Everything is BIT-EQUAL (np.array_equal, no tolerance): the percentiles against
np.percentile as float64, the enhanced image against the numpy restatement tests/scene_ref.py and against the reference's own outputs
(tests/golden/scene_bands.npz), and CoastlineExtractor on raw bands against the same call on scene_ref's uint8 image."""
import importlib

import numpy as np
import pytest
import torch

import coastline_ref as CR
import scene_ref as R
from conftest import load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("water", "rgb", "display")
DTYPES = {"u8": np.uint8, "u16": np.uint16, "i16": np.int16, "f32": np.float32}
# one pixel; one row group; odd sizes; whole 16-byte groups; more rows than blocks would need and rows at every address phase
SHAPES = [(1, 1), (3, 17), (37, 53), (64, 64), (251, 1031)]


def _scene():
    return importlib.import_module("eusipco-2026-robust-unet_amd.scene")


def _full_range(rng, dt, shape):
    if dt == np.float32:
        return (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4, shape)).astype(np.float32)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max + 1, shape).astype(dt)


def _planes(tag, h, w, seed):
    """-> {name: [h, w] plane}: the data patterns at which a radix select can go wrong"""
    dt = DTYPES[tag]
    rng = np.random.default_rng(seed)
    shape = (h, w)
    out = {"full range": _full_range(rng, dt, shape)}
    lowbyte = rng.integers(0, 256, shape)
    digit = rng.integers(0, 256, shape)
    if tag == "u8":
        out["narrow"] = (200 + lowbyte % 7).astype(dt)
    elif tag == "f32":
        out["shared high byte"] = (1.0 + rng.random(shape)).astype(np.float32)                       # [1, 2): sign and exponent shared
        out["top digit only"] = ((digit.astype(np.uint32) << 24) | 0x123456).view(np.float32)        # finite: the mantissa's top bit is clear
        assert np.isfinite(out["top digit only"]).all()
        mixed = (rng.standard_normal(shape) * 3).astype(np.float32)
        u = rng.random(shape)
        mixed[u < 0.2] = 0.0
        mixed[(u >= 0.2) & (u < 0.4)] = -0.0
        den = (rng.integers(1, 1 << 23, shape).astype(np.uint32) | (rng.integers(0, 2, shape).astype(np.uint32) << 31)).view(np.float32)
        mixed[(u >= 0.4) & (u < 0.6)] = den[(u >= 0.4) & (u < 0.6)]                                   # denormals of both signs
        out["negatives, zeros of both signs, denormals"] = mixed
    else:
        base = 0x4200 if tag == "u16" else 0x1200
        out["shared high byte"] = (base + lowbyte).astype(dt)
        out["top digit only"] = ((digit << 8) | 0x5A).astype(np.uint16).view(dt)
    zeros = _full_range(rng, dt, shape)
    zeros[rng.random(shape) < 0.9] = 0
    out["90 % zeros"] = zeros
    out["constant"] = np.full(shape, 77, dt)
    out["two values"] = np.where(rng.random(shape) < 0.5, 3, 250).astype(dt)
    if tag == "i16":
        out["straddling zero"] = rng.integers(-300, 300, shape).astype(dt)
        out["wide: b - a wraps in int16"] = np.where(rng.random(shape) < 0.5, -30000, 30000).astype(dt)
    return out


def _check_percentiles(S, raster, planes):
    names = list(planes)
    for wide in (False, True):
        for i in range(0, len(names), 3):
            sel = list(range(i, min(i + 3, len(names))))
            got = S.band_percentiles(raster, sel, as_float64=wide).cpu().numpy()
            assert got.dtype == np.float64 and got.shape == (len(sel), 2)
            for row, j in zip(got, sel):
                band = planes[names[j]]
                want = np.percentile(band.astype(np.float64) if wide else band, [2, 98])
                assert want.dtype == np.float64 and np.array_equal(row, want), (names[j], wide, row.tolist(), want.tolist())


@pytest.mark.parametrize("h,w", SHAPES)
@pytest.mark.parametrize("tag", list(DTYPES))
def test_band_percentiles_equal_numpy_bit_for_bit(tag, h, w):
    S = _scene()
    planes = _planes(tag, h, w, seed=h * 7919 + w + len(tag))
    _check_percentiles(S, np.stack(list(planes.values())), planes)


@pytest.mark.parametrize("tag", list(DTYPES))
def test_band_percentiles_on_a_column_window(tag):
    """a window of a wider raster, read in place: the row stride is not w, and rows start at every phase of the 16-byte groups"""
    S = _scene()
    h, w, left, full = 37, 53, 5, 71
    planes = _planes(tag, h, full, seed=99)
    r = S.load_raster(np.stack(list(planes.values())), DEV)
    view = r.t[:, :, left:left + w]
    win = S._Raster(view, r.code)
    assert win.args[5:] == (h * full, full, 1) and win.t.data_ptr() == view.data_ptr()
    _check_percentiles(S, win, {k: v[:, left:left + w] for k, v in planes.items()})
    strided = S._Raster(r.t[:, ::2, ::3], r.code)                                 # every other row, every third column
    assert strided.args[5:] == (h * full, 2 * full, 3)
    _check_percentiles(S, strided, {k: v[::2, ::3] for k, v in planes.items()})


def _raster(tag, h, w, seed, bands=6):
    """non-constant scene-like planes with a nodata run"""
    rng = np.random.default_rng(seed)
    a = _full_range(rng, DTYPES[tag], (bands, h, w))
    if tag == "f32":
        a = (rng.random((bands, h, w)) * 0.9 - 0.05).astype(np.float32)
    if h * w > 4:
        a.reshape(bands, -1)[:, : h * w // 10] = 0
    return a


@pytest.mark.parametrize("h,w", SHAPES[1:])
@pytest.mark.parametrize("tag", list(DTYPES))
def test_enhance_scene_equals_the_restatement(tag, h, w):
    S = _scene()
    a = _raster(tag, h, w, seed=h + 31 * w)
    for mode in MODES:
        assert np.array_equal(S.enhance_scene(a, mode), R.enhance_scene(a, mode)), mode
    for bands in (a[:4], a[:3], a[:2], a[0]):                                     # the fallback triple, plain RGB, grey from 2 and from [H, W]
        got = S.enhance_scene(bands, "water")
        assert got.dtype == np.uint8 and got.shape == (h, w, 3) and np.array_equal(got, R.enhance_scene(bands, "water"))


def test_enhance_scene_equals_the_reference_goldens(tmp_path):
    S = _scene()
    g = load_npz("scene_bands.npz")
    for k in [k for k in g if k.startswith("out_")]:
        parts = k.split("_")
        a = g["in_" + parts[1]]
        if len(parts) == 4:
            a = a[:int(parts[2][1:])]
        assert np.array_equal(S.enhance_scene(a, parts[-1]), g[k]), k
    # the other input forms: a .npy path, device tensors (int16, float32), as_tensor
    np.save(tmp_path / "scene.npy", g["in_u16"])
    assert np.array_equal(S.enhance_scene(str(tmp_path / "scene.npy")), g["out_u16_water"])
    for tag in ("i16", "f32", "u8"):
        t = S.enhance_scene(torch.from_numpy(g["in_" + tag]).to(DEV), "rgb", as_tensor=True)
        assert t.is_cuda and t.dtype == torch.uint8 and np.array_equal(t.cpu().numpy(), g[f"out_{tag}_rgb"])
    png, meta = S.convert_scene(g["in_u16"], str(tmp_path / "out" / "scene.png"), str(tmp_path / "meta" / "scene.json"))
    from PIL import Image
    import json
    assert np.array_equal(np.array(Image.open(png)), g["out_u16_water"])
    doc = json.load(open(tmp_path / "meta" / "scene.json", encoding="utf-8"))
    assert set(doc) == {"original_file", "png_file", "image_size", "bands_count", "enhancement_type", "conversion_time", "geo_transform",
                        "projection"}
    assert doc["image_size"] == [53, 37] and doc["bands_count"] == 6 and doc["geo_transform"] is None and doc["projection"] is None
    assert doc["enhancement_type"].startswith("NIR-Red-Green")
    png, meta = S.convert_scene(g["in_u16"][:3], str(tmp_path / "rgb.png"), enhance_water=False)
    assert np.array_equal(np.array(Image.open(png)), g["out_u16_b3_rgb"]) and meta["bands_count"] == 3


def test_float32_cast_rounds_to_float32_before_it_truncates():
    """p_lo = 0 and p_hi = 7 exactly; v = float32(7 m / 255) lies a hair below 7 m / 255 for about half the m, so s is a hair below m in
    float64 and exactly m after the reference's detour through a float32 array: the truncated byte differs by one"""
    S = _scene()
    h, w = 16, 32
    m = np.arange(1, 255)
    band = np.zeros(h * w, np.float32)
    band[:254] = (7.0 * m / 255).astype(np.float32)
    band[254:254 + 40] = 7.0                                                      # 40 of 512 at either end: both percentiles sit in a run
    band = np.random.default_rng(3).permutation(band).reshape(h, w)
    assert np.percentile(band, [2, 98]).tolist() == [0.0, 7.0]
    s = np.clip((band.astype(np.float64) - 0.0) / 7.0 * 255, 0, 255)
    assert int((s.astype(np.float32).astype(np.uint8) != s.astype(np.uint8)).sum()) > 50, "the case must be present"
    a = np.stack([band, band[::-1], band[:, ::-1]])
    for mode in MODES:
        assert np.array_equal(S.enhance_scene(a, mode), R.enhance_scene(a, mode)), mode


def test_darkening_threshold_at_exactly_100():
    """uint16, p_lo = 0, p_hi = 510: v = 195..205 give s = 97.5, 98, ..., 102.5 exactly; 99.5 darkens to 69.65, 100.0 stays 100"""
    S = _scene()
    h, w = 16, 32
    band = np.zeros(h * w, np.uint16)
    band[:440] = np.resize(np.arange(195, 206), 440)
    band[440:480] = 510
    band = np.random.default_rng(4).permutation(band).reshape(h, w)
    assert np.percentile(band, [2, 98]).tolist() == [0.0, 510.0]
    s = (band - np.float64(0.0)) / np.float64(510.0) * 255
    assert (s == 100.0).any() and (s == 99.5).any()
    a = np.stack([band, band, band])
    got = S.enhance_scene(a, "water")
    assert np.array_equal(got, R.enhance_scene(a, "water"))
    assert set(got[band == 200].reshape(-1, 3)[:, 0].tolist()) == {100} and set(got[band == 199].reshape(-1, 3)[:, 0].tolist()) == {69}
    assert set(got[band == 199].reshape(-1, 3)[:, 1].tolist()) == {99}            # channels 1, 2 are not darkened


@pytest.mark.parametrize("tag", list(DTYPES))
def test_constant_band_rule(tag):
    """p_hi == p_lo: the reference casts 0 / 0 and x / 0 to an integer (undefined); here NaN -> 0, +inf -> 255, -inf -> 0.  "display" has its
    guard and is defined in the reference: clip(v, 0, 255)."""
    S = _scene()
    h, w = 20, 50
    band = np.full(h * w, 50, DTYPES[tag])
    band[:5], band[5:10] = 10, 90                                                 # 1 % outliers on either side: both percentiles are 50
    band = np.random.default_rng(5).permutation(band).reshape(h, w)
    assert np.percentile(band, [2, 98]).tolist() == [50.0, 50.0]
    const = np.full((h, w), 7, DTYPES[tag])
    a = np.stack([band, const, band])
    want = np.stack([np.where(band > 50, 255, 0), np.zeros((h, w)), np.where(band > 50, 255, 0)], axis=-1).astype(np.uint8)
    for mode in ("water", "rgb"):
        assert np.array_equal(S.enhance_scene(a, mode), want), mode
    assert np.array_equal(S.enhance_scene(a, "display"), R.enhance_scene(a, "display"))
    one = np.full((3, 1, 1), 9, DTYPES[tag])                                      # a single pixel is a constant band
    assert S.enhance_scene(one, "water").tolist() == [[[0, 0, 0]]] and S.enhance_scene(one, "display").tolist() == [[[9, 9, 9]]]


@pytest.mark.parametrize("w", [53, 64, 5])
def test_output_off_the_16_byte_grid_and_with_a_row_stride(w):
    S = _scene()
    h = 37
    a = _raster("u16", h, w, seed=w)
    want = R.enhance_scene(a, "water")
    r = S.load_raster(a, DEV)
    for off in (1, 2, 3, 5, 16):
        buf = torch.full((h * w * 3 + 64,), 171, device=DEV, dtype=torch.uint8)
        out = buf[off:off + h * w * 3].view(h, w, 3)
        S._enhance(r, "water", out=out)
        assert np.array_equal(out.cpu().numpy(), want), off
        assert int((buf[:off] != 171).sum()) == 0 and int((buf[off + h * w * 3:] != 171).sum()) == 0     # nothing written outside
    wide = torch.full((h, w + 7, 3), 171, device=DEV, dtype=torch.uint8)
    out = wide[:, 2:2 + w]
    assert out.stride(0) == 3 * (w + 7)
    S._enhance(r, "water", out=out)
    assert np.array_equal(out.cpu().numpy(), want)
    assert int((wide[:, :2] != 171).sum()) == 0 and int((wide[:, 2 + w:] != 171).sum()) == 0


def test_non_finite_values_raise_from_the_host_returning_form():
    S = _scene()
    a = _raster("f32", 37, 53, seed=8)
    assert S.enhance_scene(a).shape == (37, 53, 3)
    bad = a.copy()
    bad[4, 3, 7], bad[2, 30, 1] = np.nan, np.inf                                   # both in selected bands (4, 3, 2)
    with pytest.raises(ValueError, match="2 non-finite"):
        S.enhance_scene(bad)
    assert S.enhance_scene(bad, as_tensor=True).shape == (37, 53, 3)               # the device form does not synchronise, so it cannot raise
    unselected = a.copy()
    unselected[0, 1, 1] = np.nan                                                   # band 0 is not part of the water triple
    assert np.array_equal(S.enhance_scene(unselected), S.enhance_scene(a))
    r = S.load_raster(bad, DEV)
    assert S._percentiles(r, (4, 3, 2))[1].item() == 2 and S._percentiles(S.load_raster(_raster("i16", 8, 8, 1), DEV), (0,))[1].item() == 0


@pytest.mark.parametrize("tag,passes", [("u8", 1), ("i16", 2), ("f32", 4)])
def test_timed_entry_point_computes_the_same_and_times_every_pass(tag, passes):
    """runet_band_percentiles_timed (tools/bench_scene.py's entry): the product call with an event around each pass"""
    import ctypes
    S = _scene()
    L = importlib.import_module("eusipco-2026-robust-unet_amd._lib")
    ops = importlib.import_module("eusipco-2026-robust-unet_amd.ops")
    r = S.load_raster(_raster(tag, 37, 53, seed=6), DEV)
    want, _ = S._percentiles(r, (4, 3, 2))
    (k_lo, g_lo), (k_hi, g_hi) = S.percentile_ranks(37 * 53)
    ws = torch.empty(L.lib.runet_band_percentiles_workspace(3), device=DEV, dtype=torch.uint8)
    pct = torch.empty((3, 2), device=DEV, dtype=torch.float64)
    nf = torch.empty(1, device=DEV, dtype=torch.int32)
    ms = (ctypes.c_float * 4)(-5, -5, -5, -5)
    L.check(L.lib.runet_band_percentiles_timed(*r.args, 4, 3, 2, 3, k_lo, g_lo, k_hi, g_hi, 0, pct.data_ptr(), nf.data_ptr(), ws.data_ptr(),
                                               ws.numel(), ops.stream(), ms))
    assert torch.equal(pct, want) and nf.item() == 0
    assert all(t > 0 for t in ms[:passes]) and all(t == 0 for t in ms[passes:]), list(ms)


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def extractor(pkg):
    """test_gpu_coastline.py's U-Net recipe at fewer steps: both sides of the comparisons below run the same network on what must be the same
    bytes, so the mask only has to be non-constant, not accurate"""
    torch.manual_seed(0)
    net = pkg.UNet(3, 2)
    net.load_state_dict(CR.train_plain_unet(steps=6, size=128, n=2, seed=0, lr=1e-3))
    return pkg.CoastlineExtractor(model=net, device=DEV, input_size=128)


def _scene_bands(h, w, seed):
    """uint16 [6, h, w]: bands 4, 3, 2 carry a synthetic RGB scene at another scale and offset, the rest is noise"""
    rgb, _ = CR.synthetic_scene(h, w, seed)
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 65536, (6, h, w)).astype(np.uint16)
    for i, c in zip((4, 3, 2), (0, 1, 2)):
        b[i] = rgb[:, :, c].astype(np.uint16) * 37 + 500
    return b


def test_extractor_on_raw_bands_equals_the_extractor_on_the_enhanced_image(extractor, tmp_path):
    bands = _scene_bands(150, 170, 21)
    image = R.enhance_scene(bands, "water")
    want = extractor.extract_coastline_from_image(image, tiled=True, tile=64, halo=16)
    got = extractor.extract_coastline_from_image(bands, tiled=True, tile=64, halo=16)
    assert 0 < int(want["water_mask"].sum()) < 150 * 170, "a constant mask would show nothing"
    for res in (got, extractor.extract_coastline_from_image(bands=bands, tiled=True, tile=64, halo=16)):
        assert res["image_size"] == (170, 150)
        assert np.array_equal(res["water_mask"], want["water_mask"]) and np.array_equal(res["coastline_mask"], want["coastline_mask"])
        assert (res["water_pixels"], res["coastline_pixels"]) == (want["water_pixels"], want["coastline_pixels"])
        assert res["coastlines"] == want["coastlines"]
    mask = extractor.predict_scene(bands, tile=64, halo=16)
    assert np.array_equal(mask, extractor.predict_scene(image, tile=64, halo=16)) and np.array_equal(mask, want["water_mask"])
    i16 = (bands // 2).astype(np.int16)                                           # a device tensor, and nothing comes back
    t = extractor.predict_scene(bands=torch.from_numpy(i16).to(DEV), tile=64, halo=16, as_tensor=True)
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), extractor.predict_scene(R.enhance_scene(i16, "water"), tile=64, halo=16))
    # the resized path: the enhanced image is what PIL resizes
    np.save(tmp_path / "scene.npy", bands)
    a = extractor.extract_coastline_from_image(str(tmp_path / "scene.npy"))
    b = extractor.extract_coastline_from_image(image)
    assert a["image_path"] == str(tmp_path / "scene.npy") and np.array_equal(a["water_mask"], b["water_mask"])
    assert np.array_equal(a["coastline_mask"], b["coastline_mask"])
    # a uint8 [H, W, 3] image stays an image
    assert np.array_equal(extractor.predict_scene(image, tile=64, halo=16), want["water_mask"])
    bad = bands.astype(np.float32)
    bad[4, 0, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        extractor.extract_coastline_from_image(bad, tiled=True, tile=64, halo=16)
    with pytest.raises(ValueError, match="non-finite"):
        extractor.predict_scene(bad, tile=64, halo=16)
