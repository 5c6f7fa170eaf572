#!/usr/bin/env python3
"""Generate the scene-ingestion golden vectors (tests/golden/scene_bands.npz) from the REFERENCE itself.

Runs only where the reference checkout is present (never on the GPU box).  It imports the reference's predict_coastline.py and
tif_to_image.py in-process; the packages they import at the top but that the enhancement functions never touch (cv2, osgeo, tkinter,
PIL.ImageTk, torchvision) are stubbed in sys.modules.  The three functions are called as unbound methods on synthetic rasters:
CoastlineExtractor.enhance_image_for_water(None, rgb) ("water"), CoastlineExtractor.normalize_image_for_display(None, rgb) ("display") and
TIFToImageConverter.enhance_image(None, rgb, False) ("rgb"; with True it must equal "water", which is asserted).  The band triple is stacked by
tests/scene_ref.stack (the reference picks it inside its GDAL readers).  Nothing from the reference's source is copied: the fixture holds the
input rasters and the uint8 images the reference made of them.  No constant band: those are undefined in the reference.

Usage:  python tests/golden/make_golden_scene.py [path/to/reference checkout]   (or REFERENCE_DIR=...)
"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))


class _Stub(types.ModuleType):
    """a module whose every public attribute is another stub; dunder lookups fail as on a real module, or `inspect` trips"""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        # CamelCase names are subclassed by the GUI (tk.Frame): a plain class; everything else is a further stub
        child = type(name, (), {"__init__": lambda s, *a, **k: None}) if name[0].isupper() else _Stub(self.__name__ + "." + name)
        setattr(self, name, child)
        return child

    def __call__(self, *a, **k):
        return self


for name in ("cv2", "osgeo", "osgeo.gdal", "tkinter", "tkinter.ttk", "tkinter.filedialog", "tkinter.messagebox", "PIL.ImageTk", "torchvision",
             "torchvision.transforms"):
    sys.modules.setdefault(name, _Stub(name))
import matplotlib  # noqa: E402

matplotlib.use("Agg")
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE_DIR", os.path.join(os.path.dirname(ROOT), "reference"))   # default: a sibling checkout
sys.path.insert(0, REF)
pc = importlib.import_module("predict_coastline")
t2i = importlib.import_module("tif_to_image")
sref = importlib.import_module("scene_ref")

B, H, W = 6, 37, 53
MODES = ("water", "rgb", "display")


def rasters():
    """scene-like planes: a smooth land / water gradient plus noise, a nodata corner of zeros (tie run below the 2nd percentile's rank in
    some bands, around it in others), a few saturated pixels"""
    rng = np.random.default_rng(20260)
    yy, xx = np.mgrid[:H, :W]
    base = np.stack([0.5 + 0.4 * np.sin(0.13 * xx + 0.7 * b) * np.cos(0.11 * yy - 0.3 * b) for b in range(B)])
    base = np.clip(base + 0.08 * rng.standard_normal(base.shape), 0, 1)
    nodata = (yy[None] < 2 + np.arange(B)[:, None, None]) & (xx[None] < 9)
    u16 = np.where(nodata, 0, 300 + base * 9000).astype(np.uint16)
    u16[:, 5, 40:43] = 65535
    u8 = np.where(nodata, 0, 4 + base * 240).astype(np.uint8)
    i16 = np.where(nodata, -9999, -800 + base * 6000).astype(np.int16)
    f32 = np.where(nodata, 0.0, -0.05 + base * 0.9 + 1e-4 * rng.standard_normal(base.shape)).astype(np.float32)
    return {"u8": u8, "u16": u16, "i16": i16, "f32": f32}


def reference(rgb, mode):
    with np.errstate(all="ignore"):
        if mode == "water":
            out = pc.CoastlineExtractor.enhance_image_for_water(None, rgb)
            assert np.array_equal(out, t2i.TIFToImageConverter.enhance_image(None, rgb, True)), "the two water enhancements differ"
        elif mode == "display":
            out = pc.CoastlineExtractor.normalize_image_for_display(None, rgb)
        else:
            out = t2i.TIFToImageConverter.enhance_image(None, rgb, False)
        return out.astype(np.uint8)                      # Image.fromarray(x.astype(np.uint8)) at every call site


if __name__ == "__main__":
    out = {}
    for tag, a in rasters().items():
        for b in range(B):
            assert a[b].min() != a[b].max(), "constant band"
        out["in_" + tag] = a
        cases = {"": a}
        if tag == "u16":
            cases.update({"b4_": a[:4], "b3_": a[:3], "b1_": a[:1]})     # four bands: the IndexError fallback; three; grey
        for sub, bands in cases.items():
            for mode in MODES:
                got = reference(sref.stack(bands, mode), mode)
                assert got.dtype == np.uint8 and got.shape == (H, W, 3)
                assert np.array_equal(got, sref.enhance_scene(bands, mode)), (tag, sub, mode, "scene_ref differs from the reference")
                out[f"out_{tag}_{sub}{mode}"] = got
    path = os.path.join(HERE, "scene_bands.npz")
    np.savez_compressed(path, **out)
    print("scene_bands.npz:", len(out), "arrays,", os.path.getsize(path), "bytes, numpy", np.__version__)
