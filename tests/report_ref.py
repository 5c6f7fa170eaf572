"""numpy-only restatement of the arrays behind the reference's two report figures (predict_coastline.py:708-835,
Extended_Baseline_Comparison.py:882-959), with the operations numpy itself performs in those lines: boolean / coordinate indexing,
np.histogram, np.diff, float32 arrays for what torch computes in float32.  Written independently of report.py; the yardstick of
test_report_ref_cpu.py and test_gpu_report.py."""
import math

import numpy as np

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def combined_overlay(display, water, coast):
    """:710-728 on masks that already have the display's size"""
    img = np.array(display, dtype=np.uint8, copy=True)
    ys, xs = np.where(water == 1)
    if len(ys) > 0:
        img[ys, xs] = img[ys, xs] * 0.6 + np.array([0, 100, 200]) * 0.4
    ys, xs = np.where(coast == 1)
    if len(ys) > 0:
        img[ys, xs] = [255, 255, 255]
    return img


def ndwi(bands):
    """:795-800: GetRasterBand(4) and (2) are planes 3 and 1"""
    nir, green = bands[3], bands[1]
    with np.errstate(all="ignore"):
        return (green.astype(float) - nir.astype(float)) / (green.astype(float) + nir.astype(float) + 1e-8)


def _hist(values, bins):
    counts, edges = np.histogram(values, bins=bins)
    with np.errstate(all="ignore"):                      # an empty selection: 0 / 0, NaN, as numpy gives it
        density = np.histogram(values, bins=bins, density=True)[0]
    return {"counts": counts, "edges": edges, "density": density}


def ndwi_histograms(bands, water, bins=50):
    """:803-809: plt.hist(., bins, density=True) is np.histogram of the flattened selection"""
    x = ndwi(np.asarray(bands))
    return {"water": _hist(x[water == 1].flatten(), bins), "other": _hist(x[water == 0].flatten(), bins)}


def rgb_histograms(image, bins=50):
    """:822-829"""
    return {name: _hist(np.asarray(image)[:, :, i].flatten(), bins) for i, name in enumerate(("red", "green", "blue"))}


def coastline_lengths(coastlines):
    """:763-770: open polylines, segment by segment; math.sqrt of an exact integer, then numpy's sum of the segment lengths"""
    out = []
    for line in coastlines:
        if len(line) <= 1:
            continue
        segments = [math.sqrt((int(x1) - int(x0)) ** 2 + (int(y1) - int(y0)) ** 2) for (x0, y0), (x1, y1) in zip(line[:-1], line[1:])]
        out.append(float(np.sum(np.array(segments, dtype=np.float64))))
    return out


def statistics(water, coast):
    """:739-742"""
    total, n_water, n_coast = water.size, int(np.sum(water, dtype=np.int64)), int(np.sum(coast, dtype=np.int64))
    return {"total_pixels": total, "water_pixels": n_water, "coastline_pixels": n_coast, "water_ratio": n_water / total * 100}


def bin_by_edges(x, edges):
    """the rule the kernels state: bin i iff edges[i] <= x < edges[i + 1], the last bin closed on the right; plain comparisons"""
    bins = len(edges) - 1
    counts = np.zeros(bins, dtype=np.int64)
    for i in range(bins):
        hi = (x <= edges[i + 1]) if i == bins - 1 else (x < edges[i + 1])
        counts[i] = int(np.count_nonzero((x >= edges[i]) & hi))
    return counts


def fixed_order_sum(err):
    """float32 [n] -> the float64 sum in the order include/runet_hip.h states for runet_error_overlays"""
    e = np.asarray(err, dtype=np.float32).reshape(-1)
    nb = -(-e.size // 1024)
    p = np.zeros(nb * 1024, dtype=np.float64)
    p[:e.size] = e
    p = p.reshape(nb, 4, 256)
    d = ((p[:, 0] + p[:, 1]) + p[:, 2]) + p[:, 3]
    a = d.reshape(nb, 4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        a = a[:, :, :o] + a[:, :, o:2 * o]
    chunk = ((a[:, 0, 0] + a[:, 1, 0]) + a[:, 2, 0]) + a[:, 3, 0]
    lanes = np.zeros(64, dtype=np.float64)
    for k0 in range(0, nb, 64):
        row = chunk[k0:k0 + 64]
        lanes[:row.size] = lanes[:row.size] + row
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes[:o] + lanes[o:2 * o]
    return np.float64(lanes[0])


COLOURS = np.array([[0.2, 0.8, 0.2], [0.9, 0.2, 0.2], [0.2, 0.2, 0.9], [0.9, 0.9, 0.9], [0.0, 0.0, 0.0]])      # TP FP FN TN, no class


def error_overlays(images, prob, masks, threshold=0.5, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """Extended_Baseline_Comparison.py:883-959 for all samples at once, by class index: float32 arrays where torch computes in float32,
    float64 where numpy promotes (0.6 * colour, and its sum with the float32 product 0.4 * image)"""
    x, p, g = (np.asarray(a, dtype=np.float32) for a in (images, prob, masks))
    n, _, h, w = x.shape
    p, g = p[:, 0], g[:, 0]
    with np.errstate(all="ignore"):
        vis = x * np.float32(std)[None, :, None, None] + np.float32(mean)[None, :, None, None]
        vis = np.clip(vis, np.float32(0), np.float32(1)).transpose(0, 2, 3, 1)
        positive = p > np.float32(threshold)
    cls = np.where(g == 1, np.where(positive, 0, 2), np.where(g == 0, np.where(positive, 1, 3), 4))
    dimmed = np.float32(0.4) * vis
    assert dimmed.dtype == np.float32
    counts = np.stack([(cls == k).sum(axis=(1, 2)) for k in range(5)], axis=1).astype(np.int64)
    err = np.abs(p - g)
    sums = np.array([fixed_order_sum(e) for e in err], dtype=np.float64)
    return {"image": np.ascontiguousarray(vis), "overlay": dimmed.astype(np.float64) + (0.6 * COLOURS)[cls], "error_map": err, "counts": counts,
            "error_sum": sums, "iou": counts[:, 0] / (counts[:, 0] + counts[:, 1] + counts[:, 2] + 1e-8), "mae": sums / (h * w)}
