"""The exact Euclidean distance transform and its statistics, restated as plainly as numpy allows (include/runet_hip.h states the rules;
csrc/edt.hip and boundary.py implement them).  Squared distances between pixels are integers, so everything here is compared with
np.array_equal: there is no tolerance anywhere.

  brute_d2(mask, invert)   the [h * w, features] table of squared distances, for masks of up to about 4000 pixels
  truth(mask, invert)      its row minima as int32 [h, w]; NONE where the image has no feature
  stats(d2, select, tol)   runet_edt_stats: the counts, and the root sum in the header's order
  cases()                  named masks
  mistakes()               named wrong variants; test_edt_ref_cpu.py shows that the cases can tell each of them from the truth
"""
import numpy as np

NONE = 2 ** 31 - 1


def features(mask, invert=False):
    mask = np.asarray(mask)
    return (mask == 0) if invert else (mask != 0)


def brute_d2(mask, invert=False):
    """int32 [h * w, F]: entry (p, k) = the squared distance from pixel p (row-major) to the k-th feature pixel (row-major)"""
    feat = features(mask, invert)
    h, w = feat.shape
    py, px = (a.reshape(-1, 1).astype(np.int32) for a in np.mgrid[0:h, 0:w])
    fy, fx = (a.astype(np.int32)[None] for a in np.nonzero(feat))
    return (py - fy) ** 2 + (px - fx) ** 2


def _minima(table, shape):
    if table.shape[1] == 0:
        return np.full(shape, NONE, dtype=np.int32)
    return table.min(axis=1).reshape(shape).astype(np.int32)


def truth(mask, invert=False):
    return _minima(brute_d2(mask, invert), np.asarray(mask).shape)


# ------------------------------------------------------------------------------------------------ statistics
def ordered_sum(e):
    """the header's order: chunks of 1024 (zeros beyond the end); in a chunk d[t] = ((e[t] + e[t + 256]) + e[t + 512]) + e[t + 768], four
    groups of 64 folded by halves, chunk = ((a0 + a1) + a2) + a3; lane l adds the chunks l, l + 64, ... from 0.0; the lanes fold by halves"""
    e = np.asarray(e, dtype=np.float64).reshape(-1)
    nblk = max(1, (e.size + 1023) // 1024)
    padded = np.zeros(nblk * 1024)
    padded[:e.size] = e
    chunks = []
    for c in padded.reshape(nblk, 1024):
        d = ((c[0:256] + c[256:512]) + c[512:768]) + c[768:1024]
        a = []
        for grp in d.reshape(4, 64):
            grp = grp.copy()
            for o in (32, 16, 8, 4, 2, 1):
                grp[:o] += grp[o:2 * o]
            a.append(grp[0])
        chunks.append(((a[0] + a[1]) + a[2]) + a[3])
    lanes = np.zeros(64)
    for k, v in enumerate(chunks):
        lanes[k % 64] += v
    for o in (32, 16, 8, 4, 2, 1):
        lanes[:o] += lanes[o:2 * o]
    return lanes[0]


def stats(d2, select=None, tol_sq=(), strict=False):
    """d2 int32 [n, h, w], select uint8 [n, h, w] or None -> (counts int64 [n, 4 + len(tol_sq)], sums float64 [n]).
    strict: the mistake `<` where the rule says `<=`."""
    d2 = np.asarray(d2)
    n = d2.shape[0]
    counts = np.zeros((n, 4 + len(tol_sq)), dtype=np.int64)
    sums = np.zeros(n, dtype=np.float64)
    for i in range(n):
        v = d2[i].reshape(-1).astype(np.int64)
        sel = np.ones(v.size, dtype=bool) if select is None else np.asarray(select)[i].reshape(-1) != 0
        live = sel & (v != NONE)
        counts[i, 0] = sel.sum()
        counts[i, 1] = (sel & (v == NONE)).sum()
        counts[i, 2] = v[live].max() if live.any() else 0
        counts[i, 3] = v[live].sum()
        for t, tol in enumerate(tol_sq):
            counts[i, 4 + t] = (v[live] < tol).sum() if strict else (v[live] <= tol).sum()
        sums[i] = ordered_sum(np.where(live, np.sqrt(np.where(live, v, 0).astype(np.float64)), 0.0))
    return counts, sums


# ------------------------------------------------------------------------------------------------ cases
def _random(h, w, density, seed):
    return (np.random.default_rng(seed).random((h, w)) < density).astype(np.uint8)


def _corners(h, w):
    m = np.zeros((h, w), np.uint8)
    m[0, 0] = 1
    return m


def contents(h, w, seed=0):
    """the named contents of one shape"""
    yy, xx = np.mgrid[0:h, 0:w]
    out = {"no feature": np.zeros((h, w), np.uint8), "all features": np.full((h, w), 255, np.uint8), "corner 00": _corners(h, w),
           "corner 01": _corners(h, w)[:, ::-1].copy(), "corner 10": _corners(h, w)[::-1].copy(), "corner 11": _corners(h, w)[::-1, ::-1].copy(),
           "alternating columns": ((xx % 2) == 0).astype(np.uint8), "alternating rows": ((yy % 2) == 1).astype(np.uint8),
           "checkerboard": ((xx + yy) % 2).astype(np.uint8), "random 0.5": _random(h, w, 0.5, seed), "random 0.05": _random(h, w, 0.05, seed + 1)}
    ends = np.zeros((h, w), np.uint8)
    ends[0, 0] = ends[h - 1, w - 1] = 7
    out["two ends"] = ends
    last = np.zeros((h, w), np.uint8)                    # one feature in the last row and one in the last column, neither in a corner
    last[h - 1, w // 2] = last[h // 2, w - 1] = 1
    out["last lines"] = last
    return out


SMALL_SHAPES = ((1, 1), (1, 7), (7, 1), (3, 5), (16, 17))
BRUTE_SHAPES = ((64, 64), (65, 67))                      # the table is [h w, F]: sparse contents only
SPARSE = ("no feature", "corner 00", "corner 01", "corner 10", "corner 11", "two ends", "last lines", "random 0.05")


def cases():
    """-> [(name, mask uint8 [h, w], invert)], every one small enough for brute_d2"""
    out = []
    for h, w in SMALL_SHAPES:
        for name, m in contents(h, w, seed=h * 100 + w).items():
            for invert in (False, True):
                out.append((f"{h}x{w} {name}{' inverted' if invert else ''}", m, invert))
    for h, w in BRUTE_SHAPES:
        for name, m in contents(h, w, seed=h * 100 + w).items():
            if name in SPARSE:
                out.append((f"{h}x{w} {name}", m, False))
        out.append((f"{h}x{w} random 0.95 inverted", _random(h, w, 0.95, h), True))
    return out


# ------------------------------------------------------------------------------------------------ mistakes
def _two_pass(feat, drop_last=False, empty_as_zero=False):
    """the separable form, written with minima over whole lines: g = the gap to the nearest feature of the same row (rows without one are
    not valid), then d2[y][x] = min over valid rows y' of (y - y')^2 + g[y'][x]^2.  The two switches are the mistakes below."""
    h, w = feat.shape
    x = np.arange(w)
    gap = np.abs(x[:, None] - x[None, :])                                         # [x, x']
    valid = feat.any(axis=1)
    g = np.where(feat[:, None, :], gap[None], 10 ** 6).min(axis=2)                # [y, x]
    if empty_as_zero:
        g, valid = np.where(valid[:, None], g, 0), np.ones(h, dtype=bool)
    if drop_last:
        valid = valid.copy()
        valid[h - 1] = False
    if not valid.any():
        return np.full((h, w), NONE, dtype=np.int32)
    y = np.arange(h)
    rows = np.flatnonzero(valid)
    cand = (y[:, None, None] - rows[None, :, None]) ** 2 + (g[rows] ** 2)[None]   # [y, y', x]
    return cand.min(axis=1).astype(np.int32)


def _column_pass_only(mask, invert):
    feat = features(mask, invert)
    h, w = feat.shape
    y = np.arange(h)
    gap = np.where(feat.T[:, None, :], np.abs(y[:, None] - y[None, :])[None], 10 ** 6).min(axis=2).T     # [y, x]
    return np.where(feat.any(axis=0)[None], gap ** 2, NONE).astype(np.int32)


def _city_block(mask, invert):
    feat = features(mask, invert)
    h, w = feat.shape
    py, px = (a.reshape(-1, 1) for a in np.mgrid[0:h, 0:w])
    fy, fx = (a[None] for a in np.nonzero(feat))
    return _minima((np.abs(py - fy) + np.abs(px - fx)) ** 2, (h, w))


def _frame_is_background(mask, invert):
    """the published Boundary IoU code's zero padding: with invert the ring around the image is a feature"""
    padded = np.pad(np.asarray(mask), 1)
    return truth(padded, invert)[1:-1, 1:-1]


def mistakes():
    """-> [(name, kind, fn)]: kind "d2": fn(mask, invert) -> int32 [h, w];  kind "stats": fn(d2, select, tol_sq) -> (counts, sums)"""
    return [("column pass only", "d2", _column_pass_only),
            ("city-block instead of Euclidean", "d2", _city_block),
            ("envelope off by one at a line end", "d2", lambda m, inv: _two_pass(features(m, inv), drop_last=True)),
            ("empty lines taking part as distance 0", "d2", lambda m, inv: _two_pass(features(m, inv), empty_as_zero=True)),
            ("frame counted as background", "d2", _frame_is_background),
            ("< instead of <= at a tolerance", "stats", lambda d2, sel, tol: stats(d2, sel, tol, strict=True))]
