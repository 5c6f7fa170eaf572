"""The exact Douglas-Peucker rule of include/runet_hip.h restated independently of predict.approx_poly_dp_exact and of the kernel's rounds:
a plain recursive Douglas-Peucker on Python ints and np.float64 scalars (every float64 operation rounded once), with a record of what
happened on the way, switchable NAMED MISTAKES that a wrong implementation might make, and the hand-built inputs of the tests."""
import sys
from fractions import Fraction

import numpy as np

COORD_MAX = 46340
SQRT2 = float.fromhex("0x1.6a09e667f3bcdp+0")
MISTAKES = ("unclipped", "last_index", "ge", "fused_L")


def arc_terms(p):
    """-> (A, D): the summed lengths of the axis edges and the summed |dx| of the diagonal edges of the closed contour; ValueError on a
    vertex outside [0, COORD_MAX] or an edge that is neither"""
    n = len(p)
    for i, (x, y) in enumerate(p):
        if not (0 <= x <= COORD_MAX and 0 <= y <= COORD_MAX):
            raise ValueError(f"vertex {i} out of range")
    a = d = 0
    for i in range(n):
        dx, dy = abs(p[(i + 1) % n][0] - p[i][0]), abs(p[(i + 1) % n][1] - p[i][1])
        if dx == 0 or dy == 0:
            a += dx + dy
        elif dx == dy:
            d += dx
        else:
            raise ValueError(f"edge {i} is not a run")
    return a, d


def arc_length(a, d, fused=False):
    """L of step 1: two rounded operations, or (the mistake) one fused multiply-add, emulated in exact rationals"""
    if fused:
        return np.float64(float(Fraction(a) + Fraction(d) * Fraction(SQRT2)))
    return np.float64(a) + np.float64(d) * np.float64(SQRT2)


def threshold(p, eps_factor, fused=False):
    a, d = arc_terms(p)
    eps = np.float64(eps_factor) * arc_length(a, d, fused)
    return eps * eps


def numerator(qa, qb, qi, unclipped=False):
    """-> (N, den) of step 4"""
    abx, aby = qb[0] - qa[0], qb[1] - qa[1]
    apx, apy = qi[0] - qa[0], qi[1] - qa[1]
    den = abx * abx + aby * aby
    if den == 0:
        return apx * apx + apy * apy, 1
    cross2 = (apx * aby - apy * abx) ** 2
    if unclipped:
        return cross2, den
    dot = apx * abx + apy * aby
    if dot <= 0:
        return (apx * apx + apy * apy) * den, den
    if dot >= den:
        return ((qi[0] - qb[0]) ** 2 + (qi[1] - qb[1]) ** 2) * den, den
    return cross2, den


def simplify(points, eps_factor, mistakes=()):
    """-> (kept vertices int32 [k, 2], record).  record: splits, ties (splits whose largest N is reached by more than one position),
    far_ties (vertices as far from p[0] as `far`, beyond the first), margin (the smallest |lhs - rhs| / rhs of a decision with rhs > 0,
    inf without one), depth (the deepest level of a segment with an interior position; the two chains are level 1)."""
    assert set(mistakes) <= set(MISTAKES)
    p = [(int(x), int(y)) for x, y in np.asarray(points).reshape(-1, 2)]
    n = len(p)
    rec = {"splits": 0, "ties": 0, "far_ties": 0, "margin": float("inf"), "depth": 0, "far": 0}
    thr = threshold(p, eps_factor, "fused_L" in mistakes)
    rec["thr"] = float(thr)
    if n == 0:
        return np.zeros((0, 2), np.int32), rec
    d2 = [(x - p[0][0]) ** 2 + (y - p[0][1]) ** 2 for x, y in p]
    far = min(i for i in range(n) if d2[i] == max(d2))
    rec["far"] = far
    rec["far_ties"] = sum(1 for v in d2 if v == d2[far]) - 1 if far else 0
    if far == 0:
        return np.array(p[:1], np.int32), rec
    q = p + [p[0]]
    keep = [False] * (n + 1)
    keep[0] = keep[far] = keep[n] = True
    old_limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old_limit, 2 * n + 1000))

    def chain(a, b, level):
        if b - a < 2:
            return
        rec["depth"] = max(rec["depth"], level)
        nums = []
        den = 1
        for i in range(a + 1, b):
            num, den = numerator(q[a], q[b], q[i], "unclipped" in mistakes)
            nums.append(num)
        best = max(nums)
        at = [a + 1 + j for j, v in enumerate(nums) if v == best]
        k = at[-1] if "last_index" in mistakes else at[0]
        lhs, rhs = np.float64(float(best)), thr * np.float64(float(den))
        if rhs > 0:
            rec["margin"] = min(rec["margin"], float(abs(lhs - rhs) / rhs))
        if (lhs >= rhs) if "ge" in mistakes else (lhs > rhs):
            rec["splits"] += 1
            rec["ties"] += len(at) > 1
            keep[k] = True
            chain(a, k, level + 1)
            chain(k, b, level + 1)

    try:
        chain(0, far, 1)
        chain(far, n, 1)
    finally:
        sys.setrecursionlimit(old_limit)
    return np.array([p[i] for i in range(n) if keep[i]], np.int32), rec


def pack(contours):
    """list of [k, 2] arrays -> the tracer's packed int32 {n, total, offsets [n + 1], points [total][2]}"""
    lens = [len(c) for c in contours]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    pts = np.concatenate([np.asarray(c, np.int32).reshape(-1, 2) for c in contours]).reshape(-1) if contours else np.zeros(0, np.int32)
    return np.concatenate([np.array([len(contours), int(off[-1])], np.int32), off, pts.astype(np.int32)])


def unpack(packed):
    packed = np.asarray(packed, np.int32)
    n, total = int(packed[0]), int(packed[1])
    off = packed[2:3 + n]
    pts = packed[3 + n:3 + n + 2 * total].reshape(total, 2)
    return [pts[off[i]:off[i + 1]].copy() for i in range(n)]


# ------------------------------------------------------------------------------------------------ hand-built inputs (not from the tracer)
LONG_VERTICES = 4402                                     # more than twice the 2048 vertices up to which the kernel keeps its state in LDS

# Perimeter 64 h with h = 4 and eps_factor = 1 / 64, so eps == h == 4 and thr == 16 exactly: out along y = 0 with a bump of height h, back
# along y = 0.  Vertices 2 and 3 lie at distance exactly h from the chord (0, 0) - (124, 0): N == thr * den, `>` keeps the chord, `>=` splits.
THRESHOLD_TIE = (np.array([[0, 0], [40, 0], [40, 4], [80, 4], [80, 0], [124, 0]], np.int32), 1.0 / 64.0)

# A trapezoid with A = 24, D = 18: (double)A + (double)D * sqrt2 rounds differently in one fused operation than in two (asserted by the
# CPU test).  Vertex 1 over the chord p[0] - p[2] has N = 729 and den = 225, N / den = 3.24; eps_factor is the double, found by stepping
# through the neighbours of sqrt(N / den) / L on the CPU, at which thr is 3.24 for the unfused L (`>` fails: the chord stays) and
# 3.2399999999999993 for the fused one (it splits).
FUSED_L = (np.array([[9, 0], [12, 0], [21, 9], [0, 9]], np.int32), float.fromhex("0x1.2a28290c1c381p-5"))


def skyline(widths, heights, x0=0, y0=0, diagonal_close=False):
    """(x0, y0), up to the first height, then right / up-or-down over the columns, down to y0 (or, with diagonal_close, straight back along
    a 45 degree edge: the caller makes the last x equal the last height), back along y = y0"""
    pts = [(0, 0)]
    x = 0
    for w, h in zip(widths, heights):
        pts += [(x, h), (x + w, h)]
        x += w
    if not diagonal_close:
        pts.append((x, 0))
    return np.array([(x0 + a, y0 + b) for a, b in pts], np.int32)


def long_contour():
    """one rectilinear contour of LONG_VERTICES vertices: a noisy skyline over a slow swell"""
    rng = np.random.default_rng(41)
    m = (LONG_VERTICES - 2) // 2
    widths = rng.integers(1, 4, m)
    swell = 400 + 300 * np.sin(np.arange(m) / 97.0) + 80 * np.sin(np.arange(m) / 11.0)
    heights = (swell + rng.integers(0, 25, m)).astype(np.int64)
    heights[1:][heights[1:] == heights[:-1]] += 1
    c = skyline(widths.tolist(), heights.tolist(), 3, 5)
    assert len(c) == LONG_VERTICES
    return c


def many_small(count=300, seed=17):
    """`count` contours of 11, 12 or 13 vertices (11 and 13 close along a diagonal)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        n = 11 + i % 3
        cols = 5 if n < 13 else 6
        heights = rng.integers(1, 30, cols).tolist()
        for j in range(1, cols):
            if heights[j] == heights[j - 1]:
                heights[j] += 1
        widths = rng.integers(1, 9, cols).tolist()
        diag = n != 12
        if diag:                                          # the last corner (X, h) closes on (0, 0) along a diagonal: X == h
            need = heights[-1] - sum(widths[:-1])
            if need < 1:
                heights[-1] = sum(widths[:-1]) + int(rng.integers(1, 6))
                need = heights[-1] - sum(widths[:-1])
                if cols > 1 and heights[-1] == heights[-2]:
                    heights[-1] += 1
                    need += 1
            widths[-1] = need
        c = skyline(widths, heights, int(rng.integers(0, 2000)), int(rng.integers(0, 2000)), diagonal_close=diag)
        assert len(c) == n, (len(c), n)
        out.append(c)
    return out


def hand_built():
    """-> list of (name, [contours], eps_factor)"""
    s = COORD_MAX
    plus = np.array([[5, 5], [9, 5], [5, 5], [5, 9], [5, 5], [1, 5], [5, 5], [5, 1]], np.int32)      # every arm walked out and back
    comb = np.array([[0, 3], [6, 3], [6, 9], [6, 3], [12, 3], [12, 0], [12, 3], [20, 3], [12, 3], [6, 3]], np.int32)
    full = [np.array([[0, 0], [s, 0], [s, s], [0, s]], np.int32),
            np.array([[0, 0], [s, s], [s, 0]], np.int32),
            np.array([[0, s], [s // 2, s // 2], [s, s], [s, 0], [0, 0]], np.int32),
            np.array([[0, 0], [s, 0], [s - 1, 1], [s, 2], [s, s], [s - 7, s], [s - 7, s - 3], [0, s - 3]], np.int32)]
    out = [("threshold_tie", [THRESHOLD_TIE[0]], THRESHOLD_TIE[1]),
           ("fused_L", [FUSED_L[0]], FUSED_L[1]),
           ("full_range", full, 0.002),
           ("full_range_eps0", full, 0.0),
           ("revisits", [plus, comb], 0.002),
           ("revisits_eps0", [plus, comb], 0.0),
           ("long", [long_contour()], 0.002),
           ("long_fine", [long_contour()], 0.00005),
           ("many_small", many_small(), 0.002),
           ("many_small_coarse", many_small(), 0.05),
           ("short", [np.array([[7, 7]], np.int32), np.array([[1, 1], [4, 4]], np.int32), np.array([[3, 3], [3, 3]], np.int32),
                      np.array([[2, 2], [2, 9], [2, 2]], np.int32)], 0.002)]
    return out


BAD_INPUTS = {"knight_move": [np.array([[0, 0], [5, 0], [6, 2], [0, 2]], np.int32)],
              "coordinate_46341": [np.array([[0, 0], [COORD_MAX + 1, 0], [COORD_MAX + 1, 8], [0, 8]], np.int32)],
              "negative_coordinate": [np.array([[3, 3], [9, 3], [9, 9], [3, 9]], np.int32), np.array([[0, 0], [-1, 0], [-1, 4], [0, 4]], np.int32)]}
