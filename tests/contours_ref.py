"""The device contour tracer's formulation (csrc/contours.hip, include/runet_hip.h) restated in numpy, and the masks both contour test files
run: border following as a successor map on states (pixel, direction to the previous pixel), start states from two labellings, a walk of
the map from each start back to itself, and the vertex rule.  predict.trace_external_contours is the oracle for it and for the device."""
import numpy as np
from scipy import ndimage

import coastline_ref

DI = (0, -1, -1, -1, 0, 1, 1, 1)                          # E, NE, N, NW, W, SW, S, SE; y grows downwards
DJ = (1, 1, 0, -1, -1, -1, 0, 1)
POPC = np.array([bin(v).count("1") for v in range(256)], dtype=np.int64)


def neighbour_bits(m):
    """m: bool [h, w] -> uint8 [h, w], bit d = the neighbour in direction d is set (outside the image is clear)"""
    h, w = m.shape
    pad = np.zeros((h + 2, w + 2), dtype=bool)
    pad[1:-1, 1:-1] = m
    nb = np.zeros((h, w), dtype=np.int64)
    for d in range(8):
        nb |= pad[1 + DI[d]:1 + DI[d] + h, 1 + DJ[d]:1 + DJ[d] + w].astype(np.int64) << d
    return nb


def successor_map(mask, candidates_only=True):
    """-> dict(spix, sdir, succ, ldir, sbase, has): the states in raster order of their pixels and ascending direction, each state's
    successor, and the direction its pixel is left in.  candidates_only: states only on set pixels with a clear 4-neighbour, a state whose
    successor would leave them is its own successor, an isolated pixel carries one state (direction 8) that is its own successor - the
    device's state set.  Otherwise every valid state of every set pixel (isolated pixels have none)."""
    m = np.asarray(mask) != 0
    h, w = m.shape
    nb = neighbour_bits(m)
    has = m & ((nb & 0x55) != 0x55) if candidates_only else m
    nbf = np.where(has, nb, 0).reshape(-1)
    hasf = has.reshape(-1)
    count = POPC[nbf]
    if candidates_only:
        count = np.where(hasf & (nbf == 0), 1, count)
    sbase = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64)
    n = int(count.sum())
    spix = np.repeat(np.arange(h * w), count)
    within = np.arange(n) - sbase[spix]
    sdir = np.zeros(n, dtype=np.int64)
    for s in range(n):                                    # the within-th set bit of the pixel's neighbour byte
        b, k = int(nbf[spix[s]]), int(within[s])
        if b == 0:
            sdir[s] = 8
            continue
        d = 0
        while True:
            if (b >> d) & 1:
                if k == 0:
                    break
                k -= 1
            d += 1
        sdir[s] = d
    succ = np.arange(n)
    ldir = np.full(n, 8, dtype=np.int64)
    for s in range(n):
        d = int(sdir[s])
        if d == 8:
            continue
        p, b = int(spix[s]), int(nbf[spix[s]])
        e = d
        for _ in range(8):
            e = (e + 1) % 8
            if (b >> e) & 1:
                break
        q = p + DI[e] * w + DJ[e]
        back = (e + 4) % 8
        ldir[s] = e
        if hasf[q]:
            succ[s] = sbase[q] + POPC[int(nbf[q]) & ((1 << back) - 1)]
    return {"spix": spix, "sdir": sdir, "succ": succ, "ldir": ldir, "sbase": sbase, "nb": nbf, "has": hasf}


def start_pixels(mask):
    """The raster-first pixel of every 8-connected component whose west neighbour (clear by construction) is 4-connected to the outside of
    the zero-padded image, in raster order."""
    m = np.asarray(mask) != 0
    h, w = m.shape
    pad = np.zeros((h + 2, w + 2), dtype=bool)
    pad[1:-1, 1:-1] = m
    fg, n_fg = ndimage.label(pad, structure=np.ones((3, 3), dtype=int))
    bg, _ = ndimage.label(~pad, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    outside = bg[0, 0]
    flat = fg.reshape(-1)
    labels, first = np.unique(flat, return_index=True)
    out = []
    for lab, at in zip(labels.tolist(), first.tolist()):
        if lab == 0:
            continue
        i, j = divmod(at, w + 2)
        if bg[i, j - 1] == outside:
            out.append((i - 1) * w + (j - 1))
    return sorted(out)


def trace(mask, min_points=0):
    """trace_external_contours by the parallel formulation -> list of int32 [n, 2] arrays of (x, y)"""
    m = np.asarray(mask)
    h, w = m.shape
    if h == 0 or w == 0:
        return []
    sm = successor_map(m)
    spix, sdir, succ, ldir, sbase, nb = sm["spix"], sm["sdir"], sm["succ"], sm["ldir"], sm["sbase"], sm["nb"]
    contours = []
    for p0 in start_pixels(m):
        b = int(nb[p0])
        assert sm["has"][p0] and not (b & 0x10)
        if b == 0:
            s0 = int(sbase[p0])
        else:
            d1 = next(d for d in (3, 2, 1, 0, 7, 6, 5) if (b >> d) & 1)      # the first set neighbour clockwise from west
            s0 = int(sbase[p0] + POPC[b & ((1 << d1) - 1)])
            assert sdir[s0] == d1
        pts, dirs = [], []
        s = s0
        while True:
            pts.append(int(spix[s]))
            dirs.append(int(ldir[s]))
            assert succ[s] != s or sdir[s] == 8, "a border cycle ran into a state outside the candidate pixels"
            s = int(succ[s])
            if s == s0:
                break
        assert min(pts) == p0, "the start pixel is the smallest of its cycle"
        n = len(pts)
        keep = [t for t in range(n) if dirs[t] != dirs[t - 1]] if n > 1 else [0]
        pa = np.array([pts[t] for t in keep], dtype=np.int64)
        c = np.stack([pa % w, pa // w], axis=1).astype(np.int32)
        if len(c) > min_points:
            contours.append(c)
    return contours


# ------------------------------------------------------------------------------------------------ the masks of both test files
def spiral(n):
    """a one-pixel-wide square spiral from the corner inwards, one clear pixel between its arms"""
    m = np.zeros((n, n), dtype=np.uint8)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = 1
    while True:
        moved = False
        for _ in range(2):
            ny, nx, ny2, nx2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < n and 0 <= nx < n and not m[ny, nx] and not (0 <= ny2 < n and 0 <= nx2 < n and m[ny2, nx2]):
                y, x = ny, nx
                m[y, x] = 1
                moved = True
                break
            dy, dx = dx, -dy
        if not moved:
            return m


def serpentine(n):
    """a one-pixel line over every second row, joined alternately at the right and the left end"""
    m = np.zeros((n, n), dtype=np.uint8)
    m[0::2, :] = 1
    m[1::4, -1] = 1
    m[3::4, 0] = 1
    return m


def smooth_field_water(size=256, seed=11):
    rng = np.random.default_rng(seed)
    return (ndimage.gaussian_filter(rng.standard_normal((size, size)), 6.0) > 0).astype(np.uint8)


def coastline_band(size=256, seed=11):
    return coastline_ref.dilate_diff(smooth_field_water(size, seed), 5)[0]


def noise(h, w, density, seed):
    return (np.random.default_rng(seed).random((h, w)) < density).astype(np.uint8)


def _ring(m, y0, x0, y1, x1):
    m[y0:y1, x0:x1] = 1
    m[y0 + 1:y1 - 1, x0 + 1:x1 - 1] = 0


def cases():
    """-> list of (name, uint8 mask)"""
    out = []

    def add(name, m):
        out.append((name, np.ascontiguousarray(m, dtype=np.uint8)))

    # degenerate
    add("empty", np.zeros((9, 13)))
    add("all_ones", np.ones((9, 13)))
    add("1x1_set", np.ones((1, 1)))
    add("1x1_clear", np.zeros((1, 1)))
    for name, (i, j) in {"corner_nw": (0, 0), "corner_ne": (0, -1), "corner_sw": (-1, 0), "corner_se": (-1, -1)}.items():
        m = np.zeros((7, 10))
        m[i, j] = 1
        add(name, m)
    dash = (np.arange(200) % 5 < 3).astype(np.uint8)
    add("row_full", np.ones((1, 200)))
    add("row_dashed", dash[None, :])
    add("col_full", np.ones((200, 1)))
    add("col_dashed", dash[:, None])
    m = noise(20, 30, 0.5, 3)
    add("values_2_and_255", m * np.where(noise(20, 30, 0.5, 4) > 0, 2, 255))
    # launch-plan edges
    add("5x3", noise(5, 3, 0.6, 5))
    add("37x53", noise(37, 53, 0.45, 6))
    add("64x64", noise(64, 64, 0.5, 7))
    add("130x259", noise(130, 259, 0.5, 8))
    # connectivity duality
    m = np.zeros((12, 12))
    m[2:5, 2:5] = 1
    m[5:8, 5:8] = 1
    add("squares_touching_at_a_corner", m)
    m = np.zeros((13, 13))
    for k in range(5):                                   # a diamond: closed through diagonal steps only
        m[1 + k, 6 - k] = m[1 + k, 6 + k] = m[11 - k, 6 - k] = m[11 - k, 6 + k] = 1
    m[6, 1] = m[6, 11] = 1
    m[6, 6] = 1
    add("diagonal_ring_with_dot", m)
    # nesting
    m = np.zeros((30, 30))
    _ring(m, 1, 1, 29, 29)
    _ring(m, 6, 6, 24, 24)
    m[14:16, 14:16] = 1
    add("dot_in_ring_in_ring", m)
    m = np.zeros((20, 44))
    _ring(m, 2, 2, 18, 20)
    _ring(m, 3, 24, 17, 42)
    m[8:11, 9:12] = 1
    m[9, 32] = 1
    add("two_rings_with_islands", m)
    m = np.zeros((24, 30))
    _ring(m, 5, 10, 15, 22)                              # a hole that touches nothing
    m[0:9, 0:7] = 1
    m[2:6, 0:4] = 0                                      # a component on the frame whose "hole" opens onto the frame
    m[3, 1] = 1                                          # and a pixel inside that bay: the bay is outside, so this is top-level
    add("hole_and_frame_bay", m)
    # long chains
    sp, se = spiral(64), serpentine(128)
    add("spiral_64", sp)
    add("serpentine_128", se)
    add("spiral_64_complement", 1 - sp)
    add("serpentine_128_complement", 1 - se)
    # noise
    for hw in ((96, 96), (130, 259)):
        for k, dens in enumerate((0.10, 0.30, 0.55, 0.80, 0.95)):
            add(f"noise_{hw[0]}x{hw[1]}_{dens:.2f}", noise(hw[0], hw[1], dens, 100 + 10 * hw[0] + k))
    add("coastline_band_256", coastline_band())
    return out
