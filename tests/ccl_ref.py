"""Connected components, their areas and the area filter, restated as plainly as Python allows (include/runet_hip.h states the rules;
csrc/ccl.hip and components.py implement them).  Everything is an integer and is compared with np.array_equal: there is no tolerance.

  flood_labels(mask, connectivity, invert)   a breadth-first flood fill: label = 1 + min(y * w + x) over the component, literally
  areas_frame(labels)                        runet_ccl_areas: pixel count and frame bits at every root, 0 elsewhere
  table(labels)                              runet_ccl_table: the rows {label, area, x0, y0, x1, y1, frame, 0} in ascending label
  clean(mask, ...)                           clean_water_mask on top of the flood fill -> (mask, the four counts)
  contents(h, w) / cases() / clean_cases()   named masks
  mistakes()                                 named wrong variants; test_ccl_ref_cpu.py shows that the cases tell each from the truth
"""
import numpy as np

T = 64                                                   # the kernel's tile side, both axes
STEPS4 = ((-1, 0), (0, -1), (0, 1), (1, 0))
STEPS8 = STEPS4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))


def features(mask, invert=False):
    mask = np.asarray(mask)
    return (mask == 0) if invert else (mask != 0)


def flood_labels(mask, connectivity=8, invert=False, edge_ok=None, largest=False, wrap=False):
    """int32 [h, w].  The three switches are the mistakes below: edge_ok(y, x, ny, nx) -> False drops a contact; largest takes the
    maximum index; wrap lets x + 1 run on into the next row."""
    feat = features(mask, invert)
    h, w = feat.shape
    steps = STEPS4 if connectivity == 4 else STEPS8
    f = feat.reshape(-1).tolist()
    lab = [0] * (h * w)
    for s in range(h * w):
        if not f[s] or lab[s]:
            continue
        comp = [s]
        lab[s] = -1
        i = 0
        while i < len(comp):
            p = comp[i]
            i += 1
            y, x = divmod(p, w)
            for dy, dx in steps:
                ny, nx = y + dy, x + dx
                if wrap and dy == 0:
                    if not 0 <= p + dx < h * w:
                        continue
                    ny, nx = divmod(p + dx, w)
                elif not (0 <= ny < h and 0 <= nx < w):
                    continue
                q = ny * w + nx
                if f[q] and not lab[q] and (edge_ok is None or edge_ok(y, x, ny, nx)):
                    lab[q] = -1
                    comp.append(q)
        root = max(comp) if largest else min(comp)
        for p in comp:
            lab[p] = root + 1
    return np.array(lab, dtype=np.int32).reshape(h, w)


_TRUTH = {}


def truth(name, mask, connectivity, invert):
    """flood_labels, computed once per named case and shared by the tests of a process; the array is read-only"""
    key = (name, mask.shape, connectivity, invert)
    if key not in _TRUTH:
        _TRUTH[key] = flood_labels(mask, connectivity, invert)
        _TRUTH[key].setflags(write=False)
    return _TRUTH[key]


# ------------------------------------------------------------------------------------------------ areas, frame, table, filter
def table(labels, skip_side=None):
    """int64 [K, 8]; skip_side: the mistake of a frame bit that is never set"""
    labels = np.asarray(labels)
    h, w = labels.shape
    rows = []
    for lab in np.unique(labels[labels != 0]):
        ys, xs = np.nonzero(labels == lab)
        sides = (ys.min() == 0, ys.max() == h - 1, xs.min() == 0, xs.max() == w - 1)
        frame = sum(1 << bit for bit, on in enumerate(sides) if on and bit != skip_side)
        rows.append((int(lab), ys.size, xs.min(), ys.min(), xs.max(), ys.max(), frame, 0))
    return np.array(rows, dtype=np.int64).reshape(-1, 8)


def areas_frame(labels, skip_side=None):
    """-> (areas int32 [h, w], frame uint8 [h, w])"""
    labels = np.asarray(labels)
    areas, frame = np.zeros(labels.size, np.int32), np.zeros(labels.size, np.uint8)
    for row in table(labels, skip_side):
        areas[row[0] - 1], frame[row[0] - 1] = row[1], row[6]
    return areas.reshape(labels.shape), frame.reshape(labels.shape)


def select(labels, min_area, keep_frame, value, out, inclusive=False, skip_side=None):
    """runet_ccl_filter_u8 on one image: out changed in place -> (components, pixels).  inclusive: the mistake `<=`."""
    comps = pixels = 0
    for row in table(labels, skip_side):
        small = row[1] <= min_area if inclusive else row[1] < min_area
        if small and not (keep_frame and row[6] != 0):
            out[labels == row[0]] = value
            comps += 1
            pixels += int(row[1])
    return comps, pixels


def clean(mask, min_water=0, min_land=0, connectivity=8, keep_frame=True, inclusive=False, same_connectivity=False, skip_side=None):
    """clean_water_mask -> (uint8 mask, int64 [4] = removed water components, pixels, filled land components, pixels)"""
    out = np.array(mask, dtype=np.uint8, copy=True)
    counts = np.zeros(4, dtype=np.int64)
    if min_water:
        counts[0:2] = select(flood_labels(out, connectivity), min_water, keep_frame, 0, out, inclusive, skip_side)
    if min_land:
        dual = connectivity if same_connectivity else 12 - connectivity
        counts[2:4] = select(flood_labels(out, dual, invert=True), min_land, keep_frame, 1, out, inclusive, skip_side)
    return out, counts


# ------------------------------------------------------------------------------------------------ contents
def _random(h, w, density, seed):
    return (np.random.default_rng(seed).random((h, w)) < density).astype(np.uint8)


def _spiral(h, w):
    """a one-pixel path that winds inwards with one-pixel gaps: one component under either connectivity, with the longest union chains"""
    m = np.zeros((h, w), np.uint8)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = 1

    def free(yy, xx):
        return not (0 <= yy < h and 0 <= xx < w) or not m[yy, xx]

    while True:
        for _ in range(2):
            ny, nx = y + dy, x + dx
            if 0 <= ny < h and 0 <= nx < w and not m[ny, nx] and free(ny + dy, nx + dx):
                y, x = ny, nx
                m[y, x] = 1
                break
            dy, dx = dx, -dy                             # turn right
        else:
            return m


def tile_corners(h, w):
    return [(a, b) for a in range(T, h, T) for b in range(T, w, T)]


def contents(h, w, seed=0):
    """the named contents of one shape"""
    yy, xx = np.mgrid[0:h, 0:w]
    out = {"empty": np.zeros((h, w), np.uint8), "full": np.full((h, w), 255, np.uint8), "checkerboard": ((xx + yy) % 2).astype(np.uint8)}
    corners = np.zeros((h, w), np.uint8)
    corners[0, 0] = corners[0, w - 1] = corners[h - 1, 0] = corners[h - 1, w - 1] = 1
    out["corners"] = corners
    side = min(h, w)
    out["diagonals"] = (((yy == xx) | (xx == side - 1 - yy)) & (yy < side)).astype(np.uint8)
    # two pixels that touch only diagonally across a four-tile corner, at every tile corner, in either orientation
    down, up = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    for a, b in tile_corners(h, w):
        down[a - 1, b - 1] = down[a, b] = 1
        up[a - 1, b] = up[a, b - 1] = 1
    out["corner pairs down"], out["corner pairs up"] = down, up
    # the last pixel of a row and the first of the next: never neighbours
    ends = np.zeros((h, w), np.uint8)
    if h > 1 and w > 2:
        ends[0, w - 1] = ends[1, 0] = 1
        ends[h - 2, w - 1] = ends[h - 1, 0] = 1
    out["row ends"] = ends
    # even rows full, joined alternately at the right and the left end
    snake = ((yy % 2) == 0).astype(np.uint8)
    for y in range(1, h, 2):
        snake[y, w - 1 if (y // 2) % 2 == 0 else 0] = 1
    out["serpentine"] = snake
    out["spiral"] = _spiral(h, w)
    # two arms that meet only in the last row: the smaller label travels down, across and back up
    u = np.zeros((h, w), np.uint8)
    u[:, 0] = u[:, w - 1] = u[h - 1, :] = 1
    out["u"] = u
    comb = ((xx % 3) == 0).astype(np.uint8)
    comb[h - 1, :] = 1
    out["comb"] = comb
    if min(h, w) >= 14:                                  # a ring two pixels thick, a hole, an island in the hole
        ring = np.zeros((h, w), np.uint8)
        ring[2:h - 2, 2:w - 2] = 1
        ring[4:h - 4, 4:w - 4] = 0
        ring[6:h - 6, 6:w - 6] = 1
        out["ring and island"] = ring
    for k, density in enumerate((0.05, 0.407, 0.5, 0.593, 0.9)):
        out[f"random {density}"] = _random(h, w, density, seed + k)
    return out


SMALL_SHAPES = ((1, 1), (1, 7), (7, 1), (3, 5), (16, 17), (1, 300), (300, 1))
# T - 1 / T / T + 1 and 2 T - 1 / 2 T / 2 T + 1 in each axis
PLAN_SHAPES = tuple((5, w) for w in (63, 64, 65, 127, 128, 129)) + tuple((h, 6) for h in (63, 64, 65, 127, 128, 129))
RAGGED = (131, 137)                                      # 3 x 3 tiles, the last row and column of tiles 3 and 9 pixels
BATCH = (3, 70, 75)


def cases():
    """-> [(name, mask uint8 [h, w], connectivity, invert)]"""
    out = []
    for h, w in SMALL_SHAPES + PLAN_SHAPES + (RAGGED,):
        for name, m in contents(h, w, seed=h * 100 + w).items():
            for connectivity in (4, 8):
                for invert in (False, True):
                    out.append((f"{h}x{w} {name} c{connectivity}{' inverted' if invert else ''}", m, connectivity, invert))
    return out


def batch():
    c = contents(BATCH[1], BATCH[2], seed=5)
    return np.stack([c["random 0.593"], c["spiral"], c["ring and island"]])


def specks():
    """40 x 44.  A lake of 393 pixels (20 x 20 less its holes) with two land holes: 4 pixels in a square, and 3 in a diagonal line, which
    is one hole under 8 and three under 4.  Water specks inland of 1, 2 (diagonal: one under 8, two under 4) and 6 pixels.  At the frame: a
    pond of 5 pixels on the top row, and a bay of 45 pixels in the bottom left corner with a pier of 3 land pixels on the bottom row."""
    m = np.zeros((40, 44), np.uint8)
    m[10:30, 10:30] = 1
    m[14:16, 14:16] = 0
    m[20, 20] = m[21, 21] = m[22, 22] = 0
    m[3, 3] = 1
    m[5, 20] = m[6, 21] = 1
    m[33:35, 30:33] = 1
    m[0, 38:43] = 1
    m[36:40, 0:12] = 1
    m[39, 4:7] = 0
    return m


# 1; the exact areas above and of the 20 x 22 ring (120), its hole (88) and island (80), each with area + 1; more than everything
THRESHOLDS = (1, 2, 3, 4, 5, 6, 7, 45, 46, 80, 81, 88, 89, 120, 121, 393, 394, 2000)


def clean_cases():
    """-> [(name, mask, min_water, min_land, connectivity, keep_frame)]: thresholds 1, each exact area and area + 1, keep_frame both ways"""
    out = []
    masks = {"specks": specks(), "ring and island": contents(20, 22)["ring and island"]}
    for name, m in masks.items():
        for connectivity in (4, 8):
            for keep in (True, False):
                for t in THRESHOLDS:
                    out.append((f"{name} c{connectivity} keep {keep} water {t}", m, t, 0, connectivity, keep))
                    out.append((f"{name} c{connectivity} keep {keep} land {t}", m, 0, t, connectivity, keep))
                    out.append((f"{name} c{connectivity} keep {keep} both {t}", m, t, t, connectivity, keep))
    return out


# ------------------------------------------------------------------------------------------------ mistakes
def _same_tile_or_straight(y, x, ny, nx):
    """a diagonal contact that leaves the tile in both axes at once is dropped"""
    return not (y // T != ny // T and x // T != nx // T)


def _same_tile_row(y, x, ny, nx):
    """tiles are merged along x only"""
    return y // T == ny // T


def mistakes():
    """-> [(name, kind, fn)]: kind "labels": fn(mask, connectivity, invert) -> int32 [h, w];  kind "frame": fn(labels) -> (areas, frame);
    kind "clean": fn(mask, min_water, min_land, connectivity, keep_frame) -> (mask, counts)"""
    return [("connectivities swapped", "labels", lambda m, c, inv: flood_labels(m, 12 - c, inv)),
            ("diagonal seam pairs at tile corners omitted", "labels", lambda m, c, inv: flood_labels(m, c, inv, edge_ok=_same_tile_or_straight)),
            ("seams merged in one axis only", "labels", lambda m, c, inv: flood_labels(m, c, inv, edge_ok=_same_tile_row)),
            ("maximum instead of minimum index", "labels", lambda m, c, inv: flood_labels(m, c, inv, largest=True)),
            ("row-end wrap-around", "labels", lambda m, c, inv: flood_labels(m, c, inv, wrap=True)),
            ("a frame bit missing for one side", "frame", lambda labels: areas_frame(labels, skip_side=3)),
            ("area <= min_area instead of <", "clean", lambda m, a, b, c, k: clean(m, a, b, c, k, inclusive=True)),
            ("land holes under the same connectivity as water", "clean", lambda m, a, b, c, k: clean(m, a, b, c, k, same_connectivity=True))]
