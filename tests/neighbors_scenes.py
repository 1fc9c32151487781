"""Label planes for the Neighbors_* tests, with the values worked out by hand.  scenes() returns
name -> (labels int32 [H, W], max_label, scales); HAND lists (scene, label, scale index, column,
value) for check_hand().  The GPU tests compare the kernel with tests/neighbors_ref.py on every
scene; the CPU tests check the restatement itself against HAND."""
import numpy as np

import neighbors_ref as nr


def _plane(h, w):
    return np.zeros((h, w), np.int32)


def _rect(lab, r0, c0, h, w, L):
    lab[r0:r0 + h, c0:c0 + w] = L
    return lab


def _pair(offset):
    """Single-pixel objects 1 at (20, 20) and 2 at (20, 20) + offset, D = 5."""
    lab = _plane(41, 41)
    lab[20, 20] = 1
    lab[20 + offset[0], 20 + offset[1]] = 2
    return lab


# offset -> (neighbour at D = 5, touching at D = 5)
PAIRS = {(3, 4): (1, 1), (1, 5): (0, 1), (2, 5): (0, 1), (4, 4): (0, 0), (0, 6): (0, 0), (0, 5): (1, 1)}


def size_scene(kind, band, seg, D=5):
    """One object larger than a band and a segment of the kernel, with a hole that holds the only
    other object, a single pixel at exactly D from the hole's rim and on the boundary itself: the
    first row of the window's second band with the rim D above it ("band_up"), the last row of the
    first band with the rim D below it ("band_down"), and the same for the first two segments
    ("seg_left", "seg_right").  Each is reached only at dy (dx) = +-D, through the outermost row
    (column) of a tile's halo."""
    r0, c0 = 10, 12
    h, w = band + 40, seg + 50
    lab = _plane(r0 + h + 20, c0 + w + 20)
    _rect(lab, r0, c0, h, w, 1)
    yb, xb = r0 - D + band, c0 - D + seg  # first row / column of the window's second band / segment
    if kind == "band_up":       # rim row yb - D (band 0), neighbour row yb, the first of band 1: its reach
        _rect(lab, yb - D + 1, c0 + 15, 24, 31, 0)  # at dy = -D is the outermost row of band 1's halo
        lab[yb, c0 + 30] = 2
    elif kind == "band_down":   # neighbour row yb - 1, the last of band 0, rim row yb - 1 + D (band 1): the
        _rect(lab, yb + D - 1 - 24, c0 + 15, 24, 31, 0)  # outermost row of band 0's lower halo
        lab[yb - 1, c0 + 30] = 2
    elif kind == "seg_left":    # rim column xb - D (segment 0), neighbour column xb, the first of segment 1
        _rect(lab, r0 + 10, xb - D + 1, 31, 24, 0)
        lab[r0 + 25, xb] = 2
    elif kind == "seg_right":   # neighbour column xb - 1, the last of segment 0, rim column xb - 1 + D
        _rect(lab, r0 + 10, xb + D - 1 - 24, 31, 24, 0)
        lab[r0 + 25, xb - 1] = 2
    else:
        raise ValueError(kind)
    return lab


SIZE_KINDS = ("band_up", "band_down", "seg_left", "seg_right")


def seeded_blobs(seed, h, w, n, rmin, rmax):
    """Discs at random places; a later disc takes only background."""
    rng = np.random.default_rng(seed)
    lab = _plane(h, w)
    yy, xx = np.mgrid[:h, :w]
    for L in range(1, n + 1):
        r, cy, cx = rng.integers(rmin, rmax + 1), rng.integers(0, h), rng.integers(0, w)
        m = ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r) & (lab == 0)
        lab[m] = L
    return lab


def seeded_dense(seed, h, w, n, reach):
    """Every pixel within `reach` of a random seed takes the nearest seed's label: touching cells."""
    rng = np.random.default_rng(seed)
    sy, sx = rng.integers(0, h, n), rng.integers(0, w, n)
    yy, xx = np.mgrid[:h, :w]
    d2 = (yy[..., None] - sy) ** 2 + (xx[..., None] - sx) ** 2
    lab = (d2.argmin(axis=-1) + 1).astype(np.int32)
    lab[d2.min(axis=-1) > reach * reach] = 0
    return lab


def scenes(band=64, seg=64):
    s = {}
    s["blank"] = (_plane(20, 24), 8, ("Adjacent", 5))
    s["one"] = (_rect(_plane(20, 24), 5, 6, 4, 7, 3), 8, ("Adjacent", 5))
    s["two"] = (_rect(_rect(_plane(20, 24), 5, 6, 4, 7, 3), 12, 3, 3, 3, 5), 8, ("Adjacent", 5))
    s["1x1"] = (np.array([[1]], np.int32), 4, ("Adjacent", 5))
    line = np.array([1, 1, 0, 2, 2, 2, 0, 0, 3], np.int32)
    s["1x9"] = (line[None].copy(), 4, ("Adjacent", 2, 5))
    s["9x1"] = (line[:, None].copy(), 4, ("Adjacent", 2, 5))
    lab = _plane(30, 30)
    for L, (r, c) in enumerate(((0, 0), (0, 26), (26, 0), (26, 26)), start=1):
        _rect(lab, r, c, 4, 4, L)
    _rect(lab, 13, 13, 4, 4, 5)
    s["corners"] = (lab, 8, (5, 15))
    s["side"] = (_rect(_rect(_plane(12, 16), 3, 2, 4, 4, 1), 3, 6, 4, 4, 2), 4, ("Adjacent", 2))
    s["corner_only"] = (_rect(_rect(_plane(12, 16), 2, 2, 4, 4, 1), 6, 6, 4, 4, 2), 4, ("Adjacent", 2))
    s["gap"] = (_rect(_rect(_plane(12, 16), 3, 2, 4, 4, 1), 3, 7, 4, 4, 2), 4, ("Adjacent", 2))
    for off in PAIRS:
        s[f"pair_{off[0]}_{off[1]}"] = (_pair(off), 4, (5,))
    # a 9 x 9 ring (2) around a 5 x 5 square (1) with the same centre, and a third object
    lab = _rect(_rect(_plane(40, 40), 16, 16, 9, 9, 2), 18, 18, 5, 5, 1)
    _rect(lab, 30, 5, 3, 3, 3)
    s["ring"] = (lab, 4, ("Adjacent", 3))
    lab = _plane(24, 24)
    for i in range(3):
        for j in range(3):
            _rect(lab, 3 + 6 * i, 3 + 6 * j, 6, 6, 1 + 3 * i + j)
    s["grid"] = (lab, 16, ("Adjacent", 2))
    # single pixels: four at distance 5 around (10, 10) on the axes, four more at 3-4-5 offsets
    lab = _plane(24, 24)
    for L, (r, c) in enumerate(((5, 10), (6, 7), (7, 14), (10, 5), (10, 10), (10, 15), (13, 6), (14, 13), (15, 10)),
                               start=1):
        lab[r, c] = L
    s["ties"] = (lab, 16, ("Adjacent",))
    # labels with gaps, one equal to max_label, one above it (background, but it makes an edge)
    lab = _rect(_rect(_rect(_rect(_plane(30, 40), 4, 4, 5, 5, 1), 4, 9, 5, 5, 7), 12, 20, 6, 6, 8), 18, 20, 4, 6, 300)
    _rect(lab, 4, 14, 5, 5, 999)
    _rect(lab, 22, 20, 3, 3, -4)
    s["labels"] = (lab, 300, ("Adjacent", 3))
    # one 40 x 40 object (50) with 100 single-pixel objects one background pixel off its sides
    lab = _rect(_plane(60, 60), 10, 10, 40, 40, 50)
    others = [L for L in range(1, 102) if L != 50]
    for i in range(25):
        p = 10 + 1 + i + (i // 2)  # 25 places along a side, not all adjacent to each other
        for side, (r, c) in enumerate(((8, p), (51, p), (p, 8), (p, 51))):
            lab[r, c] = others[4 * i + side]
    s["many"] = (lab, 128, ("Adjacent", 2))
    for kind in SIZE_KINDS:
        s[f"size_{kind}"] = (size_scene(kind, band, seg), 4, (4, 5))
    s["d32"] = (seeded_blobs(11, 100, 100, 12, 3, 9), 16, (32,))
    s["four_scales"] = (seeded_blobs(12, 70, 90, 14, 3, 8), 16, ("Adjacent", 2, 5, 7))
    s["dense"] = (seeded_dense(13, 96, 120, 40, 9), 64, ("Adjacent", 5))
    return s


def _c(s, col):
    return nr.N_NEIGHBORS * s + col


NN, PT, FN, FD, SN, SD, AN = range(nr.N_NEIGHBORS)
# (scene, label, scale index, column, value)
HAND = [
    ("one", 3, 0, NN, 0), ("one", 3, 1, PT, 0), ("one", 3, 0, FN, 0), ("one", 3, 1, AN, 0),
    ("two", 3, 0, FN, 5), ("two", 5, 0, FN, 3), ("two", 3, 0, SN, 0), ("two", 3, 0, SD, 0), ("two", 3, 0, AN, 0),
    ("two", 3, 1, NN, 1), ("two", 3, 0, NN, 0),
    ("1x1", 1, 0, NN, 0), ("1x1", 1, 0, PT, 0),
    # 1 1 . 2 2 2 . . 3: across the one-pixel gap (q - p)^2 = 4, beyond both D = 1 limits (1 and 2) and
    # within both D = 2 limits (4 and 6), for one of 1's two edge pixels; 3 is 3 pixels off: D = 5 only
    ("1x9", 1, 0, NN, 0), ("1x9", 1, 0, PT, 0), ("1x9", 1, 1, NN, 1), ("1x9", 1, 1, PT, 50), ("1x9", 2, 1, NN, 1),
    ("1x9", 3, 1, NN, 0), ("1x9", 3, 2, NN, 1), ("1x9", 2, 2, NN, 2), ("1x9", 2, 2, PT, 100),
    ("9x1", 1, 1, NN, 1), ("9x1", 1, 1, PT, 50), ("9x1", 3, 2, NN, 1),
    # corners: 4 x 4 squares; a corner square's nearest pixel is 10 rows and 10 columns off the middle
    # one's (200 > 25 + 5; 200 <= 225), the other corners 23 off; at D = 15 the limit 240 admits the edge
    # pixels (3, 3), (3, 2), (2, 3) of square 1 (200, 221, 221), not (2, 2) or (3, 1) (242, 244): 3 of 12
    ("corners", 1, 0, NN, 0), ("corners", 5, 0, NN, 0), ("corners", 1, 0, PT, 0),
    ("corners", 1, 1, NN, 1), ("corners", 4, 1, NN, 1), ("corners", 5, 1, NN, 4), ("corners", 1, 1, PT, 25),
    ("side", 1, 0, NN, 1), ("side", 2, 0, NN, 1), ("side", 1, 0, PT, 100 * 4 / 12),
    ("corner_only", 1, 0, NN, 0), ("corner_only", 2, 0, NN, 0), ("corner_only", 1, 0, PT, 100 * 1 / 12),
    ("corner_only", 1, 1, NN, 1),
    ("gap", 1, 0, NN, 0), ("gap", 1, 0, PT, 0), ("gap", 1, 1, NN, 1), ("gap", 2, 1, NN, 1),
    # ring (2) and square (1) share the centre (20, 20): 1 comes first in the table, so 2's rank 1 is 2 itself
    ("ring", 2, 0, FN, 2), ("ring", 2, 0, FD, 0), ("ring", 1, 0, FN, 2), ("ring", 1, 0, FD, 0),
    ("ring", 2, 0, SN, 3), ("ring", 2, 0, AN, 0), ("ring", 1, 0, NN, 1), ("ring", 2, 0, NN, 1),
    ("ring", 1, 0, PT, 100),
    ("grid", 5, 0, NN, 4), ("grid", 5, 1, NN, 8), ("grid", 1, 0, NN, 2), ("grid", 1, 1, NN, 3), ("grid", 5, 0, PT, 100),
    # ties: object 5 at (10, 10) has eight others at distance 5; the lowest table indices win
    ("ties", 5, 0, FN, 1), ("ties", 5, 0, FD, 5), ("ties", 5, 0, SN, 2), ("ties", 5, 0, SD, 5),
    ("labels", 1, 0, NN, 1), ("labels", 7, 0, NN, 1), ("labels", 8, 0, NN, 1), ("labels", 300, 0, NN, 1),
    ("labels", 7, 1, NN, 1),
    ("many", 50, 0, NN, 0), ("many", 50, 1, NN, 100), ("many", 50, 0, PT, 0),
] + [(f"pair_{o[0]}_{o[1]}", 1, 0, NN, v[0]) for o, v in PAIRS.items()] \
  + [(f"pair_{o[0]}_{o[1]}", 1, 0, PT, 100 * v[1]) for o, v in PAIRS.items()] \
  + [(f"size_{k}", L, s, NN, s) for k in SIZE_KINDS for L in (1, 2) for s in (0, 1)]


def check_hand(name, labels, rows):
    """Assert the hand-worked values of scene `name` on (object labels, rows)."""
    n = 0
    for scene, L, s, col, val in HAND:
        if scene != name:
            continue
        k = list(labels).index(L)
        assert rows[k, _c(s, col)] == val, (scene, L, s, col, rows[k, _c(s, col)], val)
        n += 1
    return n
