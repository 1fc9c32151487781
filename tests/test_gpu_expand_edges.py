"""GPU: cpx_expand_labels (k_expand.hip) bit-identical to skimage's expand_labels (the oracle's
scipy feature transform, cpx_oracle.secondary_objects) across the kernels' own edges: the 64-row
column tiles of k_edt_cols, the 8-row blocks and 256-column segments of k_edt_rows, the LDS stage
sized for distance 127, planes smaller than the distance, the inclusive distance threshold and the
packed (d^2, column) tie key — many-way ties at a rosette's centre resolve to the smallest column,
then the smallest row (scipy's rule, the lexicographic minimum of (d^2, column, row)).
"""
import numpy as np
import pytest
import torch

import cpx_oracle as orc
from cpx._lib import CPX_OK
from cpx.device import _ptr

pytestmark = pytest.mark.gpu

CPX_ERR_ARG = 1              # include/cpx.h
BIG_LABEL = (1 << 23) - 1    # include/cpx.h: label values below 2^23
SEG, COL_TILE = 256, 64      # k_expand.hip: kT (k_edt_rows segment), kColTile (k_edt_cols tile)


def _expand_call(dev, labs, d, cells=True, cyto=True):
    """(rc, cells, cyto) of one call on [B, H, W] labels; outputs start at the sentinel -7, an
    output not asked for is passed as NULL and returned as None."""
    B, H, W = labs.shape
    t = torch.from_numpy(np.ascontiguousarray(labs, np.int32)).to(dev.torch_device)
    tc = torch.full_like(t, -7) if cells else None
    ty = torch.full_like(t, -7) if cyto else None
    rc = dev.lib.cpx_expand_labels(dev.h, _ptr(t), B, H, W, d, _ptr(tc) if cells else None,
                                   _ptr(ty) if cyto else None)
    dev.sync()
    return rc, tc.cpu().numpy() if cells else None, ty.cpu().numpy() if cyto else None


def _check(dev, labs, d, what):
    rc, gc, gy = _expand_call(dev, labs, d)
    assert rc == CPX_OK, (what, rc)
    for b in range(labs.shape[0]):
        rcells, rcyto = orc.secondary_objects(labs[b], d)
        np.testing.assert_array_equal(gc[b], rcells, err_msg=f"{what} fov {b} cells")
        np.testing.assert_array_equal(gy[b], rcyto, err_msg=f"{what} fov {b} cyto")
    return gc, gy


def _labels(rng, n):
    """n label values: 1, BIG_LABEL and random ones with gaps in between."""
    v = rng.integers(2, BIG_LABEL, n).astype(np.int32)
    v[0] = 1
    v[-1] = BIG_LABEL
    return v


def sparse_pixels(H, W, seed):
    """Single labelled pixels, about one per 30 x 30 px (at least two)."""
    rng = np.random.default_rng(seed)
    n = max(2, H * W // 900)
    lab = np.zeros((H, W), np.int32)
    lab[rng.integers(0, H, n), rng.integers(0, W, n)] = _labels(rng, n)
    return lab


def rectangles(H, W, seed):
    """Small rectangles (1..6 px a side, cut at the plane), about one per 40 x 40 px."""
    rng = np.random.default_rng(seed)
    n = max(2, H * W // 1600)
    lab = np.zeros((H, W), np.int32)
    for v in _labels(rng, n):
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        lab[y:y + int(rng.integers(1, 7)), x:x + int(rng.integers(1, 7))] = v
    return lab


def edge_features(H, W, D):
    """Single pixels 1..D columns beyond every 256-column segment edge and 1..D rows beyond every
    64-row tile edge, on both sides, and nothing else: their rows / columns are reached only through
    the halo sweeps of k_edt_cols and the staged window of k_edt_rows.  (A plane without such an
    edge gets its last pixel.)"""
    lab = np.zeros((H, W), np.int32)
    steps = sorted({1, 2, max(1, D // 2), max(1, D - 1), max(1, D)})
    v = 10
    for i, j in enumerate(steps):
        for e in range(SEG, W + D, SEG):          # segment edge between columns e - 1 and e
            for x, y in ((e - 1 + j, (5 * i) % H), (e - j, (5 * i + 2) % H)):
                if 0 <= x < W:
                    lab[y, x] = v
                    v += 3
        for e in range(COL_TILE, H + D, COL_TILE):  # tile edge between rows e - 1 and e
            for y, x in ((e - 1 + j, (37 * i + 3) % W), (e - j, (37 * i + 11) % W)):
                if 0 <= y < H:
                    lab[y, x] = v
                    v += 3
    if not lab.any():
        lab[H - 1, W - 1] = v
    return lab


SHAPES = [(1, 1), (1, 300), (300, 1), (7, 255), (9, 256), (65, 257), (63, 513), (129, 31), (64, 64)]
DISTANCES = (0, 1, 2, 16, 63, 64, 127)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_and_distances(dev, shape):
    """Three FOVs that differ (sparse pixels, rectangles, features just beyond the tile and segment
    edges) at every distance; five of the planes are smaller than 127 px on an axis or both."""
    H, W = shape
    for d in DISTANCES:
        labs = np.stack([sparse_pixels(H, W, 3 * H + W), rectangles(H, W, 5 * H + W), edge_features(H, W, d)])
        gc, gy = _check(dev, labs, d, f"{shape} d {d}")
        if d == 0:
            np.testing.assert_array_equal(gc, labs)
            assert not gy.any()


def test_edge_features_scene():
    """The third FOV really sits beyond the edges: at 65 x 257, D = 16, features in column 256 (one
    past the segment edge) and in row 64 (one past the column tile), and on their near sides."""
    lab = edge_features(65, 257, 16)
    assert lab[:, 256].any() and lab[:, 255].any() and lab[:, 240].any()
    assert lab[64].any() and lab[63].any() and lab[48].any()
    assert len(np.unique(lab)) - 1 == (lab > 0).sum()
    assert (edge_features(1, 1, 127) > 0).sum() == 1


def circle_points(R):
    """The integer points (dy, dx) on the circle of radius R."""
    r = np.arange(-R, R + 1)
    dy, dx = np.meshgrid(r, r, indexing="ij")
    on = dy * dy + dx * dx == R * R
    return dy[on], dx[on]


def rosettes(R, seed):
    """Four FOVs: distinct permuted labels on every integer point of the circle of radius R around
    (cy, cx), cx on either side of the 256-column segment edge and cy on either side of a 64-row
    tile edge.  Returns (labels [4, H, W], centres, winner per FOV by the stated rule)."""
    dy, dx = circle_points(R)
    edge = COL_TILE * -(-R // COL_TILE)  # the first tile edge the circle fits above
    centres = [(cy, cx) for cy in (edge - 1, edge) for cx in (SEG - 1, SEG)]
    H, W = edge + R + 2, SEG + R + 2
    rng = np.random.default_rng(seed)
    labs = np.zeros((4, H, W), np.int32)
    winners = []
    for b, (cy, cx) in enumerate(centres):
        v = rng.permutation(np.arange(1, 3 * len(dy)))[:len(dy)].astype(np.int32)
        labs[b, cy + dy, cx + dx] = v
        first = np.lexsort((dy, dx))[0]  # smallest column, then smallest row
        winners.append(int(v[first]))
    return labs, centres, winners


@pytest.mark.parametrize("R,ways", [(5, 12), (25, 20), (65, 36), (125, 28)])
def test_rosette_ties(dev, R, ways):
    """A `ways`-way tie at the centre: at distance R it takes the label at the smallest column, then
    the smallest row; at R - 1 it stays 0.  Everything else equals the oracle."""
    assert len(circle_points(R)[0]) == ways
    for seed in (0, 1):
        labs, centres, winners = rosettes(R, 10 * R + seed)
        for b, (cy, cx) in enumerate(centres):  # the oracle follows the stated rule
            assert orc.expand_labels(labs[b], R)[cy, cx] == winners[b]
            assert orc.expand_labels(labs[b], R - 1)[cy, cx] == 0
        gc, _ = _check(dev, labs, R, f"rosette {R}")
        assert [int(gc[b][c]) for b, c in enumerate(centres)] == winners
        gc, _ = _check(dev, labs, R - 1, f"rosette {R} at {R - 1}")
        assert all(gc[b][c] == 0 for b, c in enumerate(centres))


@pytest.mark.parametrize("off,D,inside", [((3, 4), 5, True), ((44, 117), 125, True), ((1, 5), 5, False)])
def test_threshold_is_inclusive(dev, off, D, inside):
    """A lone feature reaches a pixel at squared distance exactly D^2 and not D^2 + 1, in all eight
    directions and through the segment and tile edges."""
    fy, fx = COL_TILE * -(-D // COL_TILE) - 2, SEG - 2
    H, W = fy + D + 3, fx + D + 3
    lab = np.zeros((1, H, W), np.int32)
    lab[0, fy, fx] = 77
    gc, _ = _check(dev, lab, D, f"threshold {off} D {D}")
    d2 = off[0] ** 2 + off[1] ** 2
    assert d2 == D * D + (0 if inside else 1)
    for dy, dx in (off, off[::-1]):
        for sy in (-1, 1):
            for sx in (-1, 1):
                assert gc[0, fy + sy * dy, fx + sx * dx] == (77 if inside else 0), (dy, dx, sy, sx)
    assert (gc[0] == 77).sum() > 1


def test_column_ties_take_the_smaller_row(dev):
    """Two features in one column, a pixel halfway: the upper one wins (k_edt_cols keeps the
    feature above on ties), across the 64-row tile edge and for gaps up to 2 x 127."""
    H, W = 330, 40
    gaps = (1, 2, 4, 30, 63, 64, 127)
    lab = np.zeros((len(gaps), H, W), np.int32)  # one pair per FOV
    mids = []
    for i, k in enumerate(gaps):
        x = 3 + 5 * i
        mid = 63 + i % 2 + (128 if k > 63 else 0)  # on either side of a tile edge
        lab[i, mid - k, x], lab[i, mid + k, x] = 100 + i, 200 + i
        mids.append((mid, x))
    for d in (1, 4, 64, 127):
        gc, _ = _check(dev, lab, d, f"column ties d {d}")
        for i, (k, (mid, x)) in enumerate(zip(gaps, mids)):
            assert gc[i, mid, x] == (100 + i if k <= d else 0), (i, k, d)


def test_blank_full_and_label_range(dev):
    H, W = 70, 261
    full = (1 + 5 * (np.arange(H * W, dtype=np.int64) % 1000)).astype(np.int32).reshape(H, W)
    full[0, 0], full[-1, -1] = BIG_LABEL, 1
    big = np.zeros((H, W), np.int32)
    big[3, 3], big[66, 258], big[30, 255], big[30, 256] = BIG_LABEL, 1, BIG_LABEL - 1, 2
    labs = np.stack([np.zeros((H, W), np.int32), full, big])
    for d in (0, 5, 127):
        gc, gy = _check(dev, labs, d, f"blank / full / range d {d}")
        assert not gc[0].any() and not gy[0].any()
        np.testing.assert_array_equal(gc[1], full)
        assert not gy[1].any()
        assert (gc != -7).all() and (gy != -7).all()
    assert set(np.unique(gc[2])) - {0} == {1, 2, BIG_LABEL - 1, BIG_LABEL}


def test_null_outputs_and_arguments(dev):
    """Either output may be NULL, both may not; distances outside 0..127 are CPX_ERR_ARG before any
    launch, and the next call is right."""
    labs = np.stack([rectangles(65, 257, 1), sparse_pixels(65, 257, 2)])
    ref = [orc.secondary_objects(labs[b], 16) for b in range(2)]
    rc, gc, gy = _expand_call(dev, labs, 16, cyto=False)
    assert rc == CPX_OK and gy is None
    np.testing.assert_array_equal(gc, np.stack([r[0] for r in ref]))
    rc, gc, gy = _expand_call(dev, labs, 16, cells=False)
    assert rc == CPX_OK and gc is None
    np.testing.assert_array_equal(gy, np.stack([r[1] for r in ref]))
    assert _expand_call(dev, labs, 16, cells=False, cyto=False)[0] == CPX_ERR_ARG
    _check(dev, labs, 16, "after both NULL")
    for d in (-1, 128):
        rc, gc, gy = _expand_call(dev, labs, d)
        assert rc == CPX_ERR_ARG, (d, rc)
        assert (gc == -7).all() and (gy == -7).all()
        _check(dev, labs, 16, f"after distance {d}")
