"""Procedural edge-case scenes for the mask dynamics (cpx_seg_masks, csrc/k_seg.hip: follow rounds,
histogram, seeds, seed expansion, big-mask removal, renumbering), shared by the CPU precondition
test (test_seg_scenes_ref.py) and the GPU test (test_gpu_seg_edges.py).

A scene is (yf [B, 3, Ly, Lx] float32, H, W, geom kwargs, call kwargs): yf holds (dY, dX, cellprob)
per FOV, the geom kwargs go to cpx.segment.make_geom and seg_oracle.compute_masks alike, the call
kwargs (niter, min_size, resample) to both calls.  The direct scenes use diameter 17: rescale is 1,
Ly == H, Lx == W, the bilinear upsample is the identity and yf IS the dynamics field.

`stages` returns the oracle's intermediates of one FOV and restates the few get_masks statements
behind them, with one switch per rule so that a test can compute the deliberately wrong variant;
test_seg_scenes_ref.py asserts on every scene that the unswitched restatement equals
seg_oracle.get_masks.

Plain helper module for tests (no fixtures, not collected).
"""
from __future__ import annotations

import numpy as np
from scipy import ndimage as ndi

import seg_oracle as so
import synth_golden as sg

DIRECT = {"diameter": 17.0}   # rescale 1: the field is given at the dynamics resolution
K0, SW, K1 = 16, 384, 128     # k_seg.hip's follow rounds: k0 steps until step sw, then k1
RPAD = so.RPAD


# ---------------------------------------------------------------------------------------------
# oracle staging
# ---------------------------------------------------------------------------------------------

def stages(yf, H, W, niter=None, resample=True, model="nuclei", diameter=100.0, *, min_moving=5,
           seed_min=11, good_min=3, big_ge=False, earlier_wins=False, first_of_ties=False):
    """The oracle's intermediates of one FOV (yf [3, Ly, Lx]) as a dict:
      n_moving   pixels that follow the flow
      p          final positions [2, Dy, Dx] (so.follow_flows; the start grid when nothing follows)
      h          padded histogram of the final integer positions
      seeds      [(y, x)] in the padded grid, row-major
      m0_counts  pixels per seed label (index k for seed k, label k + 1) before big-mask removal
      n_masks    labels left after big-mask removal
      labels     renumbered label image == so.get_masks (zeros when fewer than 5 pixels follow)
    The keyword-only switches state the rules (a seed is h >= seed_min, the expansion runs through
    h >= good_min, a label is dropped at count > 0.4 n, later seeds win, equal maxima of one 5 x 5
    window are all seeds, fewer than min_moving moving pixels give no masks); other values give the
    deliberately wrong variants."""
    if niter is None:
        niter = so.default_niter(model, diameter, resample)
    f = so.upsample_flows(yf, H, W) if resample else yf
    dP, cp = f[:2], f[2] > so.CELLPROB_THRESHOLD
    Dy, Dx = cp.shape
    dps = (dP * cp / np.float32(5.0)).astype(np.float32)
    n_moving = int((np.abs(dps[0]) > 1e-3).sum())
    out = {"n_moving": n_moving, "niter": niter}
    grid = np.array(np.meshgrid(np.arange(Dy), np.arange(Dx), indexing="ij")).astype(np.float32)
    if n_moving < min_moving or not cp.any():
        z = np.zeros((Dy, Dx), np.int32)
        out.update(p=grid, h=None, seeds=[], m0_counts=np.zeros(0, np.int64), n_masks=0, labels=z)
        return out
    if n_moving < 5:  # (so.follow_flows has the rule built in: follow by its literal loop)
        p = _follow_numpy(dps, niter)
    else:
        p, _ = so.follow_flows(dP, cp, niter)
    # get_masks, restated
    pi = [np.where(cp, p[i], grid[i]).ravel().astype("int32") for i in range(2)]
    shape = (Dy + 2 * RPAD, Dx + 2 * RPAD)
    h = np.zeros(shape, np.int64)
    np.add.at(h, (pi[0] + RPAD, pi[1] + RPAD), 1)
    hmax = ndi.maximum_filter1d(ndi.maximum_filter1d(h, 5, axis=0), 5, axis=1)
    seeds = list(zip(*np.nonzero((h == hmax) & (h >= seed_min))))
    if first_of_ties:
        seeds = [s for i, s in enumerate(seeds)
                 if not any(abs(s[0] - t[0]) <= 2 and abs(s[1] - t[1]) <= 2 for t in seeds[:i])]
    good = h >= good_min
    M = np.zeros(shape, np.int64)
    order = list(enumerate(seeds))
    for k, (sy, sx) in (reversed(order) if earlier_wins else order):
        cur = np.zeros(shape, bool)
        cur[sy, sx] = True
        for _ in range(5):
            cur = ndi.binary_dilation(cur, structure=np.ones((3, 3), bool)) & good
        M[cur] = k + 1
    M0 = M[pi[0] + RPAD, pi[1] + RPAD]
    counts = np.bincount(M0, minlength=len(seeds) + 1)[1:]
    big = Dy * Dx * 0.4
    drop = 1 + np.nonzero((counts >= big) if big_ge else (counts > big))[0]
    M0[np.isin(M0, drop)] = 0
    nz = M0[M0 > 0]
    uniq, first = np.unique(nz, return_index=True)
    remap = np.zeros(len(seeds) + 1, np.int64)
    remap[uniq[np.argsort(first)]] = np.arange(1, len(uniq) + 1)
    out.update(p=p, h=h, seeds=[(int(y), int(x)) for y, x in seeds], m0_counts=counts,
               n_masks=len(uniq), labels=remap[M0].reshape(Dy, Dx).astype(np.int32))
    return out


def _follow_numpy(dps, niter):
    """so.follow_flows' literal loop without its fewer-than-5 rule (for the wrong variants only)."""
    Ly, Lx = dps.shape[1:]
    p = np.array(np.meshgrid(np.arange(Ly), np.arange(Lx), indexing="ij")).astype(np.float32)
    iy, ix = np.nonzero(np.abs(dps[0]) > 1e-3)
    py, px = p[0][iy, ix].copy(), p[1][iy, ix].copy()
    I = dps.astype(np.float64)
    for _ in range(niter):
        yf, xf = py.astype(np.int32), px.astype(np.int32)
        y = (py - yf).astype(np.float32).astype(np.float64)
        x = (px - xf).astype(np.float32).astype(np.float64)
        y0, x0 = np.clip(yf, 0, Ly - 1), np.clip(xf, 0, Lx - 1)
        y1, x1 = np.minimum(Ly - 1, y0 + 1), np.minimum(Lx - 1, x0 + 1)
        d = [(I[c, y0, x0] * (1 - y) * (1 - x) + I[c, y0, x1] * (1 - y) * x +
              I[c, y1, x0] * y * (1 - x) + I[c, y1, x1] * y * x).astype(np.float32) for c in range(2)]
        py = np.clip((py + d[0]).astype(np.float32), np.float32(0), np.float32(Ly - 1))
        px = np.clip((px + d[1]).astype(np.float32), np.float32(0), np.float32(Lx - 1))
    p[0][iy, ix], p[1][iy, ix] = py, px
    return p


def oracle_labels(yf, H, W, flow_threshold, **kw):
    """so.compute_masks of one FOV; kw: a scene's geom and call kwargs."""
    kw = {k: v for k, v in kw.items() if k in ("model", "diameter", "niter", "resample", "min_size")}
    return so.compute_masks(yf, H, W, flow_threshold=flow_threshold, **kw)


def oracle_rows(yf, H, W, **kw):
    """The rows of cpx_seg_stats that the dynamics alone decide, from `stages`: n_moving,
    n_seeds_found (the oracle's seeds) and n_masks (labels left after big-mask removal)."""
    st = stages(yf, H, W, **{k: v for k, v in kw.items() if k in ("model", "diameter", "niter", "resample")})
    return {"n_moving": st["n_moving"], "n_seeds_found": len(st["seeds"]), "n_masks": st["n_masks"]}


# ---------------------------------------------------------------------------------------------
# field builders
# ---------------------------------------------------------------------------------------------

def blank(Dy, Dx):
    yf = np.zeros((3, Dy, Dx), np.float32)
    yf[2] = -1.0
    return yf


def sink_field(Dy, Dx, objs, speed=1.0):
    """objs: [(mask [Dy, Dx] bool, (cy, cx))].  Inside each mask dP = 5 speed (c - pos) / max(|c - pos|, 1)
    (so the followed field dP / 5 is a unit vector times speed, shrinking within one pixel of the
    sink), cellprob +1; outside every mask dP = 0, cellprob -1."""
    yf = blank(Dy, Dx)
    yy, xx = np.meshgrid(np.arange(Dy, dtype=np.float64), np.arange(Dx, dtype=np.float64), indexing="ij")
    for mask, (cy, cx) in objs:
        dy, dx = cy - yy, cx - xx
        nrm = np.maximum(np.hypot(dy, dx), 1.0)
        yf[0][mask] = (5.0 * speed * dy / nrm)[mask]
        yf[1][mask] = (5.0 * speed * dx / nrm)[mask]
        yf[2][mask] = 1.0
    return yf


def box(Dy, Dx, y0, y1, x0, x1):
    """Rows y0..y1 and columns x0..x1, both inclusive."""
    m = np.zeros((Dy, Dx), bool)
    m[y0:y1 + 1, x0:x1 + 1] = True
    return m


def add_column(yf, x, ys, k, down=True, v=1.0):
    """A one-pixel-wide column of k cell pixels next to the sink cell (ys, x), above it (down) or
    below, with dP / 5 == (+-v, 0): at integer x the bilinear weights never mix columns, and with
    v == 1 each pixel reaches the sink cell in as many steps as it is rows away and stops there
    (the sink cell's own field is zero), so h[ys, x] == k + 1."""
    rows = range(ys - k, ys) if down else range(ys + 1, ys + k + 1)
    for y in rows:
        assert yf[2, y, x] < 0, "columns must not overlap"
        yf[0, y, x] = np.float32(5.0 * v) if down else -np.float32(5.0 * v)
        yf[2, y, x] = 1.0
    yf[2, ys, x] = 1.0
    return yf


# ---------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------

BIG_SHAPE = (50, 50)
BIG_SINK = (15, 25)
BIG_RUN = (1049, 1050)  # object pixels in raster order, FOV 0 / FOV 1


def big_boundary():
    """Rows 0.. of a 50 x 50 plane in raster order, 1049 (FOV 0) or 1050 (FOV 1) pixels, flow to the
    sink (15, 25); the sink row's pixels have dy == 0 and do not follow, so 50 drop out and the sink
    cell itself joins: the label counts 1000 = 0.4 n (kept) and 1001 (removed).  A 6 x 6 second
    object lies below it."""
    Dy, Dx = BIG_SHAPE
    fovs = []
    for run in BIG_RUN:
        m = np.zeros(Dy * Dx, bool)
        m[:run] = True
        small = box(Dy, Dx, 34, 39, 20, 25)
        fovs.append(sink_field(Dy, Dx, [(m.reshape(Dy, Dx), BIG_SINK), (small, (36.5, 22.5))]))
    return np.stack(fovs), Dy, Dx, dict(DIRECT), {}


TIE_SHAPE = (41, 61)
TIE_DIST = (1, 2, 3, 5)


def seed_ties():
    """Two mirror-image 13 x 8 blocks (rows 14..26) whose sinks lie on row 20 at distance 1, 2, 3
    and 5 cells: 96 followers + the sink cell = 97 positions each, equal maxima."""
    Dy, Dx = TIE_SHAPE
    fovs = []
    for dist in TIE_DIST:
        gap = dist - 1 if dist % 2 == 0 else 0  # an even distance needs the blocks one column apart
        xa = 29 - (dist - 1 - gap) // 2
        xb = xa + dist
        left, right = box(Dy, Dx, 14, 26, 22, 29), box(Dy, Dx, 14, 26, 30 + gap, 37 + gap)
        assert left[20, xa] and right[20, xb]
        fovs.append(sink_field(Dy, Dx, [(left, (20, xa)), (right, (20, xb))]))
    return np.stack(fovs), Dy, Dx, dict(DIRECT), {}


def tie_sinks(dist):
    gap = dist - 1 if dist % 2 == 0 else 0
    xa = 29 - (dist - 1 - gap) // 2
    return (20, xa), (20, xa + dist)


OVERLAP_SHAPE = (33, 37)
OVERLAP_ROW, OVERLAP_X = 20, 10


def seed_overlap():
    """Seeds A (20, 10) and B (20, 17), both h == 16, joined by six cells of h == 3: either seed's
    geodesic ball of radius 5 ends one cell short of the other seed and the balls share four cells,
    which the later seed (B) keeps.  FOV 1 is the same field turned upside down (columns below the
    sink row, flowing up)."""
    Dy, Dx = OVERLAP_SHAPE
    fovs = []
    for down in (True, False):
        yf = blank(Dy, Dx)
        ys = OVERLAP_ROW if down else Dy - 1 - OVERLAP_ROW
        for i in range(8):
            add_column(yf, OVERLAP_X + i, ys, 15 if i in (0, 7) else 2, down)
        fovs.append(yf)
    return np.stack(fovs), Dy, Dx, dict(DIRECT), {}


THR_SHAPE = (31, 35)   # n % 4 == 1, nh % 4 == 1: the exact counts go through the scalar branches
THR_ROW = 15
THR_NOSEED_X, THR_SEED_X, THR_SEED_MIRROR_X = 5, 20, 11
# FOV 4: ((sink row, sink column), column above the sink, direction of the two h == 3 cells)
THR_EDGE_SEEDS = (((15, 34), True, -1), ((8, 0), False, 1), ((30, 15), True, 1), ((0, 24), False, 1))


def thr_cells(down, mirror=False):
    """FOV 0 / 1: the sink cells (no seed h == 10, seed h == 11, h == 2, h == 3, h == 3) of the
    group around the seed at x = 20, or of its left-right mirror image around x = 11.  The last
    three step away from the seed diagonally: each lies in a row that the seed's own column
    crosses, so in the histogram's rows cells that start at 1 and at 0 (moving pixels) alternate,
    with the moving pixel on either side of a cell of exactly 3."""
    s = -1 if down else 1
    ys, xs, r = (THR_ROW, THR_SEED_MIRROR_X, -1) if mirror else (THR_ROW, THR_SEED_X, 1)
    return (ys, THR_NOSEED_X), (ys, xs), (ys + s, xs - r), (ys + s, xs + r), (ys + 2 * s, xs + 2 * r)


def thresholds():
    """FOV 0: a sink with exactly 10 positions (column of 9, no seed) and one with exactly 11
    (column of 10, a seed); diagonally beside the seed, cells of exactly 2 (outside the expansion)
    and 3 (inside; the second is reached through the first only), and the seed's group once more
    as its mirror image: thr_cells.  FOV 1: the same upside down.  FOV 2: exactly 5 moving pixels.  FOV 3: exactly 4.  FOV 4: four
    seeds of exactly 11 on the plane's border, each with two cells of 3 beside it: the columns run
    along the last and the first plane column (beside them, above the short columns, the field is
    zero: a gather that took the neighbouring column's value would stop the pixels) and into the
    bottom and the top row."""
    Dy, Dx = THR_SHAPE
    fovs = []
    for down in (True, False):
        yf = blank(Dy, Dx)
        for (ys, xs), k in zip(thr_cells(down) + thr_cells(down, mirror=True)[1:], (9, 10, 1, 2, 2, 10, 1, 2, 2)):
            add_column(yf, xs, ys, k, down)
        fovs.append(yf)
    fovs.append(add_column(blank(Dy, Dx), 11, 12, 5))
    fovs.append(add_column(blank(Dy, Dx), 11, 12, 4))
    yf = blank(Dy, Dx)
    for (ys, xs), down, step in THR_EDGE_SEEDS:
        add_column(yf, xs, ys, 10, down)
        add_column(yf, xs + step, ys, 2, down)
        add_column(yf, xs + 2 * step, ys, 2, down)
    fovs.append(yf)
    return np.stack(fovs), Dy, Dx, dict(DIRECT), {}


EDGE_SHAPE = (45, 53)
# (rows, columns, sink): 8 x 8 blocks at the four corners and the four edge midpoints, their sinks
# four pixels outside the plane
EDGE_OBJS = [((0, 7), (0, 7), (-4, -4)), ((0, 7), (45, 52), (-4, 56)),
             ((37, 44), (0, 7), (48, -4)), ((37, 44), (45, 52), (48, 56)),
             ((0, 7), (23, 30), (-4, 26.5)), ((37, 44), (23, 30), (48, 26.5)),
             ((19, 26), (0, 7), (22.5, -4)), ((19, 26), (45, 52), (22.5, 56))]
EDGE_SEEDS = [(0, 0), (0, 52), (44, 0), (44, 52), (0, 26), (44, 26), (22, 0), (22, 52)]


def plane_edges():
    """Eight 64-pixel objects whose sinks lie outside the four corners and the four edges: every
    trajectory is clamped at a plane border and ends on it."""
    Dy, Dx = EDGE_SHAPE
    objs = [(box(Dy, Dx, r[0], r[1], c[0], c[1]), s) for r, c, s in EDGE_OBJS]
    return sink_field(Dy, Dx, objs)[None], Dy, Dx, dict(DIRECT), {}


ROUND_SHAPE = (40, 43)
ROUND_ROW, ROUND_X = 12, 21
ROUND_EDGES = (K0, SW, SW + K1)
ROUND_TIMERS = (15, 16, 17, 383, 384, 385, 511, 512, 513, 1175, 1176)
ROUND_NITER = (1, 15, 16, 17, 383, 384, 385, 511, 512, 513, 1175, 1176)


def round_edges():
    """The sink row 12: a seed at (12, 21) (a column of 12 above it, speed 1) and five cells of
    h == 3 on either side (columns of 2 above them), all inside the seed's expansion from step 12
    on.  Below each of the eleven cells a timer column of 4 pixels (rows 13..16) with dP / 5 ==
    (-3 / (M - 0.5), 0): its fourth pixel has 3 rows to go and enters the sink row, and with it the
    label, exactly at step M.  One timer per M in ROUND_TIMERS; the niter of the call is left to the
    caller (ROUND_NITER)."""
    Dy, Dx = ROUND_SHAPE
    yf = blank(Dy, Dx)
    for i, M in enumerate(ROUND_TIMERS):
        x = ROUND_X - 5 + i
        add_column(yf, x, ROUND_ROW, 12 if x == ROUND_X else 2)
        add_column(yf, x, ROUND_ROW, 4, down=False, v=3.0 / (M - 0.5))
    return yf[None], Dy, Dx, dict(DIRECT), {}


def timer_column(M):
    return ROUND_X - 5 + ROUND_TIMERS.index(M)


MIN_SHAPE = (31, 33)


def min_size_edge():
    """Two columns whose labels are exactly 14 and 15 pixels (13 and 14 followers + the sink cell)."""
    Dy, Dx = MIN_SHAPE
    yf = blank(Dy, Dx)
    add_column(yf, 8, 20, 13)
    add_column(yf, 22, 20, 14)
    return yf[None], Dy, Dx, dict(DIRECT), {}


ODD_SHAPES = ((301, 323), (302, 325), (299, 321))
ODD_SEEDS = {(301, 323): (1, 2), (302, 325): (3, 4), (299, 321): (5, 6)}


def synthetic_yf(Ly, Lx, seed, noise=0.05, rmin=3, rmax=6, n=6):
    """The random blob field of tests/test_gpu_seg.py (_synthetic_yf) at the network resolution."""
    lab = sg.labels(seed, Ly, Lx, n=n, rmin=rmin, rmax=rmax, skip_every=0)
    mu = so.masks_to_flows(lab)
    rng = np.random.default_rng(seed)
    yf = np.zeros((3, Ly, Lx), np.float32)
    yf[0] = 5.0 * mu[0] + noise * rng.standard_normal((Ly, Lx))
    yf[1] = 5.0 * mu[1] + noise * rng.standard_normal((Ly, Lx))
    yf[2] = np.where(lab > 0, 3.0, -3.0) + 0.5 * rng.standard_normal((Ly, Lx))
    return yf


def odd_shapes(H, W, resample=True):
    """The real 1 / 5.88 upsample (default diameter) to a plane whose pixel count and padded
    histogram size are no multiples of 4: two blob FOVs and one without any cell, so FOV 1 and 2
    start on bases that are not 16-byte aligned."""
    Ly, Lx = so.net_size(H, W)
    a, b = ODD_SEEDS[(H, W)]
    yf = np.stack([synthetic_yf(Ly, Lx, a), synthetic_yf(Ly, Lx, b), np.full((3, Ly, Lx), -1.0, np.float32)])
    return yf, H, W, {}, ({} if resample else {"resample": False})


DIRECT_SCENES = {"big_boundary": big_boundary, "seed_ties": seed_ties, "seed_overlap": seed_overlap,
                 "thresholds": thresholds, "plane_edges": plane_edges, "min_size_edge": min_size_edge}
