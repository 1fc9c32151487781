"""Procedural scenes for the step loop of the flow follower (csrc/k_seg.hip, k_dyn_follow: two
trajectories per thread, items i and i + 256 of a block's 512; the gathers of a step are skipped
while a trajectory stays in its cell; paired 16-byte gathers with a right-edge form), shared by the
CPU precondition test (test_follow_scenes_ref.py) and the GPU test (test_gpu_follow_pairs.py).

Scenes have the form of tests/seg_scenes.py: (yf [B, 3, Dy, Dx], H, W, geom kwargs, call kwargs),
all at diameter 17 (the field is the dynamics field, 200 steps).  Every plane has at most 2048
pixels: k_dyn_prep compacts the moving pixels of one block of 2048 in raster order, so item i of the
first round is the i-th moving pixel in raster order and thread t of block b follows items
512 b + t and 512 b + 256 + t.

`follow` restates seg_oracle.follow_flows step by step, keeps every position and the taps of each
item's last gather, and has one switch per rule so that a test can compute the deliberately wrong
variant.

Plain helper module for tests (no fixtures, not collected).
"""
from __future__ import annotations

import numpy as np

import seg_oracle as so
from seg_scenes import DIRECT, add_column, blank, box, sink_field

NITER = 200   # so.default_niter(diameter=17.0)
PAIR = 256    # items i and i + PAIR of a block's 2 * PAIR share a thread


# ---------------------------------------------------------------------------------------------
# the follower, restated with history
# ---------------------------------------------------------------------------------------------

def dynamics_field(yf):
    return (yf[:2] * (yf[2] > so.CELLPROB_THRESHOLD) / np.float32(5.0)).astype(np.float32)


def partner(i, n):
    """The item that shares a thread with item i in the first round (None: none does)."""
    j = i + PAIR if i % (2 * PAIR) < PAIR else i - PAIR
    return j if 0 <= j < n else None


def follow(yf, niter=NITER, *, key="cell", couple=False, skip=(), right_tap_left=False):
    """Positions of every moving pixel (raster order == item order) after each step.

    Returns a dict: iy, ix (start pixels), pos [niter + 1, 2, N] float32, gathered [niter, N] bool
    (the step's cell differs from the cell of the item's last gather), literal [niter, N] bool
    (py < 1 or px < 1 at the step), stopped [N] (first step whose update left the position
    unchanged; niter when none did), p [2, Dy, Dx] the final positions on the pixel grid.

    Switches (the wrong variants): key "x" / "y" gathers again only when that coordinate of the
    cell changes and otherwise works on the taps it has; couple stops an item's first-round
    partner with it; skip: items that are never followed; right_tap_left takes the value of
    x0 - 1 for the tap x0 on the last column."""
    dps = dynamics_field(yf)
    Dy, Dx = dps.shape[1:]
    iy, ix = np.nonzero(np.abs(dps[0]) > 1e-3)
    N = iy.size
    py, px = iy.astype(np.float32), ix.astype(np.float32)
    I = dps.astype(np.float64)
    pos = np.empty((niter + 1, 2, N), np.float32)
    pos[0] = py, px
    gathered = np.zeros((niter, N), bool)
    literal = np.zeros((niter, N), bool)
    stopped = np.full(N, niter)
    frozen = np.zeros(N, bool)
    frozen[list(skip)] = True
    last = np.full(N, -1, np.int64)
    prev_cell = np.full(N, -1, np.int64)
    taps = np.zeros((4, 2, N))
    for s in range(niter):
        yi, xi = py.astype(np.int32), px.astype(np.int32)
        y = (py - yi).astype(np.float32).astype(np.float64)
        x = (px - xi).astype(np.float32).astype(np.float64)
        y0, x0 = np.clip(yi, 0, Dy - 1), np.clip(xi, 0, Dx - 1)
        y1, x1 = np.minimum(Dy - 1, y0 + 1), np.minimum(Dx - 1, x0 + 1)
        cell = y0.astype(np.int64) * Dx + x0
        k = {"cell": cell, "x": x0.astype(np.int64), "y": y0.astype(np.int64)}[key]
        new = k != last
        gathered[s] = cell != prev_cell
        prev_cell = cell
        literal[s] = (py < 1) | (px < 1)
        xa = np.where(right_tap_left & (x0 == Dx - 1) & (x0 > 0), x0 - 1, x0)
        fresh = np.stack([I[:, y0, xa], I[:, y0, x1], I[:, y1, xa], I[:, y1, x1]])
        taps[..., new] = fresh[..., new]
        last = k
        a, b, c, e = taps
        d = [(a[i] * (1 - y) * (1 - x) + b[i] * (1 - y) * x + c[i] * y * (1 - x) + e[i] * y * x).astype(np.float32)
             for i in range(2)]
        ny = np.clip((py + d[0]).astype(np.float32), np.float32(0), np.float32(Dy - 1))
        nx = np.clip((px + d[1]).astype(np.float32), np.float32(0), np.float32(Dx - 1))
        same = (ny == py) & (nx == px)
        newly = same & ~frozen & (stopped == niter)
        stopped[newly] = s
        if couple:
            for i in np.nonzero(newly)[0]:
                j = partner(int(i), N)
                if j is not None:
                    frozen[j] = True
        py, px = np.where(frozen, py, ny), np.where(frozen, px, nx)
        pos[s + 1] = py, px
    p = np.array(np.meshgrid(np.arange(Dy), np.arange(Dx), indexing="ij")).astype(np.float32)
    p[0][iy, ix], p[1][iy, ix] = py, px
    return {"iy": iy, "ix": ix, "pos": pos, "gathered": gathered, "literal": literal, "stopped": stopped, "p": p}


def labels_of(yf, p):
    """get_masks on positions p (the label image before the flow-error filter and min_size)."""
    return so.get_masks(p, yf[2] > so.CELLPROB_THRESHOLD)


# ---------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------

COUNT_SHAPE = (26, 27)
COUNTS = (256, 257, 512, 513)
COUNT_BAND = 4  # rows per object


def pair_counts(N):
    """The first N pixels of a 26 x 27 plane in raster order follow the flow, in bands of four rows
    (108 pixels, under 40 % of the plane) that each flow to a sink in column 3 (inside every band,
    also a partial one); the sinks lie between two rows, so every one of the N pixels has dy != 0
    and moves.  N == 256: no thread has
    a second item; 257: one thread has one; 512 / 513: the same for the second block."""
    Dy, Dx = COUNT_SHAPE
    run = np.zeros(Dy * Dx, bool)
    run[:N] = True
    run = run.reshape(Dy, Dx)
    objs = []
    for r in range(0, Dy, COUNT_BAND):
        m = run & box(Dy, Dx, r, min(Dy, r + COUNT_BAND) - 1, 0, Dx - 1)
        if m.any():
            objs.append((m, (r + 1.5, 3.0)))
    return sink_field(Dy, Dx, objs)[None], Dy, Dx, dict(DIRECT), {}


PARTNER_SHAPE = (40, 40)
# rows of the parts of FOV 0 (FOV 1 swaps SLOW and FAST)
P_TOP, P_STEP1_ROW, P_SLOW, P_FAST = (0, 5), 6, (8, 19), (22, 33)
P_SLOW_SPEED, P_TOP_SPEED = 0.04, 0.1


def partners():
    """A 40 x 40 plane whose moving pixels come, in raster order, as:
      TOP    rows 0..5 (240 items), speed 0.1 towards (0.5, 20): row 0 and, later, the rows that
             have arrived above y == 1 take the literal top / left expression; 200 steps of motion
      STEP1  row 6 (40 items), dP / 5 == (1, 0) into the zero field of row 7: each is on its exact
             fixed point after step 1
      SLOW   12 rows (478 items: two pixels far from the sink have |dy| <= 1e-3), speed 0.04: up to
             25 steps in one cell, never arrives
      FAST   12 rows (480 items), speed 1: a new cell at nearly every step until it arrives
    so that the threads of the first round pair TOP with STEP1 and SLOW (block 0) and SLOW with
    FAST (block 1).  FOV 1 swaps SLOW and FAST: FAST is the first of a pair there."""
    Dy, Dx = PARTNER_SHAPE
    fovs = []
    for swap in (False, True):
        slow, fast = (P_FAST, P_SLOW) if swap else (P_SLOW, P_FAST)
        yf = sink_field(Dy, Dx, [(box(Dy, Dx, *P_TOP, 0, Dx - 1), (0.5, 20.0))], speed=P_TOP_SPEED)
        # (the parts do not overlap: adding a part's field minus the blank plane places it)
        for rows, speed in ((slow, P_SLOW_SPEED), (fast, 1.0)):
            part = [(box(Dy, Dx, *rows, 0, Dx - 1), ((rows[0] + rows[1]) / 2, 20.0))]
            yf += sink_field(Dy, Dx, part, speed=speed) - blank(Dy, Dx)
        for x in range(Dx):
            add_column(yf, x, P_STEP1_ROW + 1, 1)
        fovs.append(yf)
    return np.stack(fovs), Dy, Dx, dict(DIRECT), {}


RETURN_SHAPE = (31, 35)
RETURN_CENTRE = (15, 17)   # a pixel corner: the four cells around it are visited turn by turn
RETURN_OMEGA, RETURN_KAPPA, RETURN_R = 0.08, 0.02, 6


def returning():
    """A slow inward spiral around the pixel corner (15, 17): dP / 5 == omega J (pos - c) -
    kappa (pos - c) inside radius 6.  A trajectory takes about 78 steps per turn and so leaves each
    cell it crosses and comes back to the cells near the centre a turn later."""
    Dy, Dx = RETURN_SHAPE
    yf = blank(Dy, Dx)
    yy, xx = np.meshgrid(np.arange(Dy, dtype=np.float64), np.arange(Dx, dtype=np.float64), indexing="ij")
    ry, rx = yy - RETURN_CENTRE[0], xx - RETURN_CENTRE[1]
    m = np.hypot(ry, rx) <= RETURN_R
    yf[0][m] = (5.0 * (-RETURN_OMEGA * rx - RETURN_KAPPA * ry))[m]
    yf[1][m] = (5.0 * (RETURN_OMEGA * ry - RETURN_KAPPA * rx))[m]
    yf[2][m] = 1.0
    return yf[None], Dy, Dx, dict(DIRECT), {}


EDGE_DY = 31
EDGE_DX = (2, 34, 35)
EDGE_COL = 14  # followers per column: 15-pixel labels


def buffer_edges(Dx, nan_beside=False):
    """Columns of 14 followers that end (a) on the last column in row 15, (b) on the plane's last
    pixel, both running down the last column, and (c) for Dx > 2 on the last row in the middle
    column.  Beside the last column the field is zero, or with nan_beside NaN (cellprob -1: those
    pixels do not move): the tap that the oracle clamps to the last column must not come
    from there, not even with a weight of zero.  FOV 1 is a plain second plane (one column in the
    middle) to stand before or after FOV 0 in a batch."""
    Dy = EDGE_DY
    yf = blank(Dy, Dx)
    add_column(yf, Dx - 1, 15, EDGE_COL)            # rows 1..14 -> (15, Dx - 1)
    add_column(yf, Dx - 1, Dy - 1, EDGE_COL)        # rows 16..29 -> (30, Dx - 1), the last pixel
    if Dx > 2:  # (on a plane of two columns the two bottom labels would merge and exceed 40 %)
        add_column(yf, Dx // 2, Dy - 1, EDGE_COL)
    if nan_beside:
        assert Dx >= 3
        yf[0, :, Dx - 2] = np.nan
        yf[1, :, Dx - 2] = np.nan
    other = add_column(blank(Dy, Dx), 0, 20, EDGE_COL)
    return np.stack([yf, other]), Dy, Dx, dict(DIRECT), {}


SCALAR_SHAPE = (40, 1)


def scalar_path():
    """Dx == 1: the plain-load kernel k_dyn_follow<2, false>.  Two columns, one flowing down and
    one up."""
    Dy, Dx = SCALAR_SHAPE
    yf = blank(Dy, Dx)
    add_column(yf, 0, 16, EDGE_COL)
    add_column(yf, 0, 20, EDGE_COL, down=False)
    return yf[None], Dy, Dx, dict(DIRECT), {}


SCENES = {"partners": partners, "returning": returning, "scalar_path": scalar_path}
for _n in COUNTS:
    SCENES[f"pair_counts_{_n}"] = (lambda n: lambda: pair_counts(n))(_n)
for _dx in EDGE_DX:
    SCENES[f"buffer_edges_{_dx}"] = (lambda dx: lambda: buffer_edges(dx))(_dx)
SCENES["buffer_edges_nan_34"] = lambda: buffer_edges(34, nan_beside=True)
SCENES["buffer_edges_nan_35"] = lambda: buffer_edges(35, nan_beside=True)
