"""Procedural edge-case scenes for the Cells watershed (k_watershed.hip) and its expand_labels
footprint (k_expand.hip), shared by the CPU precondition test (test_ws_scenes_ref.py) and the GPU
tests (test_gpu_watershed_edges.py).  A scene is (nuclei [H, W] int32, corr [H, W] float32,
distance); `batch_mixed` stacks five of one shape.

Plain helper module for tests (no fixtures, not collected).
"""
from __future__ import annotations

import numpy as np

import cpx_oracle as orc
import ws_oracle as wo

TILE = 32                    # k_watershed.hip's tile edge (ws_levels.h kT)
BIG_LABEL = (1 << 23) - 1    # the largest label the packed expand pass carries
SUBNORMAL = np.float32(1e-40)
# the serpentines run with the API's cap of 64 relax rounds: (H, W, pitch, seed)
ROUND_SCENES = {"pitch4": (96, 96, 4, 1), "pitch8": (96, 96, 8, 1)}
BATCH_SHAPES = ((64, 96), (33, 33))  # batch_mixed: 6 and 4 tiles per FOV
SPECIAL_SEED = 6  # special_values at 70 x 100: every class of special value decides labels
SPECIAL = np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, 0.5, 0.99, 1.0, 65534.99, 65535.0, 1e9,
                    SUBNORMAL, 1000.0, 2000.0], np.float32)


def same_value(a, v):
    """Elementwise `a is the float32 value v`, telling NaN, -0.0 and 0.0 apart (bit patterns)."""
    return np.asarray(a, np.float32).view(np.uint32) == np.float32(v).view(np.uint32)


def _rect_nuclei(rng, H, W, lo=2, hi=7):
    """lo..hi small rectangular nuclei (1..3 px a side, cut at the plane), later ones on top."""
    nuc = np.zeros((H, W), np.int32)
    for lab in range(1, int(rng.integers(lo, hi + 1)) + 1):
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        nuc[y:y + int(rng.integers(1, 4)), x:x + int(rng.integers(1, 4))] = lab
    return nuc


def heavy_ties(H, W, seed):
    """Few nuclei on five finite 16-bit levels: nearly every flood decision is a raster-index tie."""
    rng = np.random.default_rng(seed)
    corr = rng.integers(0, 5, (H, W)).astype(np.float32) * 1000
    return _rect_nuclei(rng, H, W), corr


def special_values(H, W, seed, distance=15):
    """The heavy-tie scene with every elevation drawn from SPECIAL (NaN, +-inf, negative, -0.0,
    fractions, the 65535 clamp from both sides, a subnormal, two plain levels)."""
    rng = np.random.default_rng(seed)
    corr = SPECIAL[rng.integers(0, len(SPECIAL), (H, W))]
    return _rect_nuclei(rng, H, W, 4, 7), corr, distance


def serpentine(H, W, pitch, seed):
    """Dim random walls (100..5000) and one bright random corridor (50000..60000) along every
    `pitch`-th row, joined alternately at the right and left ends: the flood has to follow the
    corridor through every tile it crosses, one tile per relax round.  Marker 7 at the corridor's
    start, marker 3 at its end, BIG_LABEL at the plane centre when that is a wall pixel; distance
    127 (the footprint is the whole plane for the shapes used)."""
    rng = np.random.default_rng(seed)
    corr = rng.integers(100, 5001, (H, W)).astype(np.float32)
    bright = rng.integers(50000, 60001, (H, W)).astype(np.float32)
    cor = np.zeros((H, W), bool)
    rows = list(range(0, H, pitch))
    for k, y in enumerate(rows):
        cor[y] = True
        if k + 1 < len(rows):
            cor[y:rows[k + 1], W - 1 if k % 2 == 0 else 0] = True
    corr[cor] = bright[cor]
    nuc = np.zeros((H, W), np.int32)
    nuc[0, 0] = 7
    nuc[rows[-1], W - 1 if (len(rows) - 1) % 2 == 0 else 0] = 3
    if not cor[H // 2, W // 2]:
        nuc[H // 2, W // 2] = BIG_LABEL
    return nuc, corr, 127


ONE_WAY = ("up", "down", "left", "right")


def one_way(direction, seed=0):
    """One row or column of four tiles (97 x 20 or 20 x 97) with two touching 1-pixel markers in
    the middle of one end: the flood can only travel in `direction`, so each tile is woken by one
    kind of neighbour flag alone.  Heavy-tie elevations, distance 127 (the footprint is the plane)."""
    rng = np.random.default_rng(seed)
    nuc = np.zeros((97, 20), np.int32)
    nuc[0, 9], nuc[0, 10] = 1, 2          # "down"
    if direction in ("up", "left"):
        nuc = nuc[::-1]
    if direction in ("left", "right"):
        nuc = nuc.T
    nuc = np.ascontiguousarray(nuc)
    return nuc, rng.integers(0, 5, nuc.shape).astype(np.float32) * 1000, 127


def plateau(H, W):
    """Constant elevation: the keys differ by the raster index alone.  Two 1-pixel markers in
    opposite corners, distance 127."""
    nuc = np.zeros((H, W), np.int32)
    nuc[0, 0] = 1
    nuc[H - 1, W - 1] = 2
    return nuc, np.full((H, W), 1000.0, np.float32), 127


def dense_lattice():
    """One 32 x 32 tile with the most seeds it can have: markers where (x + 2y) % 5 == 0 (205 of
    them, distinct labels), so every free pixel off the plane's border touches a marker (794 of the
    819; the other 25 lie on the border, within 2 px of one) and is improved when the round-0 queue
    is seeded.  Marker intensities fall in raster order, the free pixels are heavy ties; distance 2
    (the footprint is the plane)."""
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:TILE, 0:TILE]
    mark = (xx + 2 * yy) % 5 == 0
    n = int(mark.sum())
    nuc = np.zeros((TILE, TILE), np.int32)
    nuc[mark] = rng.permutation(np.arange(1, 2 * n + 1))[:n]
    corr = rng.integers(0, 5, (TILE, TILE)).astype(np.float32) * 1000
    corr[mark] = 60000.0 - 40.0 * np.arange(n, dtype=np.float32)
    return nuc, corr, 2


def all_nuclei(H, W):
    """Every pixel a nucleus: 5 x 7 blocks of several labels with gaps in the numbering."""
    yy, xx = np.mgrid[0:H, 0:W]
    return (1 + 3 * ((yy // 5) * ((W + 6) // 7) + xx // 7)).astype(np.int32)


def batch_mixed(H, W):
    """B = 5 FOVs of one shape at distance 127: a serpentine, a blank FOV, an all-nuclei FOV, a
    special_values FOV, the serpentine turned by 180 degrees.  In tile order the last tile of a FOV
    is followed by the first tile of the next: they must not exchange halos or flags."""
    n0, c0, d = serpentine(H, W, 3, 21)  # pitch 3: the centre is a wall pixel and holds BIG_LABEL
    n3, c3, _ = special_values(H, W, 22, d)
    noise = np.random.default_rng(23).integers(0, 5, (2, H, W)).astype(np.float32) * 1000
    nuc = np.stack([n0, np.zeros_like(n0), all_nuclei(H, W), n3, n0[::-1, ::-1]])
    corr = np.stack([c0, noise[0], noise[1], c3, c0[::-1, ::-1]])
    return np.ascontiguousarray(nuc), np.ascontiguousarray(corr), d


def jacobi_tile_rounds(nuclei, corr, distance, return_levels=False):
    """Rounds of the Jacobi tile model of k_ws_relax, the confirming round included: in each round
    every 32 x 32 tile relaxes B(p) = max(key(p), min_n B(n)) to its fixed point against its
    neighbours' levels of the previous round.  The kernel's halos are at least as fresh, so this is
    an upper bound of the relax rounds it needs."""
    H, W = nuclei.shape
    INF = np.uint64(0xFFFFFFFFFFFFFFFF)
    foot = orc.expand_labels(nuclei, distance) > 0
    key = wo.elevation_key(corr)
    free = foot & (nuclei == 0)
    L = np.where(nuclei > 0, key, INF).astype(np.uint64)
    rounds = 0
    while True:
        old = L.copy()
        while True:  # all tiles at once: a step across a tile edge reads the previous round
            before = L.copy()
            for axis, rev in ((1, False), (1, True), (0, False), (0, True)):
                n = L.shape[axis]
                for i in (range(n - 2, -1, -1) if rev else range(1, n)):
                    j = i + 1 if rev else i - 1
                    src = old if i // TILE != j // TILE else L
                    if axis == 1:
                        cur, prv, k, f = L[:, i], src[:, j], key[:, i], free[:, i]
                    else:
                        cur, prv, k, f = L[i], src[j], key[i], free[i]
                    nv = np.maximum(k, np.minimum(cur, prv))
                    cur[f] = nv[f]
            if np.array_equal(before, L):
                break
        rounds += 1
        if np.array_equal(old, L):
            break
    return (rounds, L) if return_levels else rounds
