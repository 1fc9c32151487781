"""numpy restatement of the Neighbors_* block (include/cpx.h): CellProfiler 4's
MeasureObjectNeighbors with an object set measured against itself, in the "Adjacent" and "Within a
specified distance" modes.  Brute force over the explicit offsets of the two disks, object by
object; nothing here is separable, banded or tiled, so it shares no structure with the kernel."""
import numpy as np

N_NEIGHBORS = 7
(NUMBER_OF_NEIGHBORS, PERCENT_TOUCHING, FIRST_NUMBER, FIRST_DISTANCE, SECOND_NUMBER, SECOND_DISTANCE,
 ANGLE) = range(N_NEIGHBORS)


def distance_of(scale) -> int:
    return 1 if isinstance(scale, str) and scale.lower() == "adjacent" else int(scale)


def clean(labels, max_label):
    """The plane with every value outside 1..max_label as background."""
    lab = np.asarray(labels).astype(np.int64)
    return np.where((lab >= 1) & (lab <= max_label), lab, 0)


def disk_offsets(r2: int):
    """All integer (dy, dx) with dy^2 + dx^2 <= r2."""
    m = int(np.floor(np.sqrt(r2)))
    return [(dy, dx) for dy in range(-m, m + 1) for dx in range(-m, m + 1) if dy * dy + dx * dx <= r2]


def edge_mask(lab, L):
    """E_L: pixels of L with an 8-neighbour of another value, the outside of the plane counting as one."""
    H, W = lab.shape
    pad = np.full((H + 2, W + 2), -1, np.int64)
    pad[1:-1, 1:-1] = lab
    diff = np.zeros((H, W), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                diff |= pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] != L
    return (lab == L) & diff


def _labels_near(lab, rr, cc, offsets):
    """[len(rr), len(offsets)] label at (rr + dy, cc + dx), 0 outside the plane."""
    H, W = lab.shape
    out = np.zeros((len(rr), len(offsets)), np.int64)
    for i, (dy, dx) in enumerate(offsets):
        y, x = rr + dy, cc + dx
        ok = (y >= 0) & (y < H) & (x >= 0) & (x < W)
        out[ok, i] = lab[y[ok], x[ok]]
    return out


def touch(lab, L, D):
    """(NumberOfNeighbors, t, |E_L|) of label L at distance D on a cleaned plane."""
    rr, cc = np.nonzero(lab == L)
    near = _labels_near(lab, rr, cc, disk_offsets(D * D))
    n_nb = len(set(np.unique(near).tolist()) - {0, int(L)})
    er, ec = np.nonzero(edge_mask(lab, L))
    near = _labels_near(lab, er, ec, disk_offsets(D * D + D))
    t = int(((near != 0) & (near != L)).any(axis=1).sum())
    return n_nb, t, len(er)


def centres(lab):
    """(labels [n] ascending, centres [n, 2] float64): exact integer sums, one division each."""
    ls = np.unique(lab[lab > 0])
    c = np.zeros((len(ls), 2), np.float64)
    for k, L in enumerate(ls):
        rr, cc = np.nonzero(lab == L)
        c[k] = np.float64(int(rr.sum())) / np.float64(len(rr)), np.float64(int(cc.sum())) / np.float64(len(cc))
    return ls, c


def ranking(c, k):
    """(order, d): every object j ordered by (d(k, j), j) ascending, and the distances."""
    d = np.sqrt((c[k, 0] - c[:, 0]) ** 2 + (c[k, 1] - c[:, 1]) ** 2)
    return sorted(range(len(c)), key=lambda j: (d[j], j)), d


def closest(ls, c):
    """[n, 5]: first number, first distance, second number, second distance, angle."""
    n = len(ls)
    out = np.zeros((n, 5), np.float64)
    for k in range(n):
        order, d = ranking(c, k)
        if n >= 2:
            out[k, 0], out[k, 1] = ls[order[1]], d[order[1]]
        if n >= 3:
            out[k, 2], out[k, 3] = ls[order[2]], d[order[2]]
            v1, v2 = c[order[1]] - c[k], c[order[2]] - c[k]
            out[k, 4] = np.arctan2(abs(v1[1] * v2[0] - v1[0] * v2[1]), v1[0] * v2[0] + v1[1] * v2[1]) * (180.0 / np.pi)
    return out


def neighbors(labels, max_label, scales):
    """(object labels [n], rows [n, 7 * len(scales)]) of one plane."""
    lab = clean(labels, max_label)
    ls, c = centres(lab)
    n = len(ls)
    rows = np.zeros((n, N_NEIGHBORS * len(scales)), np.float64)
    cl = closest(ls, c)
    for s, scale in enumerate(scales):
        D = distance_of(scale)
        for k, L in enumerate(ls):
            n_nb, t, e = touch(lab, L, D)
            rows[k, N_NEIGHBORS * s + NUMBER_OF_NEIGHBORS] = n_nb
            rows[k, N_NEIGHBORS * s + PERCENT_TOUCHING] = np.float64(t * 100) / np.float64(e)
        rows[:, N_NEIGHBORS * s + FIRST_NUMBER:N_NEIGHBORS * (s + 1)] = cl
    return ls, rows
