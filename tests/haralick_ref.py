"""fp64 numpy restatement of the opt-in Haralick texture columns (include/cpx.h, "the Haralick
texture columns the Texture_* block lacks").  The count matrix N is the one the
existing Texture_* columns are computed from: cpx_oracle.glcm of cpx_oracle.texture_input, called
here and not restated, so the block stays tied to the golden-pinned matrix.

Test infrastructure only; the product computes these in csrc/k_haralick.hip."""
import math

import numpy as np
from scipy import ndimage as ndi

import cpx_oracle as orc

N_HAR = 9
(VARIANCE, SUM_AVERAGE, SUM_VARIANCE, SUM_ENTROPY, ENTROPY, DIFFERENCE_VARIANCE, DIFFERENCE_ENTROPY,
 INFO_MEAS1, INFO_MEAS2) = range(N_HAR)
LEVELS = 256


def n_texture_haralick(C: int) -> int:
    return 4 * N_HAR * C if C > 0 else 0


def entropy(q: np.ndarray) -> float:
    """H(q) = -sum_{q > 0} q log2 q, +0.0 for an all-zero or one-bin vector."""
    q = np.asarray(q, np.float64).ravel()
    q = q[q > 0]
    return float(-np.sum(q * np.log2(q)) + 0.0)


def marginals(N: np.ndarray):
    """(px, py, psum[511], pdiff[256], p) of the count matrix N (T = sum N > 0); p = the non-zero
    entries of P = N / T (the zero entries add nothing to any sum).  The marginal counts are
    summed as integers and divided by T once, so a one-bin marginal is exactly 1.0."""
    n = N.shape[0]
    T = float(N.sum())
    i, j = np.nonzero(N)
    c = N[i, j].astype(np.int64)

    def hist(idx, size):
        h = np.zeros(size, np.int64)
        np.add.at(h, idx, c)
        return h / T

    return hist(i, n), hist(j, n), hist(i + j, 2 * n - 1), hist(np.abs(i - j), n), c / T


def from_counts(N: np.ndarray):
    """The nine columns of one count matrix and its entropies (HX, HY, HXY)."""
    if N.sum() == 0:
        return [0.0] * N_HAR, (0.0, 0.0, 0.0)
    px, py, psum, pdiff, P = marginals(N)
    lv = np.arange(len(px), dtype=np.float64)
    ks = np.arange(len(psum), dtype=np.float64)
    mux = float(np.sum(lv * px))
    sav = float(np.sum(ks * psum))
    mud = float(np.sum(lv * pdiff))
    hx, hy, hxy = entropy(px), entropy(py), entropy(P)
    hmax = max(hx, hy)
    row = [0.0] * N_HAR
    row[VARIANCE] = float(np.sum((lv - mux) ** 2 * px))
    row[SUM_AVERAGE] = sav
    row[SUM_VARIANCE] = float(np.sum((ks - sav) ** 2 * psum))
    row[SUM_ENTROPY] = entropy(psum)
    row[ENTROPY] = hxy
    row[DIFFERENCE_VARIANCE] = float(np.sum((lv - mud) ** 2 * pdiff))
    row[DIFFERENCE_ENTROPY] = entropy(pdiff)
    row[INFO_MEAS1] = (hxy - hx - hy) / hmax if hmax > 0 else 0.0
    row[INFO_MEAS2] = math.sqrt(max(0.0, 1.0 - math.exp(-2.0 * (hx + hy - hxy))))
    return row, (hx, hy, hxy)


def count_matrices(labels: np.ndarray, plane32: np.ndarray):
    """Per present label in ascending order the four count matrices [4, 256, 256] of one channel."""
    out = []
    for i, sl in enumerate(ndi.find_objects(labels)):
        if sl is None:
            continue
        q8 = orc.texture_input(plane32, labels, sl, i + 1)
        out.append(np.stack([orc.glcm(q8, 3, d * math.pi / 4) for d in range(4)]))
    return out


def haralick(labels: np.ndarray, planes: np.ndarray):
    """labels int [H, W]; planes float32 [C, H, W] -> (rows float64 [n_objects, 36 * C], column
    (c * 4 + d) * 9 + j, one row per present label in ascending order; entropies float64
    [n_objects, C, 4, 3] = (HX, HY, HXY) of every matrix)."""
    C = planes.shape[0]
    per_ch = [count_matrices(labels, planes[c]) for c in range(C)]
    n = len(per_ch[0])
    rows = np.zeros((n, 4 * N_HAR * C), np.float64)
    ent = np.zeros((n, C, 4, 3), np.float64)
    for c in range(C):
        for k in range(n):
            for d in range(4):
                r, e = from_counts(per_ch[c][k][d])
                rows[k, (c * 4 + d) * N_HAR:(c * 4 + d + 1) * N_HAR] = r
                ent[k, c, d] = e
    return rows, ent
