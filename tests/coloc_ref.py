"""fp64 numpy restatement of the per-object colocalization columns (include/cpx.h, "per-object
colocalization"): per object and per channel pair, boolean masks and .sum().

Test infrastructure only; the product computes these in csrc/k_coloc.hip."""
import itertools

import numpy as np

N_COLOC = 6


def n_colocalization(C: int) -> int:
    return N_COLOC * (C * (C - 1) // 2)


def colocalization(labels: np.ndarray, planes: np.ndarray, threshold: float = 15.0) -> np.ndarray:
    """labels int [H, W]; planes float32 [C, H, W] -> float64 [n_objects, 6 * C (C - 1) / 2], one
    row per present label in ascending order."""
    C = planes.shape[0]
    ids = np.unique(labels[labels > 0])
    out = np.empty((len(ids), n_colocalization(C)), np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k, L in enumerate(ids):
            P = labels == L
            x = [planes[a][P].astype(np.float64) for a in range(C)]
            n = x[0].size
            mean = [xa.sum() / n for xa in x]
            t = [(threshold / 100.0) * xa.max() for xa in x]
            for pi, (a, b) in enumerate(itertools.combinations(range(C), 2)):
                xa, xb = x[a], x[b]
                da, db = xa - mean[a], xb - mean[b]
                ga, gb = xa >= t[a], xb >= t[b]
                S = ga & gb
                sab, saa, sbb = (xa[S] * xb[S]).sum(), (xa[S] * xa[S]).sum(), (xb[S] * xb[S]).sum()
                out[k, 6 * pi:6 * pi + 6] = [
                    np.float64((da * db).sum()) / np.sqrt((da * da).sum() * (db * db).sum()),
                    np.float64(sab) / np.sqrt(saa * sbb),
                    np.float64(xa[S].sum()) / np.float64(xa[ga].sum()),
                    np.float64(xb[S].sum()) / np.float64(xb[gb].sum()),
                    np.float64(sab) / np.float64(saa),
                    np.float64(sab) / np.float64(sbb)]
    return out
