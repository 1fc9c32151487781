"""fp64 numpy restatement of the per-object intensity quantile, edge and location columns
(include/cpx.h, "per-object intensity quantile, edge and location columns"), the
arithmetic of CellProfiler 4's MeasureObjectIntensity: one lexsort by (label, value) for the order
statistics, explicit shifted comparisons for the edge set.

Test infrastructure only; the product computes these in csrc/k_intensity_ext.hip."""
import numpy as np

N_IEXT = 14
(LOWER_QUARTILE, MEDIAN, UPPER_QUARTILE, MAD, INTEGRATED_EDGE, MEAN_EDGE, STD_EDGE, MIN_EDGE, MAX_EDGE,
 MASS_DISPLACEMENT, CENTER_MASS_X, CENTER_MASS_Y, MAX_X, MAX_Y) = range(N_IEXT)
# bit-equal columns (exact selection, exact interpolation weights) / columns that are float64 sums
PICK = (LOWER_QUARTILE, MEDIAN, UPPER_QUARTILE, MAD, MIN_EDGE, MAX_EDGE, MAX_X, MAX_Y)
SUMS = (INTEGRATED_EDGE, MEAN_EDGE, STD_EDGE, CENTER_MASS_X, CENTER_MASS_Y)


def n_intensity_ext(C: int) -> int:
    return N_IEXT * C if C > 0 else 0


def quantile(v: np.ndarray, f: float) -> float:
    """CellProfiler's quantile of an ascending sequence (not numpy.percentile)."""
    n = len(v)
    t = n * f
    i = int(np.floor(t))
    g = t - i
    return v[i] * (1.0 - g) + v[i + 1] * g if i < n - 1 else v[i]


def edge_mask(labels: np.ndarray) -> np.ndarray:
    """Object pixels in the plane's first or last row or column, or with an 8-neighbour of another
    label (background included)."""
    H, W = labels.shape
    e = np.zeros((H, W), bool)
    e[0, :] = e[-1, :] = e[:, 0] = e[:, -1] = True
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            if dr == 0 and dc == 0:
                continue
            # pixel (r, c) against its neighbour (r + dr, c + dc), where both are in the plane
            pr = slice(max(-dr, 0), H - max(dr, 0))
            pc = slice(max(-dc, 0), W - max(dc, 0))
            qr = slice(max(dr, 0), H - max(-dr, 0))
            qc = slice(max(dc, 0), W - max(-dc, 0))
            e[pr, pc] |= labels[pr, pc] != labels[qr, qc]
    return e & (labels > 0)


def intensity_ext(labels: np.ndarray, planes: np.ndarray) -> np.ndarray:
    """labels int [H, W]; planes float32 [C, H, W] -> float64 [n_objects, 14 * C], one row per
    present label in ascending order, column 14 * c + j."""
    C = planes.shape[0]
    rr, cc = np.nonzero(labels > 0)                 # raster order
    lab = labels[rr, cc]
    edge = edge_mask(labels)[rr, cc]
    ids, count = np.unique(lab, return_counts=True)
    by_label = np.argsort(lab, kind="stable")       # raster order within a label
    start = np.concatenate([[0], np.cumsum(count)])
    out = np.empty((len(ids), N_IEXT * C), np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for c in range(C):
            x_all = planes[c][rr, cc].astype(np.float64)
            order = np.lexsort((x_all, lab))        # by label, then by value: NaN last, -0.0 == +0.0
            for k in range(len(ids)):
                sl = slice(start[k], start[k + 1])
                q = out[k, N_IEXT * c:N_IEXT * (c + 1)]
                n = count[k]
                v = x_all[order[sl]]                # ascending
                p = by_label[sl]                    # the object's pixels in raster order
                x, r, col, e = x_all[p], rr[p], cc[p], edge[p]
                q[LOWER_QUARTILE] = quantile(v, 0.25)
                med = quantile(v, 0.5)
                q[MEDIAN] = med
                q[UPPER_QUARTILE] = quantile(v, 0.75)
                q[MAD] = quantile(np.sort(np.abs(x - med)), 0.5)
                xe = x[e]
                ne = xe.size
                mean_e = xe.sum() / ne
                q[INTEGRATED_EDGE] = xe.sum()
                q[MEAN_EDGE] = mean_e
                q[STD_EDGE] = np.sqrt(((xe - mean_e) ** 2).sum() / ne)
                q[MIN_EDGE] = xe.min()
                q[MAX_EDGE] = xe.max()
                cm_y = (r * x).sum() / x.sum()
                cm_x = (col * x).sum() / x.sum()
                q[MASS_DISPLACEMENT] = np.sqrt((r.sum() / n - cm_y) ** 2 + (col.sum() / n - cm_x) ** 2)
                q[CENTER_MASS_X] = cm_x
                q[CENTER_MASS_Y] = cm_y
                first = np.argmax(x)                # first maximum in raster order; a NaN is the largest
                q[MAX_X] = col[first]
                q[MAX_Y] = r[first]
    out[:, [N_IEXT * c + j for c in range(C) for j in PICK]] += 0.0   # a picked -0.0 is written as +0.0
    return out
