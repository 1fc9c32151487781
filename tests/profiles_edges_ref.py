"""Edge-case input tables for the profile kernels (csrc/k_profiles.hip) and their references,
written directly from pandas / scipy / exact rationals (tests/test_gpu_profiles_edges.py).

Every table has mixed magnitudes (normal * {1e-3, 1, 1e5}, so that a dropped, duplicated or
reordered row changes the last bits of a Kahan sum), about 3 % NaN and a fixed seed, and is built
once (lru_cache).  Test infrastructure only."""
import math
from fractions import Fraction
from functools import lru_cache
from types import SimpleNamespace as NS

import numpy as np

MAD_SCALE = 1 / 1.4826
DBL_MAX = np.finfo(np.float64).max


def mixed(rng, shape, nan=0.03):
    X = rng.normal(size=shape) * rng.choice([1e-3, 1.0, 1e5], size=shape)
    if nan:
        X[rng.random(shape) < nan] = np.nan
    return X


def order_offs(group, G):
    """Rows sorted by group (stable: original row order inside a group) and group offsets."""
    order = np.argsort(group, kind="stable").astype(np.int32)
    offs = np.zeros(G + 1, dtype=np.int32)
    np.cumsum(np.bincount(group, minlength=G), out=offs[1:])
    return order, offs


def _interleaved_groups(rng, counts):
    group = np.repeat(np.arange(len(counts)), counts)
    return group[rng.permutation(len(group))]


# ------------------------------------------------------------------------------- group mean
MEAN_COUNTS = [0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 200, 2]
MEAN_KS = [1, 63, 64, 65, 130]


@lru_cache(maxsize=None)
def mean_table():
    """16 groups at the edges of the 32-row chunks and the 64-row double buffer, rows interleaved,
    130 columns.  Special cells sit in column 0 (present for every K) and column 64 (the second
    column block): all NaN, +inf, +inf then -inf, -inf only."""
    rng = np.random.default_rng(101)
    group = _interleaved_groups(rng, MEAN_COUNTS)
    X = mixed(rng, (len(group), max(MEAN_KS)))
    for col in (0, 64):
        rows = {g: np.nonzero(group == g)[0] for g in (5, 7, 9, 11)}
        X[rows[5], col] = np.nan
        X[rows[7][40], col] = np.inf
        X[rows[9][3], col], X[rows[9][70], col] = np.inf, -np.inf
        X[rows[11][100], col] = -np.inf
    row_scale = rng.choice([9 / 7, 3.0, 1.0], size=len(group))
    col_scaled = (rng.random(X.shape[1]) < 0.5).astype(np.uint8)
    col_scaled[:2] = (1, 0)
    # streaming splits: s1 has exactly 64 rows of group 7 before it (a multiple of the chunk),
    # s2 falls in the middle of every larger group
    s1 = int(np.nonzero(group == 7)[0][64])
    s2 = int(np.nonzero(group == 14)[0][150])
    return NS(X=X, group=group, G=len(MEAN_COUNTS), row_scale=row_scale, col_scaled=col_scaled,
              splits=sorted((s1, s2)))


def pandas_group_mean(X, group, G):
    """(mean [G, K], nobs [G, K]) of pandas' groupby; absent groups: NaN and 0."""
    import pandas as pd
    gb = pd.DataFrame(X).groupby(group)
    idx = np.arange(G)
    return (gb.mean().reindex(idx).to_numpy(),
            gb.count().reindex(idx, fill_value=0).to_numpy(dtype=np.int64))


def scaled(X, row_scale, col_scaled):
    """The table pandas would reduce after multiplying the scaled columns by the row scale."""
    Xs = X.copy()
    c = np.nonzero(col_scaled[:X.shape[1]])[0]
    Xs[:, c] = Xs[:, c] * row_scale[:, None]
    return Xs


# ----------------------------------------------------------------------------- group median
MEDIAN_COUNTS = {"small": [1, 2, 3, 255, 256, 257, 511, 512, 513, 1025, 4097],
                 "large": [8192, 8193, 16384]}


@lru_cache(maxsize=None)
def median_table(size, with_nan):
    """Group sizes around the sort's powers of two.  Column 0: mixed, with a +inf, a -inf and a
    majority of +inf in three groups; column 1: rounded (heavy ties); last column: scaled by
    row_scale.  with_nan: 3 % NaN and one all-NaN group x column; otherwise m == n."""
    counts = MEDIAN_COUNTS[size]
    K = 3 if size == "small" else 2
    rng = np.random.default_rng(202 + (size == "large") + 2 * with_nan)
    group = _interleaved_groups(rng, counts)
    X = mixed(rng, (len(group), K), nan=0.03 if with_nan else 0)
    X[:, 1] = np.round(X[:, 1])
    G = len(counts)
    rows = [np.nonzero(group == g)[0] for g in range(G)]
    X[rows[G - 3][0], 0] = np.inf
    X[rows[G - 2][-1], 0] = -np.inf
    maj = rows[G - 4] if size == "small" else rows[1]      # 512 rows / 8193 rows
    X[maj[rng.permutation(len(maj))[:len(maj) // 2 + 5]], 0] = np.inf
    if with_nan:
        X[rows[3 if size == "small" else 0], 1] = np.nan
    col_scaled = np.zeros(K, dtype=np.uint8)
    col_scaled[K - 1] = 1
    row_scale = rng.choice([9 / 7, 3.0, 1.0], size=len(group))
    return NS(X=X, group=group, G=G, K=K, max_rows=max(counts), row_scale=row_scale,
              col_scaled=col_scaled, inf_majority=(G - 4 if size == "small" else 1, 0),
              all_nan=(3 if size == "small" else 0, 1) if with_nan else None)


def pandas_group_median(t):
    import pandas as pd
    Xs = scaled(t.X, t.row_scale, t.col_scaled)
    return pd.DataFrame(Xs).groupby(t.group).median().reindex(np.arange(t.G)).to_numpy()


# ------------------------------------------------------------------------------- robust MAD
MAD_NFIT = [1, 2, 3, 255, 256, 257, 1000, 4095, 4096]
MAD_N = 5000
MAD_INF_NFIT = [6, 257, 1000]
MAD_INF_COLUMNS = ["one +inf", "+inf and -inf", "majority +inf first", "majority +inf last",
                   "majority -inf first", "majority -inf last", "middle pair (finite, +inf)",
                   "middle pair (-inf, +inf)", "middle pair overflows"]


def _fit_rows(rng, n_fit):
    return rng.permutation(MAD_N)[:n_fit].astype(np.int32)      # shuffled, non-contiguous


@lru_cache(maxsize=None)
def mad_table(n_fit):
    """[N=5000, K=6]: mixed; rounded and free of NaN (the sort holds exactly n_fit values);
    constant over the fit rows; ~30 % NaN over the fit rows; all NaN over the fit rows; column 0
    again with 1e300 in every non-fit row."""
    rng = np.random.default_rng(300 + n_fit)
    fit = _fit_rows(rng, n_fit)
    X = mixed(rng, (MAD_N, 6))
    X[:, 1] = np.round(mixed(rng, MAD_N, nan=0))
    X[fit, 2] = 7.25
    X[fit[rng.random(n_fit) < 0.3], 3] = np.nan
    X[fit, 4] = np.nan
    X[:, 5] = X[:, 0]
    other = np.ones(MAD_N, dtype=bool)
    other[fit] = False
    X[other, 5] = 1e300
    return NS(X=X, fit=fit)


@lru_cache(maxsize=None)
def mad_inf_table(n_fit):
    """Fit rows holding +-inf, one column per MAD_INF_COLUMNS entry; "first"/"last" is the
    position of the infinite values in the order of the fit index.  The middle-pair columns
    drop one fit row (NaN) when n_fit is odd, so that their count is even."""
    rng = np.random.default_rng(400 + n_fit)
    fit = _fit_rows(rng, n_fit)
    X = mixed(rng, (MAD_N, len(MAD_INF_COLUMNS)))
    V = mixed(rng, (n_fit, len(MAD_INF_COLUMNS)), nan=0)     # V[i] = value at fit[i]
    V[rng.random(n_fit) < 0.03, :2] = np.nan
    maj = n_fit // 2 + 1
    V[n_fit // 3, 0] = np.inf
    V[n_fit // 3, 1], V[n_fit - 2, 1] = np.inf, -np.inf
    V[:maj, 2] = np.inf
    V[n_fit - maj:, 3] = np.inf
    V[:maj, 4] = -np.inf
    V[n_fit - maj:, 5] = -np.inf
    m = n_fit - n_fit % 2
    if n_fit % 2:
        V[n_fit - 1, 6:9] = np.nan
    pos = rng.permutation(m)
    V[pos[:m // 2], 6] = np.inf
    V[pos[:m // 2], 7], V[pos[m // 2:], 7] = -np.inf, np.inf
    V[pos[:m // 2 + 1], 8] = 1.5e308 + 1e305 * rng.random(m // 2 + 1)   # middle pair sums past DBL_MAX
    X[fit] = V
    return NS(X=X, fit=fit)


def scipy_mad_fit(X_fit):
    """pycytominer RobustMAD.fit from the libraries: (pandas median, scipy MAD)."""
    import warnings
    import pandas as pd
    from scipy.stats import median_abs_deviation
    X_fit = np.asarray(X_fit, dtype=np.float64)
    if X_fit.shape[0] == 0:
        return np.full(X_fit.shape[1], np.nan), np.full(X_fit.shape[1], np.nan)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        med = pd.DataFrame(X_fit).median().to_numpy()
        mad = median_abs_deviation(X_fit, nan_policy="omit", scale=MAD_SCALE)
    return med, np.asarray(mad, dtype=np.float64)


# ----------------------------------------------------------------------------- column stats
STATS_N = [1, 2, 255, 256, 257, 4095, 4096]
STATS_COLUMNS = ["distinct", "all equal", "two values, equal counts", "runs of 5, 5, 1", "rounded",
                 "+0.0 and -0.0", "with +-inf", "all NaN", "one non-NaN"]


@lru_cache(maxsize=None)
def stats_table(N):
    rng = np.random.default_rng(500 + N)
    X = np.empty((N, len(STATS_COLUMNS)))
    X[:, 0] = rng.permutation(N) * 0.37 - 11.0
    X[:, 1] = -2.5
    pair = np.array([1.0] * (N // 2) + [4.0] * (N // 2) + [np.nan] * (N % 2))   # equal counts
    X[:, 2] = pair[rng.permutation(N)]
    runs = np.full(N, np.nan)
    runs[:min(N, 11)] = ([3.0] * 5 + [-8.0] * 5 + [0.5])[:N]
    X[:, 3] = runs[rng.permutation(N)]
    X[:, 4] = np.round(mixed(rng, N, nan=0.03) if N > 2 else rng.normal(size=N))
    X[:, 5] = np.where(rng.random(N) < 0.5, 0.0, -0.0)
    X[:, 6] = mixed(rng, N)
    if N >= 2:
        X[0, 6], X[N - 1, 6] = np.inf, -np.inf
        if N > 4:
            X[2, 6] = np.inf
    else:
        X[0, 6] = np.inf
    X[:, 7] = np.nan
    X[:, 8] = np.nan
    X[rng.integers(N), 8] = 42.0
    return X


def pandas_column_stats(X):
    """(na_count, nunique, top count, second count, max, min) per column, from pandas."""
    import pandas as pd
    rows = []
    for j in range(X.shape[1]):
        s = pd.Series(X[:, j])
        vc = s.value_counts()
        rows.append((int(s.isna().sum()), int(s.nunique()),
                     int(vc.iloc[0]) if len(vc) > 0 else 0, int(vc.iloc[1]) if len(vc) > 1 else 0,
                     float(s.max()), float(s.min())))
    return rows


# --------------------------------------------------------------------------------- nancorr
CORR_SHAPES = [(1, 3), (2, 3), (3, 1), (5, 300), (384, 23), (8192, 2), (0, 2)]


@lru_cache(maxsize=None)
def corr_table(N, K):
    """Where the shape has room: a constant column, an all-NaN column, two columns whose finite
    rows do not overlap, two that overlap in one row, +-inf entries, an exact and a negated copy."""
    rng = np.random.default_rng(600 + 7 * N + K)
    X = mixed(rng, (N, K))
    if N == 0:
        return X
    if K >= 3:
        X[:, 1] = X[:, 0]                      # exact copy
        X[:, 2] = -X[:, 0]                     # negated copy
    if K >= 2 and N > 2:
        X[0, K - 1], X[N - 1, K - 1] = np.inf, -np.inf
    if K >= 12:
        X[:, 3] = 3.0                          # constant
        X[:, 4] = np.nan                       # all NaN
        half = np.arange(N) < N // 2
        X[half, 5], X[~half, 6] = np.nan, np.nan            # no common finite row
        X[:, 7:9] = rng.normal(size=(N, 2))
        X[np.arange(N) > N // 2, 7], X[np.arange(N) < N // 2, 8] = np.nan, np.nan   # one common row
    return X


# ---------------------------------------------------------------------------------- cosine
COSINE_CONFIGS = {"nine groups": ([0, 1, 24, 1, 0, 40, 2, 3, 0], 57), "one group": ([30], 57),
                  "one feature": ([0, 1, 24, 1, 0, 40, 2, 3, 0], 1)}


@lru_cache(maxsize=None)
def cosine_groups(name):
    """Groups with a zero row, an all-NaN row and scattered NaN; in the largest group rows
    (2, 9) are identical and rows (4, 17) opposite."""
    sizes, F = COSINE_CONFIGS[name]
    rng = np.random.default_rng(700 + len(sizes) + F)
    groups = [mixed(rng, (n, F), nan=0.03 if F > 1 else 0) for n in sizes]
    big = groups[int(np.argmax(sizes))]
    big[0], big[1] = 0.0, np.nan
    big[2] = big[9] = np.nan_to_num(big[9], nan=0.25)
    big[17] = np.nan_to_num(big[17], nan=-0.5)
    big[4] = -big[17]
    return groups


def cosine_longdouble(g):
    """sum (a / |a|) (b / |b|) in long double over np.triu_indices(n, 1); NaN read as 0, a zero
    norm replaced by 1."""
    x = np.nan_to_num(np.asarray(g, dtype=np.float64), nan=0.0).astype(np.longdouble)
    nrm = np.sqrt((x * x).sum(axis=1))
    nrm[nrm == 0] = 1
    xn = x / nrm[:, None]
    i, j = np.triu_indices(len(x), 1)
    return (xn[i] * xn[j]).sum(axis=1)


# --------------------------------------------------------------------------- MAD transform
def _rounded_power(t, k):
    try:
        return float(Fraction(t) ** k)
    except OverflowError:
        return math.copysign(math.inf, t) if k % 2 else math.inf


def overflow_edge(k):
    """The smallest double whose correctly rounded k-th power is inf."""
    t = DBL_MAX ** (1 / k)
    while math.isfinite(_rounded_power(t, k)):
        t = float(np.nextafter(t, np.inf))
    while not math.isfinite(_rounded_power(float(np.nextafter(t, 0.0)), k)):
        t = float(np.nextafter(t, 0.0))
    return t


@lru_cache(maxsize=None)
def power_inputs():
    """~2000 values of t: both signs log-spaced over 1e-100 .. 1e120, zeros, +-inf, NaN, and the
    8 doubles on each side of DBL_MAX**(1/6) and DBL_MAX**(1/3) and of the exact edges where
    t**6 and then t**3 round to inf (the float expression DBL_MAX**(1/k) lies some 30 doubles
    below its edge, because 1/k is rounded).  |t| < 1e-100 is left out on purpose: there t**3 is
    subnormal and the kernel's double-double product can differ from a correctly rounded power
    by double rounding."""
    mag = np.logspace(-100, 120, 960)
    edge = []
    for centre in (DBL_MAX ** (1 / 6), DBL_MAX ** (1 / 3), overflow_edge(6), overflow_edge(3)):
        lo = hi = centre
        edge.append(centre)
        for _ in range(8):
            lo, hi = np.nextafter(lo, 0.0), np.nextafter(hi, np.inf)
            edge += [lo, hi]
    edge = np.array(edge)
    return np.concatenate([mag, -mag, edge, -edge, [0.0, -0.0, np.inf, -np.inf, np.nan]])


@lru_cache(maxsize=None)
def power_expected():
    """|p3 / sqrt(1 + p6)| with p3, p6 the correctly rounded t**3, t**6 (exact rationals)."""
    t = power_inputs()
    with np.errstate(all="ignore"):
        p3, p6 = t ** 3, t ** 6        # zeros, inf and NaN: numpy's own
        for i, v in enumerate(t.tolist()):
            if math.isfinite(v) and v != 0.0:
                p3[i], p6[i] = _rounded_power(v, 3), _rounded_power(v, 6)
        return np.abs(p3 / np.sqrt(1.0 + p6))
