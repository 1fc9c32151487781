"""Profile kernels (csrc/k_profiles.hip) at the edges of their sorts, chunks, limits and
infinities, bit-exact against the libraries they restate: pandas groupby mean / median,
DataFrame.corr, value_counts / nunique / isna / max / min, scipy median_abs_deviation, and exact
rationals for the powers of the double sigmoid (cosine similarities: 1e-13 against long double).

The input tables and their library references live in tests/profiles_edges_ref.py.  The CPU
tests pin oracle/profiles_oracle.py to the libraries on these very inputs, so the inputs can be
validated without a GPU; the GPU tests drive cpx.device.Device directly.
"""
import numpy as np
import pytest

import profiles_edges_ref as R
import profiles_oracle as po

pd = pytest.importorskip("pandas")


def _eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _stats_equal(a, b):
    return all(tuple(x[:4]) == tuple(y[:4]) and _eq(x[4:], y[4:]) for x, y in zip(a, b)) and len(a) == len(b)


# ------------------------------------------------------------------------------------ CPU
def test_inputs_group_mean_oracle_is_pandas():
    t = R.mean_table()
    ref, nobs = R.pandas_group_mean(t.X, t.group, t.G)
    assert _eq(po.group_kahan_mean(t.X, t.group, t.G), ref)
    assert np.isnan(ref[0]).all() and (nobs[0] == 0).all()              # the empty group
    for col in (0, 64):
        assert np.isnan(ref[5, col]) and nobs[5, col] == 0              # all NaN
        assert ref[7, col] == np.inf and ref[11, col] == -np.inf
        assert np.isnan(ref[9, col]) and nobs[9, col] > 0               # +inf then -inf
    Xs = R.scaled(t.X, t.row_scale, t.col_scaled)
    assert _eq(po.group_kahan_mean(Xs, t.group, t.G), R.pandas_group_mean(Xs, t.group, t.G)[0])
    # the streaming splits: one on a multiple of the 32-row chunk of a group, one inside groups
    full = np.bincount(t.group, minlength=t.G)
    cut = [(c, n) for s in t.splits for c, n in zip(np.bincount(t.group[:s], minlength=t.G), full)
           if 0 < c < n]
    assert any(c % 32 == 0 for c, n in cut) and any(c % 32 for c, n in cut)
    assert 64 in [np.bincount(t.group[:s], minlength=t.G)[7] for s in t.splits]


@pytest.mark.parametrize("size", ["small", "large"])
@pytest.mark.parametrize("with_nan", [False, True], ids=["no_nan", "nan"])
def test_inputs_group_median_oracle_is_pandas(size, with_nan):
    t = R.median_table(size, with_nan)
    ref = R.pandas_group_median(t)
    Xs = R.scaled(t.X, t.row_scale, t.col_scaled)
    mine = np.array([[po.median_1d(Xs[t.group == g, j]) for j in range(t.K)] for g in range(t.G)])
    assert _eq(mine, ref)
    assert ref[t.inf_majority] == np.inf
    assert np.isnan(ref).sum() == (1 if with_nan else 0)
    if with_nan:
        assert np.isnan(ref[t.all_nan])
    assert np.bincount(t.group).tolist() == R.MEDIAN_COUNTS[size]


@pytest.mark.parametrize("n_fit", [0] + R.MAD_NFIT)
def test_inputs_robust_mad_oracle_is_pandas_scipy(n_fit):
    t = R.mad_table(n_fit)
    med, mad = po.robust_mad_fit(t.X[t.fit])
    med_ref, mad_ref = R.scipy_mad_fit(t.X[t.fit])
    assert _eq(med, med_ref) and _eq(mad, mad_ref)
    if n_fit:
        assert mad_ref[2] == 0.0 and np.isnan(med_ref[4]) and np.isnan(mad_ref[4])
        assert med_ref[5] == med_ref[0] and mad_ref[5] == mad_ref[0]
        assert len(set(t.fit.tolist())) == n_fit                 # distinct rows ...
        assert n_fit < 255 or (np.diff(t.fit) < 0).sum() > n_fit // 4    # ... in shuffled order


@pytest.mark.parametrize("n_fit", R.MAD_INF_NFIT)
def test_inputs_robust_mad_inf_oracle_is_pandas_scipy(n_fit):
    t = R.mad_inf_table(n_fit)
    med, mad = po.robust_mad_fit(t.X[t.fit])
    med_ref, mad_ref = R.scipy_mad_fit(t.X[t.fit])
    assert _eq(med, med_ref) and _eq(mad, mad_ref)
    inf, nan = np.inf, np.nan
    assert np.isfinite(med_ref[:2]).all() and np.isfinite(mad_ref[:2]).all()
    assert _eq(med_ref[2:], [inf, inf, -inf, -inf, inf, nan, inf])
    assert _eq(mad_ref[2:], [nan, nan, nan, nan, nan, nan, inf])


@pytest.mark.parametrize("N", R.STATS_N)
def test_inputs_column_stats_oracle_is_pandas(N):
    X = R.stats_table(N)
    assert _stats_equal(po.column_stats(X), R.pandas_column_stats(X))


@pytest.mark.parametrize("N,K", R.CORR_SHAPES)
def test_inputs_nancorr_oracle_is_pandas(N, K):
    X = R.corr_table(N, K)
    assert _eq(po.nancorr(X), pd.DataFrame(X).corr().to_numpy())


def test_inputs_power_expected():
    """The exact-rational expectation agrees with numpy's own powers to a few ulp where both are
    finite, and passes from 1 to 0 (t**6 overflows) and to NaN (t**3 overflows) at the roots."""
    t, exp = R.power_inputs(), R.power_expected()
    assert 1900 < len(t) < 2100
    with np.errstate(all="ignore"):
        ref = np.abs(t ** 3 / np.sqrt(1 + t ** 6))
    edges = (R.overflow_edge(6), R.overflow_edge(3))
    far = ~np.any([np.abs(np.abs(t) / e - 1) < 1e-3 for e in edges], axis=0)
    # numpy's SIMD array pow strays up to a few tens of ulp from the correctly rounded powers
    np.testing.assert_allclose(exp[far], ref[far], rtol=1e-13, atol=0)
    for k, e, below, above in zip((6, 3), edges, (1.0, 0.0), (0.0, np.nan)):
        assert abs(R.DBL_MAX ** (1 / k) / e - 1) < 1e-13
        a, ulp = np.abs(t), np.spacing(e)
        under = exp[(a >= e - 8.5 * ulp) & (a < e)]          # 8 doubles below the edge, both signs
        over = exp[(a >= e) & (a <= e + 8.5 * ulp)]          # the edge and 8 above
        assert len(under) == 16 and len(over) == 18
        assert np.allclose(under, below, rtol=1e-14, atol=0) and _eq(over, [above] * 18)


# ------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def eng(dev):
    from cpx.profiles import ProfileEngine
    return ProfileEngine(dev)


def _raises(match):
    from cpx._lib import CpxError
    return pytest.raises(CpxError, match=match)


def _group_mean(eng, X, group, G, K, ld=None, slices=None, row_scale=None, col_scaled=None):
    """cpx_group_kahan_accumulate (one call per row slice, shared state) + finalize."""
    import torch
    n = len(X)
    buf = np.full((n, ld or K), 1e300)           # sentinel in the columns past K
    buf[:, :K] = X[:, :K]
    vals = eng._t(buf)
    sumx = torch.zeros((G, K), dtype=torch.float64, device=eng.td)
    comp = torch.zeros_like(sumx)
    nobs = torch.zeros((G, K), dtype=torch.int64, device=eng.td)
    rs = None if row_scale is None else eng._t(row_scale)
    cs = None if col_scaled is None else eng._t(col_scaled[:K])
    for lo, hi in slices or [(0, n)]:
        order, offs = R.order_offs(group[lo:hi], G)
        eng.dev.group_kahan(vals[lo:hi], eng._t(order), eng._t(offs), sumx, comp, nobs,
                            None if rs is None else rs[lo:hi], cs)
    out = torch.empty_like(sumx)
    eng.dev.group_finalize(sumx, nobs, out)
    return out.cpu().numpy(), nobs.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("K", R.MEAN_KS)
def test_group_mean_chunk_edges(eng, K):
    t = R.mean_table()
    ref, nobs_ref = R.pandas_group_mean(t.X[:, :K], t.group, t.G)
    got, nobs = _group_mean(eng, t.X, t.group, t.G, K)
    assert np.isnan(got[0]).all() and (nobs[0] == 0).all()
    assert np.array_equal(nobs, nobs_ref)
    assert _eq(got, ref)


@pytest.mark.gpu
def test_group_mean_ld_streaming_and_row_scale(eng):
    t = R.mean_table()
    K = 65
    ref, nobs_ref = R.pandas_group_mean(t.X[:, :K], t.group, t.G)
    got, nobs = _group_mean(eng, t.X, t.group, t.G, K, ld=70)             # ld > K
    assert _eq(got, ref) and np.array_equal(nobs, nobs_ref)
    s1, s2 = t.splits
    got, nobs = _group_mean(eng, t.X, t.group, t.G, K, slices=[(0, s1), (s1, s2), (s2, len(t.X))])
    assert _eq(got, ref) and np.array_equal(nobs, nobs_ref)
    assert 0 < t.col_scaled[:K].sum() < K
    Xs = R.scaled(t.X[:, :K], t.row_scale, t.col_scaled)
    got, _ = _group_mean(eng, t.X, t.group, t.G, K, row_scale=t.row_scale, col_scaled=t.col_scaled)
    assert _eq(got, R.pandas_group_mean(Xs, t.group, t.G)[0])
    assert not _eq(got, ref)


@pytest.mark.gpu
def test_group_mean_rejects_bad_sizes(eng):
    """Host-side argument checks (nothing is launched): G = 65536, K = 0, ld < K."""
    import torch
    from cpx._lib import check
    from cpx.device import _ptr
    v = torch.zeros((4, 4), dtype=torch.float64, device=eng.td)
    i32 = torch.zeros(8, dtype=torch.int32, device=eng.td)
    st = torch.zeros((2, 4), dtype=torch.float64, device=eng.td)
    comp = torch.zeros_like(st)
    nobs = torch.zeros((2, 4), dtype=torch.int64, device=eng.td)

    def call(K, ld, G):
        check(eng.dev.lib.cpx_group_kahan_accumulate(eng.dev.h, _ptr(v), 4, K, ld, _ptr(i32), _ptr(i32),
                                                     G, None, None, _ptr(st), _ptr(comp), _ptr(nobs)),
              "cpx_group_kahan_accumulate")
    for K, ld, G in ((4, 4, 65536), (0, 4, 2), (4, 3, 2)):
        with _raises("cpx_group_kahan_accumulate: bad sizes"):
            call(K, ld, G)
    call(4, 4, 2)      # the same buffers with good sizes pass


def _group_median(eng, t, max_rows=None):
    import torch
    order, offs = R.order_offs(t.group, t.G)
    out = torch.empty((t.G, t.K), dtype=torch.float64, device=eng.td)
    eng.dev.group_median(eng._t(t.X), eng._t(order), eng._t(offs), max_rows or t.max_rows, out,
                         eng._t(t.row_scale), eng._t(t.col_scaled))
    return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("size", ["small", "large"])
@pytest.mark.parametrize("with_nan", [False, True], ids=["no_nan", "nan"])
def test_group_median_sort_sizes(eng, size, with_nan):
    """small: 1 .. 4097 rows per group (K = 3); large: 8192, 8193 and 16384 rows (K = 2), the
    launches past 64 KB of dynamic LDS."""
    t = R.median_table(size, with_nan)
    got = _group_median(eng, t)
    assert _eq(got, R.pandas_group_median(t))
    assert got[t.inf_majority] == np.inf


@pytest.mark.gpu
def test_group_median_rejects_too_many_rows(eng):
    t = R.median_table("small", False)
    with _raises("cpx_group_median: bad argument \\(at most 16384 rows per group\\)"):
        _group_median(eng, t, max_rows=16385)


def _robust_mad(eng, X, fit):
    import torch
    K = X.shape[1]
    med = torch.empty(K, dtype=torch.float64, device=eng.td)
    mad = torch.empty_like(med)
    eng.dev.robust_mad(eng._t(X.T), eng._t(fit), R.MAD_SCALE, med, mad)
    return med.cpu().numpy(), mad.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("n_fit", [0] + R.MAD_NFIT)
def test_robust_mad_sizes(eng, n_fit):
    """n_fit = 0 gives NaN, NaN like the libraries (an empty fit index is accepted)."""
    t = R.mad_table(n_fit)
    med, mad = _robust_mad(eng, t.X, t.fit)
    med_ref, mad_ref = R.scipy_mad_fit(t.X[t.fit])
    assert _eq(med, med_ref) and _eq(mad, mad_ref)
    if n_fit == 0:
        assert np.isnan(med).all() and np.isnan(mad).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n_fit", R.MAD_INF_NFIT)
def test_robust_mad_infinite_values(eng, n_fit):
    """A median of +-inf that a value equals gives a NaN MAD (scipy: inf - inf among the
    deviations), whatever the order of the fit rows; an overflowed median gives inf."""
    t = R.mad_inf_table(n_fit)
    med, mad = _robust_mad(eng, t.X, t.fit)
    med_ref, mad_ref = R.scipy_mad_fit(t.X[t.fit])
    for j, name in enumerate(R.MAD_INF_COLUMNS):
        assert _eq(med[j], med_ref[j]) and _eq(mad[j], mad_ref[j]), (name, med[j], mad[j])
    # the same rows gathered in the reverse order
    med_r, mad_r = _robust_mad(eng, t.X, t.fit[::-1].copy())
    assert _eq(med_r, med_ref) and _eq(mad_r, mad_ref)


@pytest.mark.gpu
def test_robust_mad_rejects_too_many_fit_rows(eng):
    X = R.mad_table(4096).X
    with _raises("cpx_robust_mad: bad argument \\(at most 4096 fit rows\\)"):
        _robust_mad(eng, X, np.arange(4097, dtype=np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("N", R.STATS_N)
def test_column_stats_sizes(eng, N):
    X = R.stats_table(N)
    got = eng.column_stats(X)
    assert _stats_equal(got, R.pandas_column_stats(X)), got
    assert _stats_equal(got, po.column_stats(X))


@pytest.mark.gpu
def test_column_stats_rejects_too_many_rows(eng):
    with _raises("cpx_column_stats: bad argument \\(at most 4096 rows\\)"):
        eng.column_stats(np.zeros((4097, 2)))


@pytest.mark.gpu
@pytest.mark.parametrize("N,K", R.CORR_SHAPES)
def test_nancorr_shapes(eng, N, K):
    """(5, 300): 177 blocks of pairs ending mid-block; (8192, 2): the 64 KB LDS launch;
    (0, 2): an empty matrix, all NaN."""
    X = R.corr_table(N, K)
    got = eng.corr(X)
    assert np.array_equal(got, got.T, equal_nan=True)
    assert _eq(got, pd.DataFrame(X).corr().to_numpy())


@pytest.mark.gpu
def test_nancorr_rejects_too_many_rows(eng):
    with _raises("cpx_nancorr: bad argument \\(N <= 8192 rows\\)"):
        eng.corr(np.zeros((8193, 2)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(R.COSINE_CONFIGS))
def test_cosine_groups(eng, name):
    groups = R.cosine_groups(name)
    got = eng.group_cosine(groups)
    assert [len(v) for v in got] == [len(g) * (len(g) - 1) // 2 for g in groups]
    if name == "nine groups":
        assert sum(len(v) for v in got) == 1060          # five blocks of 256 pairs
    for g, v in zip(groups, got):
        np.testing.assert_allclose(v, R.cosine_longdouble(g).astype(np.float64), rtol=0, atol=1e-13)
    # np.triu_indices order: the identical rows (2, 9) and the opposite rows (4, 17) of the
    # largest group; the zero row 0 and the all-NaN row 1 give 0 with every other row
    b = int(np.argmax([len(g) for g in groups]))
    i, j = np.triu_indices(len(groups[b]), 1)
    v = got[b]
    assert abs(v[(i == 2) & (j == 9)][0] - 1.0) <= 1e-13
    assert abs(v[(i == 4) & (j == 17)][0] + 1.0) <= 1e-13
    assert (v[(i <= 1) | (j <= 1)] == 0.0).all()


def _mad_transform(eng, X, med, mad, eps, sigmoid, alpha=1.0):
    import torch
    col = eng._t(X.T)
    out = torch.empty_like(col)
    eng.dev.mad_transform(col, eng._t(med), eng._t(mad), eps, out, double_sigmoid=sigmoid, alpha=alpha)
    return out.cpu().numpy().T


@pytest.mark.gpu
def test_mad_transform_powers_bit_exact(eng):
    """med 0, mad 1, eps 0, alpha 1: t = x exactly; every element equals |p3 / sqrt(1 + p6)| of
    the correctly rounded powers, through the overflow of t**6 and of t**3."""
    t = R.power_inputs()
    got = _mad_transform(eng, t[:, None], np.zeros(1), np.ones(1), 0.0, True)[:, 0]
    exp = R.power_expected()
    bad = np.nonzero(~((got == exp) | (np.isnan(got) & np.isnan(exp))))[0]
    assert len(bad) == 0, [(float(t[i]).hex(), got[i], exp[i]) for i in bad[:10]]


@pytest.mark.gpu
def test_mad_transform_without_sigmoid(eng):
    rng = np.random.default_rng(801)
    X = R.mixed(rng, (257, 3))                   # 771 elements: not a multiple of the block
    X[5, 0] = np.inf
    med = np.array([0.5, np.nan, -3e4])
    mad = np.array([0.0, 2.0, np.inf])
    eps = 1e-18
    with np.errstate(all="ignore"):
        ref = (X - med) / (mad + eps)
    assert _eq(_mad_transform(eng, X, med, mad, eps, False), ref)
    one = _mad_transform(eng, np.array([[7.5]]), np.array([1.5]), np.array([3.0]), 0.0, False)   # K = N = 1
    assert one.shape == (1, 1) and one[0, 0] == 2.0
    one = _mad_transform(eng, np.array([[7.5]]), np.array([1.5]), np.array([3.0]), 0.0, True, alpha=2.0)
    assert one[0, 0] == 1.0 / np.sqrt(2.0)
