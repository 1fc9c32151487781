"""QC spectrum (k_qc.hip) and flat-field (k_illum.hip) kernels off the 2080 x 2080 plate shape,
every expectation computed at test time in fp64 numpy by the oracle (cpx_oracle.rps,
calculate_qc_metrics, illum_correct_qc, illum_correct_producer, calculate_saturation_cp_exact).
No kernel is compared with another kernel of the library.

Tolerances are those of tests/test_gpu_parity.py: slope rel 1e-9 / abs 1e-12; every ring sum
ps[r]/ps[0] against powersum[r]/powersum[0] at rtol 1e-9 (libcpx skips the reference's median
normalisation, one constant factor per plane); n_rings, n_valid, PercentMaximal, max_q, min_q and
the fp32 corrected plane exact; sum_q within N * 2**-53 relative of math.fsum of the fp64
quotients (the worst-case bound of an fp64 sum of N same-sign terms, whatever its order).

Inputs are uniform integer noise in [100, 4000) with an illumination function 0.7 + 0.6 * rand:
white noise puts comparable power in every ring, so a wrong butterfly moves some ring far more
than 1e-9 (blob images let the high rings fall to rounding level and hide such errors).

Which case reaches which path (K = min(H, W) // 8, KC = max(K, 1), npair = (H + 1) // 2;
k_qc_rows_2080 runs when W == 2080 and KC == 260, k_qc_cols_2080 when H == 2080):
  * make_plan radices 3, 7, 11, the lone radix 2 before odd stages, five stages, kMaxN:
    test_generic_fft_every_radix (each shape as the row plan and as the column plan);
  * odd H on the generic path: 63 x 99, 49 x 121, 77 x 91, 169 x 56, 4095 x 56, 2079 x 2080;
  * k_qc_rows_2080, one-row last pair and partial last block: test_rows_2080_fast_path_off_square
    (H = 2197: KC 260, npair % 4 == 3; 2100: 2; 2145: 1) and the modes at 2080 x 2080 (0);
  * k_qc_cols_2080 with W != 2080: test_cols_2080_fast_path_other_widths (W = 99: KC 12;
    W = 56: KC 7, one plane and eight; W = 2197: KC 260) and 2080 x 2079 (KC 259);
  * the three remaining illumination modes of k_qc_rows_2080: test_rows_2080_illumination_modes;
  * eq_count >= n/2 + 1 in k_qc_slope: test_median_zero_rule_at_its_threshold;
  * k_illum_correct<*, false>, plane % C and per-plane aux / XCD reorder with several planes:
    test_illum_scalar_path, test_illum_misaligned_pointers, test_generic_fft_batches.
"""
import ctypes as ct
import math

import numpy as np
import pytest
import torch

import cpx_oracle as orc
from cpx import _lib
from cpx.device import as_numpy

from test_gpu_parity import _run_qc, _t, _u16

pytestmark = pytest.mark.gpu

MODES = ("none", "f32", "f64", "image")


def _noise(seed, n, H, W, C=1):
    """n planes of uniform u16 noise in [100, 4000) and C flat-fields 0.7 + 0.6 * rand (fp64)."""
    rng = np.random.default_rng(seed)
    raw = rng.integers(100, 4000, (n, H, W), dtype=np.uint16)
    ill = 0.7 + 0.6 * rng.random((C, H, W))
    return raw, ill


def _illum_for(ill, mode):
    """The flat-field as the mode hands it over: None, float32 or float64 ('image' divides by
    the float32 one on the host, as the reference's per-channel float path does)."""
    if ill is None or mode == "none":
        return None
    return ill.astype(np.float64) if mode == "f64" else ill.astype(np.float32)


def _run_image(dev, img):
    """CPX_DTYPE_IMAGE_F64, called as cpx/qc.py calculate_qc_metrics does: the float64 plane is
    passed both as `raw` and as `illum`.  img [H,W] f64 -> (stats, qc, powersum)."""
    H, W = img.shape
    t = _t(dev, img.astype(np.float64))
    stats = dev.empty_bytes(64)
    qc = dev.empty_bytes(24)
    ps = torch.empty((1, max(min(H, W) // 8 - 2, 1)), dtype=torch.float64, device=dev.torch_device)
    p = ct.c_void_p(t.data_ptr())
    dev._bind_stream()
    _lib.check(dev.lib.cpx_illum_correct(dev.h, p, p, _lib.CPX_DTYPE_IMAGE_F64, 1, 1, H, W, None,
                                         ct.c_void_p(stats.data_ptr())), "cpx_illum_correct")
    _lib.check(dev.lib.cpx_qc_rps(dev.h, p, p, _lib.CPX_DTYPE_IMAGE_F64, 1, 1, H, W,
                                  ct.c_void_p(stats.data_ptr()), ct.c_void_p(ps.data_ptr()),
                                  ct.c_void_p(qc.data_ptr())), "cpx_qc_rps")
    dev.sync()
    return as_numpy(stats, "stats"), as_numpy(qc, "qc"), ps.cpu().numpy()


def _reference(img):
    """(powersum, metrics) of one fp64 plane: cpx_oracle.calculate_qc_metrics, keeping the ring
    sums of the one cpx_oracle.rps call it makes (an fft2 of a full plane is not run twice)."""
    kept = {}
    real = orc.rps

    def rps_once(x):
        kept["rps"] = real(x)
        return kept["rps"]

    orc.rps = rps_once
    try:
        m = orc.calculate_qc_metrics(img, "x")
    finally:
        orc.rps = real
    return np.asarray(kept["rps"][2], dtype=np.float64), m


def _assert_plane(img, st, qc, ps, tag, live):
    """One plane's stats / qc records and ring sums against the oracle on the fp64 plane `img`.
    live: the plane is ordinary, so its spectrum must really have been compared."""
    H, W = img.shape
    n_rings = max(min(H, W) // 8 - 2, 0)
    powersum, m = _reference(img)
    exp_slope, exp_pct = m["ImageQuality_PowerLogLogSlope_x"], m["ImageQuality_PercentMaximal_x"]
    assert qc["n_rings"] == n_rings, tag
    assert qc["pct_max"] == exp_pct and st["pct_max"] == exp_pct, tag
    if np.isnan(exp_slope):
        assert np.isnan(qc["slope"]), tag
    else:
        assert qc["slope"] == pytest.approx(exp_slope, rel=1e-9, abs=1e-12), tag
    compared = False
    if n_rings > 0:
        assert powersum.shape == (n_rings,), tag
        with np.errstate(invalid="ignore"):
            assert qc["n_valid"] == int(np.sum(powersum > 0)), tag
        if np.all(np.isfinite(powersum)) and powersum[0] > 0:
            np.testing.assert_allclose(ps[:n_rings] / ps[0], powersum / powersum[0], rtol=1e-9,
                                       err_msg=tag)
            compared = True
    assert compared or not live, f"{tag}: spectrum not compared"


def _check(dev, raw, ill, C, mode, tag, live=True):
    """raw [n,H,W] u16 and ill [C,H,W] fp64 (or None) through illum_correct + qc_rps in `mode`,
    every plane against the oracle."""
    n = raw.shape[0]
    il = _illum_for(ill, mode)
    with np.errstate(all="ignore"):
        imgs = [orc.illum_correct_qc(raw[p], None if il is None else il[p % C]) for p in range(n)]
    if mode == "image":
        for p in range(n):
            st, qc, ps = _run_image(dev, imgs[p])
            _assert_plane(imgs[p], st[0], qc[0], ps[0], f"{tag} image p{p}", live)
        return
    st, qc, ps, corr = _run_qc(dev, raw, il, C)
    for p in range(n):
        _assert_plane(imgs[p], st[p], qc[p], ps[p], f"{tag} {mode} p{p}", live)
        if mode == "f32":
            with np.errstate(all="ignore"):
                np.testing.assert_array_equal(corr[p], orc.illum_correct_producer(raw[p], il[p % C]),
                                              err_msg=f"{tag} p{p}")


# ---------------------------------------------------------------------------------------------
# A. generic FFT: every radix, as the row plan (W) and as the column plan (H)
# ---------------------------------------------------------------------------------------------

# (H, W): the plans make_plan gives for H and W
RADIX_SHAPES = [
    (63, 99),      # [7,3,3] x [11,3,3]; both odd (one-row last pair), N odd
    (49, 121),     # [7,7] x [11,11]: the twiddled second stage of each prime
    (77, 91),      # [11,7] x [13,7]
    (54, 50),      # [2,3,3,3] x [2,5,5]: the radix-2 stage that precedes odd stages
    (169, 56),     # [13,13] x [8,7]
    (4095, 56),    # [13,7,5,3,3]: five stages, odd, next to kMaxN
    (4096, 48),    # [8,8,8,8]: kMaxN itself; [8,2,3]
    (2079, 2080),  # [11,7,3,3,3]; K = 259, so neither 2080 row kernel; transposed: k_qc_cols_2080
]


@pytest.mark.parametrize("transposed", [False, True], ids=["rows_cols", "transposed"])
@pytest.mark.parametrize("shape", RADIX_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_generic_fft_every_radix(dev, shape, transposed):
    H, W = shape[::-1] if transposed else shape
    assert min(H, W) // 8 >= 6  # at least 4 rings: a defined slope
    raw, ill = _noise(1000 + H + 7 * W, 1, H, W)
    _check(dev, raw, ill, 1, "f32", f"{H}x{W}")


@pytest.mark.parametrize("H,W,n,C", [(63, 99, 8, 3), (56, 64, 8, 2)])
def test_generic_fft_batches(dev, H, W, n, C):
    """Several distinct planes, C > 1: plane p uses flat-field p % C and its own aux record; both
    shapes have KC = 7 and KC * n = 56 column blocks, so k_qc_cols' XCD reorder is on with a KC
    that is no power of two.  A swapped plane or channel fails."""
    assert (min(H, W) // 8) * n % 8 == 0 and min(H, W) // 8 == 7
    raw, ill = _noise(2000 + H, n, H, W, C)
    _check(dev, raw, ill, C, "f32", f"{H}x{W}x{n}")
    _check(dev, raw, ill, C, "f64", f"{H}x{W}x{n}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("H,W", [(63, 99), (54, 50)])
def test_generic_fft_illumination_modes(dev, H, W, mode):
    raw, ill = _noise(3000 + H, 2, H, W, 2)
    _check(dev, raw, ill, 2, mode, f"{H}x{W}")


# ---------------------------------------------------------------------------------------------
# B. the 2080 fast paths off the square
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("H,rem", [(2197, 3), (2100, 2), (2145, 1)])
def test_rows_2080_fast_path_off_square(dev, H, rem):
    """k_qc_rows_2080 (W == 2080, KC == 260) with H != 2080: a partial last block of row pairs
    (npair % 4 = rem) and, for odd H, a last pair of one row; the column pass is the generic
    one ([13,13,13] for 2197, [4,7,5,5,3] for 2100, [13,11,5,3] for 2145)."""
    W = 2080
    assert min(H, W) // 8 == 260 and ((H + 1) // 2) % 4 == rem
    raw, ill = _noise(4000 + H, 1, H, W)
    _check(dev, raw, ill, 1, "f32", f"{H}x{W}")


@pytest.mark.parametrize("W,n,KC", [(99, 1, 12), (56, 1, 7), (56, 8, 7), (2197, 1, 260)])
def test_cols_2080_fast_path_other_widths(dev, W, n, KC):
    """k_qc_cols_2080 (H == 2080) with W != 2080: its W - 1 - j fold, its compact row indexing and
    its XCD reorder (off for one plane of KC 7 or 12, on for eight planes: plane = V / KC with
    KC = 7) fed by the generic row pass."""
    H = 2080
    assert max(min(H, W) // 8, 1) == KC
    raw, ill = _noise(5000 + W + n, n, H, W, min(n, 3))
    _check(dev, raw, ill, min(n, 3), "f32", f"{H}x{W}x{n}")


@pytest.fixture(scope="module")
def full_plane():
    return _noise(6000, 1, 2080, 2080)


@pytest.mark.parametrize("mode", ["none", "f64", "image"])
def test_rows_2080_illumination_modes(dev, full_plane, mode):
    """k_qc_rows_2080<0>, <2> and <3> (the full-FOV tests use an f32 flat-field only)."""
    raw, ill = full_plane
    _check(dev, raw, ill, 1, mode, "2080x2080")


# ---------------------------------------------------------------------------------------------
# C. validity rules at their thresholds
# ---------------------------------------------------------------------------------------------


def _mean_1000_plane(H, W, n_equal, seed):
    """u16 plane of mean exactly 1000.0 with exactly n_equal pixels equal to it: the others in
    pairs 1000 +- d (d >= 1), and one triple 998, 1001, 1001 when their number is odd."""
    rng = np.random.default_rng(seed)
    n = H * W
    rest = n - n_equal
    vals = [np.full(n_equal, 1000, np.int64)]
    if rest % 2:
        vals.append(np.array([998, 1001, 1001], np.int64))
        rest -= 3
    d = rng.integers(1, 900, rest // 2)
    vals += [1000 + d, 1000 - d]
    flat = np.concatenate(vals)
    assert flat.size == n
    img = rng.permutation(flat).reshape(H, W).astype(np.uint16)
    assert img.astype(np.float64).mean() == 1000.0
    assert int(np.sum(img == 1000)) == n_equal
    return img


@pytest.mark.parametrize("mode", ["none", "image"])
@pytest.mark.parametrize("H,W", [(63, 99), (54, 50)])
def test_median_zero_rule_at_its_threshold(dev, H, W, mode):
    """median(|img - mean|) == 0 exactly when n // 2 + 1 pixels equal the mean (n odd or even):
    slope 0.0 there, an ordinary slope with one equal pixel fewer."""
    n = H * W
    over = _mean_1000_plane(H, W, n // 2 + 1, 7000 + H)
    under = _mean_1000_plane(H, W, n // 2, 7100 + H)
    ref_over = orc.calculate_qc_metrics(over.astype(float), "x")["ImageQuality_PowerLogLogSlope_x"]
    ref_under = orc.calculate_qc_metrics(under.astype(float), "x")["ImageQuality_PowerLogLogSlope_x"]
    assert np.median(np.abs(over.astype(float) - 1000.0)) == 0.0 and ref_over == 0.0
    assert np.median(np.abs(under.astype(float) - 1000.0)) > 0.0 and abs(ref_under) > 1e-3
    _check(dev, over[None], None, 1, mode, f"{H}x{W} n/2+1 equal", live=False)
    _check(dev, under[None], None, 1, mode, f"{H}x{W} n/2 equal")


def test_edge_planes_at_an_odd_shape(dev):
    """Constant plane, NaN and zero in the flat-field (NaN / inf quotient) at 63 x 99, and a plane
    with min(H, W) < 24 (no ring, slope NaN) at 21 x 99."""
    H, W = 63, 99
    raw, ill = _noise(8000, 1, H, W)
    const = np.full((1, H, W), 1234, np.uint16)
    for mode in ("none", "image"):
        _check(dev, const, None, 1, mode, "constant", live=False)
    ill_nan, ill_zero = ill.copy(), ill.copy()
    ill_nan[0, 17, 33] = np.nan
    ill_zero[0, 62, 98] = 0.0
    for mode in ("f32", "f64", "image"):
        _check(dev, raw, ill_nan, 1, mode, "nan illum", live=False)
        _check(dev, raw, ill_zero, 1, mode, "zero illum", live=False)
    st, _, _, _ = _run_qc(dev, raw, ill_zero.astype(np.float32))
    assert st[0]["has_inf"] == 1 and st[0]["has_nan"] == 0 and st[0]["max_q"] == np.inf
    st, _, _, _ = _run_qc(dev, raw, ill_nan.astype(np.float32))
    assert st[0]["has_nan"] == 1
    raw, ill = _noise(8001, 2, 21, 99, 2)
    for mode in MODES:
        _check(dev, raw, ill, 2, mode, "21x99", live=False)
    _, qc, _, _ = _run_qc(dev, raw, ill.astype(np.float32), 2)
    assert qc[0]["n_rings"] == 0 and np.isnan(qc[0]["slope"])


# ---------------------------------------------------------------------------------------------
# D. unsupported sizes fail cleanly
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("H,W", [(34, 40), (4100, 40)], ids=["factor17", "above_kMaxN"])
def test_unsupported_fft_size_raises_and_leaves_device_usable(dev, H, W):
    """A length with a prime factor above 13, or above kMaxN, is refused by cpx_qc_rps's argument
    check (CPX_ERR_SHAPE, status 3) before any launch; the next supported call is unaffected."""
    raw, ill = _noise(9000 + H, 1, H, W)
    with pytest.raises(_lib.CpxError, match=r"cpx_qc_rps failed with status 3\b"):
        _run_qc(dev, raw, ill.astype(np.float32))
    raw, ill = _noise(9001 + H, 1, 63, 99)
    _check(dev, raw, ill, 1, "f32", f"63x99 after {H}x{W}")


# ---------------------------------------------------------------------------------------------
# E. k_illum_correct: scalar path, plane % C, misaligned pointers
# ---------------------------------------------------------------------------------------------


def _assert_stats(st, q, tag):
    """Every field of one cpx_plane_stats record against the fp64 quotient plane q."""
    n = q.size
    has_nan = bool(np.isnan(q).any())
    assert st["n"] == n, tag
    assert st["has_nan"] == int(has_nan), tag
    assert st["pct_max"] == orc.calculate_saturation_cp_exact(q), tag
    if has_nan:
        assert np.isnan(st["max_q"]) and np.isnan(st["min_q"]) and np.isnan(st["sum_q"]), tag
        assert st["count_max"] == 0, tag
        return
    assert st["has_inf"] == int(bool(np.isinf(q).any())), tag
    assert st["max_q"] == q.max() and st["min_q"] == q.min(), tag
    assert st["count_max"] == int(np.sum(q == q.max())), tag
    ref = math.fsum(q.ravel().tolist())
    if math.isfinite(ref):
        assert abs(st["sum_q"] - ref) <= n * 2.0 ** -53 * abs(ref), (tag, st["sum_q"], ref)
    else:
        assert st["sum_q"] == ref, tag


def _tied_planes(seed, n, H, W, C):
    """Noise planes whose maximum is tied at p + 1 pixels of plane p, spread over the plane (first
    pixel, last pixel and between: different blocks and waves); the flat-field is 0.5 there so the
    tie holds in every mode.  The flat-field of the last channel has a zero: the planes that use it
    have max +inf."""
    raw, ill = _noise(seed, n, H, W, C)
    N = H * W
    pos = [0, N - 1, N // 2, N // 3, N // 5, 2 * N // 3, N // 7][:n]
    ill.reshape(C, N)[:, pos] = 0.5
    for p in range(n):
        raw[p].reshape(N)[pos[:p + 1]] = 65535
    ill[C - 1].reshape(N)[N // 2 + 11] = 0.0
    return raw, ill


def _run_illum(dev, raw_t, il_t, mode, C, n, H, W, corr_t):
    """cpx_illum_correct on device tensors as given (possibly misaligned views)."""
    stats = dev.empty_bytes(64 * n)
    if mode == "image":
        dev._bind_stream()
        _lib.check(dev.lib.cpx_illum_correct(dev.h, ct.c_void_p(raw_t.data_ptr()), ct.c_void_p(il_t.data_ptr()),
                                             _lib.CPX_DTYPE_IMAGE_F64, C, n, H, W,
                                             ct.c_void_p(corr_t.data_ptr()), ct.c_void_p(stats.data_ptr())),
                   "cpx_illum_correct")
    else:
        dev.illum_correct(raw_t.view(n, H, W), il_t, C, corr_t, stats)
    dev.sync()
    return as_numpy(stats, "stats").copy(), corr_t.cpu().numpy().reshape(n, H, W)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("H,W", [(63, 99), (37, 51)])
def test_illum_scalar_path(dev, H, W, mode):
    """H * W % 8 != 0: k_illum_correct<*, false>.  5 planes over C = 2 flat-fields, maxima tied at a
    different number of pixels per plane, +inf maxima through a zero of the flat-field."""
    assert (H * W) % 8 != 0
    n, C = 5, 2
    raw, ill = _tied_planes(10000 + H, n, H, W, C)
    il = _illum_for(ill, "f32" if mode == "image" else mode)
    with np.errstate(all="ignore"):
        q = [orc.illum_correct_qc(raw[p], None if il is None else il[p % C]) for p in range(n)]
    corr_t = torch.empty((n, H, W), dtype=torch.float32, device=dev.torch_device)
    if mode == "image":
        # the float64 planes themselves, one per channel: plane p is image p % C
        st, corr = _run_illum(dev, _u16(dev, raw), _t(dev, np.stack(q[:C])), mode, C, n, H, W, corr_t)
        q = [q[p % C] for p in range(n)]
    else:
        st, corr = _run_illum(dev, _u16(dev, raw), None if il is None else _t(dev, il), mode, C, n, H, W, corr_t)
    for p in range(n):
        _assert_stats(st[p], q[p], f"{H}x{W} {mode} p{p}")
        if mode != "none":
            assert st[p]["has_inf"] == int(p % C == C - 1)
        if mode == "f32":
            with np.errstate(all="ignore"):
                exp = orc.illum_correct_producer(raw[p], il[p % C])
        else:
            exp = q[p].astype(np.float32)  # the fp64 quotient stored as fp32
        np.testing.assert_array_equal(corr[p], exp, err_msg=f"{H}x{W} {mode} p{p}")
    if mode in ("none", "f32", "f64"):
        assert [int(s["count_max"]) for s in st if np.isfinite(s["max_q"])] == \
            [p + 1 for p in range(n) if mode == "none" or p % C != C - 1]


@pytest.mark.parametrize("which", ["raw", "illum", "out"])
def test_illum_misaligned_pointers(dev, which):
    """64 x 80 (H * W % 8 == 0) with one of raw / f32 flat-field / output starting one element into
    a longer allocation (2, 4, 4 bytes off 16-byte alignment): the scalar path, bit for bit the
    aligned call's results and the reference's."""
    H, W, n, C = 64, 80, 3, 2
    N = H * W
    raw, ill = _tied_planes(11000, n, H, W, C)
    il = ill.astype(np.float32)

    def dev_copy(a, dtype, off):
        flat = torch.zeros(a.size + 8, dtype=dtype, device=dev.torch_device)
        view = flat[off:off + a.size]
        view.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(dev.torch_device))
        assert view.is_contiguous() and view.data_ptr() == flat.data_ptr() + off * flat.element_size()
        return flat, view

    def run(off_raw, off_il, off_out):
        keep_r, r = dev_copy(raw.view(np.int16), torch.int16, off_raw)
        keep_i, i = dev_copy(il, torch.float32, off_il)
        keep_o, o = dev_copy(np.zeros(n * N, np.float32), torch.float32, off_out)
        assert keep_r.data_ptr() % 16 == 0 and keep_i.data_ptr() % 16 == 0 and keep_o.data_ptr() % 16 == 0
        st, corr = _run_illum(dev, r, i.view(C, H, W), "f32", C, n, H, W, o)
        assert float(keep_o[:off_out].abs().sum()) == 0.0 and float(keep_o[off_out + n * N:].abs().sum()) == 0.0
        return st, corr

    st0, corr0 = run(0, 0, 0)
    st1, corr1 = run(int(which == "raw"), int(which == "illum"), int(which == "out"))
    assert st1.tobytes() == st0.tobytes()
    assert corr1.tobytes() == corr0.tobytes()
    for p in range(n):
        with np.errstate(all="ignore"):
            q = orc.illum_correct_qc(raw[p], il[p % C])
            np.testing.assert_array_equal(corr1[p], orc.illum_correct_producer(raw[p], il[p % C]))
        _assert_stats(st1[p], q, f"misaligned {which} p{p}")
