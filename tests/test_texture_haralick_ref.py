"""CPU: the opt-in Haralick texture columns' names and widths (cpx.csvout, cpx.device, cpx.plate's
flag, PlateTables' header under every combination of the three opt-in flags), and the numpy
restatement the GPU tests compare against (tests/haralick_ref.py) pinned on closed forms and on
the identities that tie it to the existing greycoprops columns."""
import itertools
import math
import os
import re

import numpy as np
import pytest

import cpx_oracle as orc
import haralick_ref as hr
import synth_golden as sg
from cpx.csvout import (HARALICK_NAMES, PlateTables, colocalization_names, feature_names, haralick_names,
                        intensity_ext_names)
from cpx.device import n_colocalization, n_features, n_intensity_ext, n_texture_haralick

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- names, widths, flags ---------------------------------------------------------------------
def test_names_one_channel_direction_major():
    names = haralick_names(["DNA"])
    assert names[:9] == [f"Texture_{n}_DNA_3_00_256" for n in
                         ("Variance", "SumAverage", "SumVariance", "SumEntropy", "Entropy", "DifferenceVariance",
                          "DifferenceEntropy", "InfoMeas1", "InfoMeas2")]
    assert names[9] == "Texture_Variance_DNA_3_01_256" and names[35] == "Texture_InfoMeas2_DNA_3_03_256"
    two = haralick_names(["DNA", "AGP"])
    assert two[:36] == names and two[36] == "Texture_Variance_AGP_3_00_256"
    # column (c * 4 + d) * 9 + j
    assert two[(1 * 4 + 2) * 9 + 4] == "Texture_Entropy_AGP_3_02_256"
    assert "InverseDifferenceMoment" not in " ".join(two)  # it is the existing Homogeneity column


@pytest.mark.parametrize("C", range(1, 10))
def test_name_count_unique_and_disjoint(C):
    chans = [f"ch{c}" for c in range(C)]
    names = haralick_names(chans)
    assert len(names) == n_texture_haralick(C) == 36 * C == hr.n_texture_haralick(C)
    assert len(set(names)) == len(names)
    assert not set(names) & (set(feature_names(chans)) | set(colocalization_names(chans)) |
                             set(intensity_ext_names(chans)))


def test_library_column_count_and_header_order():
    from cpx import _lib
    lib = _lib.load()
    assert [lib.cpx_n_texture_haralick(C) for C in range(-1, 11)] == [0, 0] + [36 * C for C in range(1, 11)]
    assert n_texture_haralick(5) == 180 and n_texture_haralick(0) == 0
    assert _lib.N_HAR == hr.N_HAR == len(HARALICK_NAMES) == 9
    hdr = open(os.path.join(REPO, "include", "cpx.h")).read()
    assert int(re.search(r"#define CPX_N_HAR (\d+)", hdr).group(1)) == 9
    macro = {"Variance": "VARIANCE", "SumAverage": "SUM_AVERAGE", "SumVariance": "SUM_VARIANCE",
             "SumEntropy": "SUM_ENTROPY", "Entropy": "ENTROPY", "DifferenceVariance": "DIFFERENCE_VARIANCE",
             "DifferenceEntropy": "DIFFERENCE_ENTROPY", "InfoMeas1": "INFO_MEAS1", "InfoMeas2": "INFO_MEAS2"}
    for idx, name in enumerate(HARALICK_NAMES):
        assert int(re.search(rf"#define CPX_HAR_{macro[name]} (\d+)", hdr).group(1)) == idx
        assert getattr(hr, macro[name]) == idx


@pytest.mark.parametrize("coloc, iext, har", list(itertools.product((False, True), repeat=3)))
def test_csv_header_for_every_flag_combination(tmp_path, coloc, iext, har):
    chans = ["DNA", "AGP"]
    want = feature_names(chans) + (colocalization_names(chans) if coloc else []) + \
        (intensity_ext_names(chans) if iext else []) + (haralick_names(chans) if har else [])
    t = PlateTables(chans, colocalization=coloc, intensity_ext=iext, texture_haralick=har)
    assert t.cols == want
    width = n_features(2) + (n_colocalization(2) if coloc else 0) + (n_intensity_ext(2) if iext else 0) + \
        (n_texture_haralick(2) if har else 0)
    assert len(want) == width
    t.add_objects("Nuclei", 1, np.array([1, 2]), np.arange(2.0 * width).reshape(2, width))
    with pytest.raises(ValueError):
        t.add_objects("Nuclei", 2, np.array([1, 2]), np.zeros((2, width + 1)))
    t.write_objects(str(tmp_path), "Nuclei")
    with open(tmp_path / "Nuclei.csv") as f:
        lines = f.read().splitlines()
    assert lines[0].split(",")[3:] == want and len(lines) == 3
    assert len(lines[1].split(",")) == 3 + width


def test_plate_parser_flag_and_config_default():
    from cpx import plate
    from cpx.pipeline import PipelineConfig
    base = ["--load-data", "ld.csv", "--data-path", "d", "--channels", "DNA", "AGP", "--out", "o"]
    assert plate.parse_args(base).texture_haralick is False
    a = plate.parse_args(base + ["--texture-haralick"])
    assert a.texture_haralick is True and a.colocalization is False and a.intensity_extended is False
    assert PipelineConfig().texture_haralick is False


# ---- the restatement on closed forms ----------------------------------------------------------
def _matrices(x, lab=None):
    x = np.asarray(x, np.float32)
    lab = np.ones(x.shape, np.int32) if lab is None else np.asarray(lab, np.int32)
    return hr.count_matrices(lab, x)


def test_checkerboard_closed_form():
    """An 8 x 8 checkerboard of levels 0 and 255.  (0, 3) joins unlike squares: N(0, 255) = N(255, 0)
    = 20; (2, 2) joins like squares: N(0, 0) = N(255, 255) = 18."""
    yy, xx = np.mgrid[0:8, 0:8]
    N = _matrices(((yy + xx) % 2).astype(np.float32))[0]
    assert N[0][0, 255] == N[0][255, 0] == 20 and N[0].sum() == 40
    assert N[1][0, 0] == N[1][255, 255] == 18 and N[1].sum() == 36
    im2 = math.sqrt(1.0 - math.exp(-2.0))
    r, e = hr.from_counts(N[0])
    assert e == (1.0, 1.0, 1.0)
    assert r == [127.5 ** 2, 255.0, 0.0, 0.0, 1.0, 0.0, 0.0, -1.0, im2]
    r, e = hr.from_counts(N[1])
    assert e == (1.0, 1.0, 1.0)
    assert r == [127.5 ** 2, 255.0, 255.0 ** 2, 1.0, 1.0, 0.0, 0.0, -1.0, im2]


def test_one_pair_matrix():
    N = np.zeros((256, 256), np.int64)
    N[3, 10] = 1
    r, e = hr.from_counts(N)
    assert r == [0.0, 13.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0] and e == (0.0, 0.0, 0.0)
    assert not np.signbit(r).any()
    # a rank-one matrix (independent rows and columns): HXY = HX + HY, so both InfoMeas are 0
    N = np.zeros((256, 256), np.int64)
    N[np.ix_([2, 9], [5, 7])] = [[1, 3], [2, 6]]
    r, (hx, hy, hxy) = hr.from_counts(N)
    assert abs(hxy - hx - hy) < 1e-15 and abs(r[hr.INFO_MEAS1]) < 1e-15 and r[hr.INFO_MEAS2] < 1e-7


def test_no_pair_gives_nine_positive_zeros():
    r, e = hr.from_counts(np.zeros((256, 256), np.int64))
    assert r == [0.0] * 9 and not np.signbit(r).any() and e == (0.0, 0.0, 0.0)
    # a 3 x 1 object: no direction has a pair
    rows, ent = hr.haralick(np.ones((3, 1), np.int32), np.array([[[5.0], [7.0], [9.0]]], np.float32))
    assert rows.shape == (1, 36) and (rows == 0.0).all() and not np.signbit(rows).any() and (ent == 0.0).all()
    # 1 x 7: (0, 3) only
    rows, _ = hr.haralick(np.ones((1, 7), np.int32), np.arange(7, dtype=np.float32).reshape(1, 1, 7))
    assert rows[0, hr.SUM_AVERAGE] > 0 and (rows[0, 9:] == 0.0).all()


def _random_matrices():
    """Count matrices of random crops: smooth and noisy planes, labels with masked bbox pixels."""
    H, W = 120, 136
    lab = sg.labels(31, H, W, n=14, rmin=3, rmax=24)
    rng = np.random.default_rng(5)
    planes = [sg.plane(40, H, W, n_blobs=12, saturate=False).astype(np.float32),
              rng.uniform(-50.0, 900.0, (H, W)).astype(np.float32)]
    out = [N for p in planes for m in hr.count_matrices(lab, p) for N in m if N.sum() > 0]
    assert len(out) > 40
    return out


def test_identities_with_greycoprops_on_random_crops():
    lv = np.arange(256, dtype=np.float64)
    for N in _random_matrices():
        r, _ = hr.from_counts(N)
        con, dis = orc.greycoprops(N)[:2]
        px, py, psum, pdiff, _ = hr.marginals(N)
        mud = float(np.sum(lv * pdiff))
        mux, muy = float(np.sum(lv * px)), float(np.sum(lv * py))
        P = N / N.sum()
        cov = float(np.sum(P * np.outer(lv - mux, lv - muy)))
        vy = float(np.sum((lv - muy) ** 2 * py))
        np.testing.assert_allclose(con, r[hr.DIFFERENCE_VARIANCE] + mud ** 2, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(dis, mud, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(r[hr.SUM_AVERAGE], mux + muy, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(r[hr.SUM_VARIANCE], r[hr.VARIANCE] + vy + 2.0 * cov, rtol=1e-9, atol=1e-9)
        assert np.isfinite(r).all() and 0.0 <= r[hr.INFO_MEAS2] <= 1.0 and r[hr.INFO_MEAS1] <= 1e-12


def test_hxy1_and_hxy2_equal_hx_plus_hy():
    """Haralick's HXY1 = -sum P log2(px py) and HXY2 = -sum px py log2(px py), as literal double sums."""
    for N in _random_matrices()[::3]:
        px, py, _, _, _ = hr.marginals(N)
        P = N / N.sum()
        Q = np.outer(px, py)
        with np.errstate(divide="ignore", invalid="ignore"):
            lq = np.where(Q > 0, np.log2(Q), 0.0)
        hx, hy = hr.entropy(px), hr.entropy(py)
        assert abs(-np.sum(P * lq) - (hx + hy)) <= 1e-12
        assert abs(-np.sum(Q * lq) - (hx + hy)) <= 1e-12
