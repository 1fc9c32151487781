"""CPU: the intensity-extension columns' names and widths (cpx.csvout, cpx.device, cpx.plate's flag,
PlateTables' column order with and without colocalization), and the numpy restatement the GPU
tests compare against (tests/intensity_ext_ref.py) pinned on hand cases with the values written
out, its edge set against an independent scipy form."""
import numpy as np
import pytest

import intensity_ext_ref as ir
import synth_golden as sg
from cpx.csvout import PlateTables, colocalization_names, feature_names, intensity_ext_names
from cpx.device import n_colocalization, n_features, n_intensity_ext


def test_names_two_channels():
    assert intensity_ext_names(["DNA", "AGP"]) == [
        "Intensity_LowerQuartileIntensity_DNA", "Intensity_MedianIntensity_DNA",
        "Intensity_UpperQuartileIntensity_DNA", "Intensity_MADIntensity_DNA",
        "Intensity_IntegratedIntensityEdge_DNA", "Intensity_MeanIntensityEdge_DNA",
        "Intensity_StdIntensityEdge_DNA", "Intensity_MinIntensityEdge_DNA", "Intensity_MaxIntensityEdge_DNA",
        "Intensity_MassDisplacement_DNA", "Location_CenterMassIntensity_X_DNA",
        "Location_CenterMassIntensity_Y_DNA", "Location_MaxIntensity_X_DNA", "Location_MaxIntensity_Y_DNA",
        "Intensity_LowerQuartileIntensity_AGP", "Intensity_MedianIntensity_AGP",
        "Intensity_UpperQuartileIntensity_AGP", "Intensity_MADIntensity_AGP",
        "Intensity_IntegratedIntensityEdge_AGP", "Intensity_MeanIntensityEdge_AGP",
        "Intensity_StdIntensityEdge_AGP", "Intensity_MinIntensityEdge_AGP", "Intensity_MaxIntensityEdge_AGP",
        "Intensity_MassDisplacement_AGP", "Location_CenterMassIntensity_X_AGP",
        "Location_CenterMassIntensity_Y_AGP", "Location_MaxIntensity_X_AGP", "Location_MaxIntensity_Y_AGP"]


@pytest.mark.parametrize("C", range(1, 9))
def test_name_count_is_n_intensity_ext(C):
    chans = [f"ch{c}" for c in range(C)]
    names = intensity_ext_names(chans)
    assert len(names) == n_intensity_ext(C) == 14 * C == ir.n_intensity_ext(C)
    assert len(set(names)) == len(names)
    assert not set(names) & (set(feature_names(chans)) | set(colocalization_names(chans)))


def test_library_column_count_and_constants():
    from cpx import _lib
    lib = _lib.load()
    assert [lib.cpx_n_intensity_ext(C) for C in range(-1, 10)] == [0, 0] + [14 * C for C in range(1, 10)]
    assert n_intensity_ext(5) == 70 and n_intensity_ext(0) == 0
    assert _lib.N_IEXT == ir.N_IEXT == 14
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cpx.h")).read()
    assert int(re.search(r"#define CPX_IEXT_LDS_PIXELS (\d+)", hdr).group(1)) == _lib.IEXT_LDS_PIXELS
    # the header's column indices are the restatement's and the names' order
    for name, idx in (("LOWER_QUARTILE", ir.LOWER_QUARTILE), ("MEDIAN", ir.MEDIAN), ("UPPER_QUARTILE", ir.UPPER_QUARTILE),
                      ("MAD", ir.MAD), ("INTEGRATED_EDGE", ir.INTEGRATED_EDGE), ("MEAN_EDGE", ir.MEAN_EDGE),
                      ("STD_EDGE", ir.STD_EDGE), ("MIN_EDGE", ir.MIN_EDGE), ("MAX_EDGE", ir.MAX_EDGE),
                      ("MASS_DISPLACEMENT", ir.MASS_DISPLACEMENT), ("CENTER_MASS_X", ir.CENTER_MASS_X),
                      ("CENTER_MASS_Y", ir.CENTER_MASS_Y), ("MAX_X", ir.MAX_X), ("MAX_Y", ir.MAX_Y)):
        assert int(re.search(rf"#define CPX_IEXT_{name} (\d+)", hdr).group(1)) == idx


def test_plate_tables_column_order():
    chans = ["DNA", "AGP"]
    F, K, X = n_features(2), n_colocalization(2), n_intensity_ext(2)
    assert PlateTables(chans).cols == feature_names(chans)
    assert PlateTables(chans, intensity_ext=False).cols == feature_names(chans)
    assert PlateTables(chans, colocalization=True).cols == feature_names(chans) + colocalization_names(chans)
    ext = PlateTables(chans, intensity_ext=True)
    assert ext.cols == feature_names(chans) + intensity_ext_names(chans)
    both = PlateTables(chans, colocalization=True, intensity_ext=True)
    assert both.cols == feature_names(chans) + colocalization_names(chans) + intensity_ext_names(chans)
    lab = np.array([1, 2])
    ext.add_objects("Nuclei", 1, lab, np.zeros((2, F + X)))
    with pytest.raises(ValueError):
        ext.add_objects("Nuclei", 2, lab, np.zeros((2, F)))
    both.add_objects("Nuclei", 1, lab, np.zeros((2, F + K + X)))
    with pytest.raises(ValueError):
        both.add_objects("Nuclei", 2, lab, np.zeros((2, F + X)))
    assert list(both.frames()["Nuclei"].columns[3:]) == both.cols


def test_plate_parser_flag_and_config_default():
    from cpx import plate
    from cpx.pipeline import PipelineConfig
    base = ["--load-data", "ld.csv", "--data-path", "d", "--channels", "DNA", "AGP", "--out", "o"]
    assert plate.parse_args(base).intensity_extended is False
    a = plate.parse_args(base + ["--intensity-extended"])
    assert a.intensity_extended is True and a.colocalization is False
    assert PipelineConfig().intensity_ext is False


# ---- the restatement on hand cases ------------------------------------------------------------
def _one(x, lab=None):
    x = np.asarray(x, np.float32)
    lab = np.ones(x.shape, np.int32) if lab is None else np.asarray(lab, np.int32)
    return ir.intensity_ext(lab, x[None])


@pytest.mark.parametrize("n, want", [(1, (0, 0, 0)), (2, (0.5, 1, 1)), (3, (0.75, 1.5, 2)), (4, (1, 2, 3)),
                                     (5, (1.25, 2.5, 3.75)), (6, (1.5, 3, 4.5))])
def test_ref_quantiles_of_a_ramp(n, want):
    """v = 0 .. n - 1: CellProfiler's rule (n = 2: the larger value is the median)."""
    x = np.arange(n, dtype=np.float32)[::-1].reshape(1, n)      # unsorted on purpose
    r = _one(x)[0]
    assert tuple(r[[ir.LOWER_QUARTILE, ir.MEDIAN, ir.UPPER_QUARTILE]]) == want
    assert tuple(ir.quantile(np.arange(n, dtype=np.float64), f) for f in (0.25, 0.5, 0.75)) == want


def test_ref_mad_with_ties():
    # v = 1 1 2 2 2 4 9: n = 7, t = 3.5 -> (2 + 2) / 2 = 2; |x - 2| sorted = 0 0 0 1 1 2 7 -> (1 + 1) / 2 = 1
    r = _one([[2, 9, 1, 2, 4, 1, 2]])[0]
    assert r[ir.MEDIAN] == 2.0 and r[ir.MAD] == 1.0
    assert r[ir.LOWER_QUARTILE] == 1.0 * 0.25 + 2.0 * 0.75      # t = 1.75
    assert r[ir.UPPER_QUARTILE] == 4.0 * 0.75 + 9.0 * 0.25      # t = 5.25
    # constant object: MAD 0
    assert _one(np.full((3, 3), 5.0))[0][ir.MAD] == 0.0


def test_ref_three_by_three_in_a_corner():
    """A 3 x 3 object at (0, 0) of a 5 x 5 plane: only its centre pixel (1, 1) is no edge pixel."""
    lab = np.zeros((5, 5), np.int32)
    lab[:3, :3] = 1
    x = np.zeros((5, 5), np.float32)
    x[:3, :3] = [[1, 2, 3], [4, 50, 6], [7, 8, 9]]
    assert ir.edge_mask(lab).sum() == 8 and not ir.edge_mask(lab)[1, 1]
    r = _one(x, lab)[0]
    assert r[ir.INTEGRATED_EDGE] == 40.0 and r[ir.MEAN_EDGE] == 5.0
    assert r[ir.STD_EDGE] == np.sqrt((16 + 9 + 4 + 1 + 1 + 4 + 9 + 16) / 8.0)
    assert r[ir.MIN_EDGE] == 1.0 and r[ir.MAX_EDGE] == 9.0
    assert r[ir.MEDIAN] == 6.5                                   # 1 2 3 4 6 7 8 9 50: t = 4.5 -> (6 + 7) / 2
    assert (r[ir.MAX_Y], r[ir.MAX_X]) == (1.0, 1.0)


def test_ref_center_of_mass_and_displacement():
    lab = np.zeros((4, 6), np.int32)
    lab[1:3, 1:5] = 7
    x = np.zeros((4, 6), np.float32)
    x[1, 1] = 2.0
    x[2, 4] = 6.0
    r = _one(x, lab)[0]
    # sum x = 8; sum r x = 2 + 12 = 14; sum c x = 2 + 24 = 26; centroid (1.5, 2.5)
    assert r[ir.CENTER_MASS_Y] == 14.0 / 8.0 and r[ir.CENTER_MASS_X] == 26.0 / 8.0
    assert r[ir.MASS_DISPLACEMENT] == np.sqrt(0.25 ** 2 + 0.75 ** 2)
    assert (r[ir.MAX_Y], r[ir.MAX_X]) == (2.0, 4.0)
    # an all-zero object: 0 / 0
    z = _one(np.zeros((2, 2)))[0]
    assert np.isnan(z[[ir.CENTER_MASS_X, ir.CENTER_MASS_Y, ir.MASS_DISPLACEMENT]]).all()
    assert (z[ir.MAX_Y], z[ir.MAX_X]) == (0.0, 0.0) and z[ir.MEDIAN] == 0.0


def test_ref_first_maximum_in_raster_order():
    x = np.array([[1, 9, 3], [9, 2, 9]], np.float32)
    r = _one(x)[0]
    assert (r[ir.MAX_Y], r[ir.MAX_X]) == (0.0, 1.0)
    x[1, 0] = np.nan                                            # a NaN counts as the largest
    r = _one(x)[0]
    assert (r[ir.MAX_Y], r[ir.MAX_X]) == (1.0, 0.0)
    assert np.isnan(r[ir.MAX_EDGE]) and np.isnan(r[ir.MIN_EDGE])
    assert r[ir.LOWER_QUARTILE] == 2.0 * 0.5 + 3.0 * 0.5        # 1 2 3 9 9 nan: NaN sorts last; t = 1.5


def test_ref_negative_zero_is_positive_zero():
    r = _one([[-3.0, -0.0, -0.0]])[0]                           # t = 1.5: (-0 - 0) / 2
    assert r[ir.MEDIAN] == 0.0 and not np.signbit(r[ir.MEDIAN])
    assert not np.signbit(r[ir.MAX_EDGE]) and r[ir.MIN_EDGE] == -3.0


def test_ref_rows_follow_ascending_labels():
    lab = np.array([[5, 5, 2], [5, 2, 2]], np.int32)
    x = np.array([[1, 2, 3], [4, 5, 6]], np.float32)
    r = _one(x, lab)
    assert r.shape == (2, 14)
    assert r[0, ir.MEDIAN] == 5.0 * 0.5 + 6.0 * 0.5 and r[1, ir.MEDIAN] == 2.0 * 0.5 + 4.0 * 0.5
    assert (r[0, ir.MAX_Y], r[0, ir.MAX_X]) == (1.0, 2.0) and (r[1, ir.MAX_Y], r[1, ir.MAX_X]) == (1.0, 0.0)


def test_edge_set_against_scipy_filters():
    """minimum_filter != maximum_filter over the 3 x 3 neighbourhood, or the plane border."""
    from scipy.ndimage import maximum_filter, minimum_filter
    lab = sg.labels(70, 200, 232, n=30, rmin=3, rmax=30)
    border = np.zeros(lab.shape, bool)
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = True
    want = ((minimum_filter(lab, 3, mode="nearest") != maximum_filter(lab, 3, mode="nearest")) | border) & (lab > 0)
    got = ir.edge_mask(lab)
    np.testing.assert_array_equal(got, want)
    ids, n = np.unique(lab[lab > 0], return_counts=True)
    assert len(ids) == 28 and n.min() == 3
    assert min(int(got[lab == L].sum()) for L in ids) >= 3
