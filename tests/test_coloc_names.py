"""CPU: the colocalization columns' names and widths (cpx.csvout, cpx.device, cpx.plate's flags), and
the numpy restatement the GPU tests compare against (tests/coloc_ref.py) pinned on hand cases."""
import numpy as np
import pytest

import coloc_ref
from cpx.csvout import PlateTables, colocalization_names, feature_names
from cpx.device import n_colocalization, n_features


def test_names_three_channels():
    assert colocalization_names(["DNA", "ER", "RNA"]) == [
        "Correlation_Correlation_DNA_ER", "Correlation_Overlap_DNA_ER", "Correlation_Manders_DNA_ER",
        "Correlation_Manders_ER_DNA", "Correlation_K_DNA_ER", "Correlation_K_ER_DNA",
        "Correlation_Correlation_DNA_RNA", "Correlation_Overlap_DNA_RNA", "Correlation_Manders_DNA_RNA",
        "Correlation_Manders_RNA_DNA", "Correlation_K_DNA_RNA", "Correlation_K_RNA_DNA",
        "Correlation_Correlation_ER_RNA", "Correlation_Overlap_ER_RNA", "Correlation_Manders_ER_RNA",
        "Correlation_Manders_RNA_ER", "Correlation_K_ER_RNA", "Correlation_K_RNA_ER"]


@pytest.mark.parametrize("C", range(1, 9))
def test_name_count_is_n_colocalization(C):
    chans = [f"ch{c}" for c in range(C)]
    names = colocalization_names(chans)
    assert len(names) == n_colocalization(C) == 6 * C * (C - 1) // 2 == coloc_ref.n_colocalization(C)
    assert len(set(names)) == len(names)
    assert not set(names) & set(feature_names(chans))


def test_library_column_count():
    from cpx import _lib
    lib = _lib.load()
    assert [lib.cpx_n_colocalization(C) for C in range(0, 9)] == [0] + [n_colocalization(C) for C in range(1, 9)]
    assert n_colocalization(5) == 60 and n_colocalization(1) == 0


def test_plate_tables_width():
    chans = ["DNA", "AGP"]
    F, K = n_features(2), n_colocalization(2)
    off = PlateTables(chans)
    assert off.cols == feature_names(chans)
    assert PlateTables(chans, colocalization=False).cols == feature_names(chans)
    on = PlateTables(chans, colocalization=True)
    assert on.cols == feature_names(chans) + colocalization_names(chans)
    lab = np.array([1, 2])
    on.add_objects("Nuclei", 1, lab, np.zeros((2, F + K)))
    with pytest.raises(ValueError):
        on.add_objects("Nuclei", 2, lab, np.zeros((2, F)))
    off.add_objects("Nuclei", 1, lab, np.zeros((2, F)))
    with pytest.raises(ValueError):
        off.add_objects("Nuclei", 2, lab, np.zeros((2, F + K)))
    assert list(on.frames()["Nuclei"].columns[3:]) == on.cols


def test_plate_parser_flags():
    from cpx import plate
    base = ["--load-data", "ld.csv", "--data-path", "d", "--channels", "DNA", "AGP", "--out", "o"]
    a = plate.parse_args(base)
    assert a.colocalization is False and a.colocalization_threshold == 15.0
    a = plate.parse_args(base + ["--colocalization", "--colocalization-threshold", "20"])
    assert a.colocalization is True and a.colocalization_threshold == 20.0


def test_pipeline_config_defaults_off():
    from cpx.pipeline import PipelineConfig
    cfg = PipelineConfig()
    assert cfg.colocalization is False and cfg.coloc_threshold == 15.0


# ---- the restatement on hand cases ------------------------------------------------------------
def _one(xa, xb, threshold=15.0):
    xa, xb = np.asarray(xa, np.float32), np.asarray(xb, np.float32)
    lab = np.ones(xa.shape, np.int32)
    r = coloc_ref.colocalization(lab, np.stack([xa, xb]), threshold)
    assert r.shape == (1, 6)
    return r[0]


def test_ref_linear_relations():
    xa = np.arange(1, 13, dtype=np.float32).reshape(3, 4)
    assert _one(xa, 2 * xa + 3)[0] == pytest.approx(1.0, abs=1e-15)
    assert _one(xa, -xa + 50)[0] == pytest.approx(-1.0, abs=1e-15)


def test_ref_one_pixel():
    r = _one([[7.0]], [[3.0]])
    assert np.isnan(r[0])
    assert r[1] == 1.0 and r[2] == 1.0 and r[3] == 1.0
    assert r[4] == 21.0 / 49.0 and r[5] == 21.0 / 9.0


def test_ref_constant_channel_and_empty_set():
    r = _one([[5.0, 5.0, 5.0]], [[1.0, 2.0, 3.0]])
    assert np.isnan(r[0]) and np.isfinite(r[1:]).all()
    # no pixel at or above both thresholds: every S sum is 0 -> Overlap and K are 0/0, Manders 0/100
    r = _one([[100.0, 1.0]], [[1.0, 100.0]])
    assert np.isfinite(r[0]) and np.isnan(r[[1, 4, 5]]).all() and r[2] == 0.0 and r[3] == 0.0


def test_ref_manders_and_k_by_hand():
    xa = [[10, 20, 30], [40, 50, 100]]
    xb = [[100, 5, 60], [0, 80, 50]]
    # t_a = t_b = 15; S = {(30, 60), (50, 80), (100, 50)}; x_a >= t_a: all but 10; x_b >= t_b: 100, 60, 80, 50
    r = _one(xa, xb)
    assert r[2] == 180.0 / 240.0
    assert r[3] == 190.0 / 290.0
    assert r[4] == 10800.0 / 13400.0
    assert r[5] == 10800.0 / 12500.0
    assert r[1] == 10800.0 / np.sqrt(13400.0 * 12500.0)
    xa64, xb64 = np.ravel(xa).astype(float), np.ravel(xb).astype(float)
    assert r[0] == pytest.approx(np.corrcoef(xa64, xb64)[0, 1], abs=1e-15)
    # threshold 0: S = P, both Manders 1; threshold 100: only pixels at both maxima (none here)
    r0 = _one(xa, xb, 0.0)
    assert r0[2] == 1.0 and r0[3] == 1.0
    r100 = _one(xa, xb, 100.0)
    assert np.isnan(r100[[1, 4, 5]]).all() and r100[2] == 0.0 and r100[3] == 0.0


def test_ref_rows_follow_ascending_labels_and_skip_other_objects():
    lab = np.array([[5, 5, 2], [5, 2, 2]], np.int32)
    xa = np.array([[1, 2, 3], [4, 5, 6]], np.float32)
    xb = np.array([[6, 5, 4], [3, 2, 1]], np.float32)
    r = coloc_ref.colocalization(lab, np.stack([xa, xb]))
    assert r.shape == (2, 6)
    np.testing.assert_array_equal(r[0], _one([[3, 5, 6]], [[4, 2, 1]]))
    np.testing.assert_array_equal(r[1], _one([[1, 2, 4]], [[6, 5, 3]]))
