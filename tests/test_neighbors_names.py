"""CPU: the names, order and place of the Neighbors_* columns (cpx.csvout.neighbors_names,
PlateTables(neighbors=...)) and the --neighbors option's parsing."""
import pytest

from cpx import csvout


def test_neighbors_names():
    names = csvout.neighbors_names(("Adjacent", 5))
    assert names == [
        "Neighbors_NumberOfNeighbors_Adjacent", "Neighbors_PercentTouching_Adjacent",
        "Neighbors_FirstClosestObjectNumber_Adjacent", "Neighbors_FirstClosestDistance_Adjacent",
        "Neighbors_SecondClosestObjectNumber_Adjacent", "Neighbors_SecondClosestDistance_Adjacent",
        "Neighbors_AngleBetweenNeighbors_Adjacent",
        "Neighbors_NumberOfNeighbors_5", "Neighbors_PercentTouching_5",
        "Neighbors_FirstClosestObjectNumber_5", "Neighbors_FirstClosestDistance_5",
        "Neighbors_SecondClosestObjectNumber_5", "Neighbors_SecondClosestDistance_5",
        "Neighbors_AngleBetweenNeighbors_5"]
    assert csvout.neighbors_names(()) == []
    assert csvout.neighbors_names((1,))[0] == "Neighbors_NumberOfNeighbors_1"  # D = 1 given as a number
    assert len(set(csvout.neighbors_names(("Adjacent", 1, 2, 32)))) == 28


def test_counts_and_constants():
    from cpx import _lib
    from cpx.device import n_neighbors, neighbors_distances
    assert _lib.N_NEIGHBORS == 7 and _lib.NEIGHBORS_MAX_DISTANCE == 32 and _lib.NEIGHBORS_MAX_SCALES == 4
    assert n_neighbors(()) == 0 and n_neighbors(("Adjacent", 5)) == 14 and n_neighbors(3) == 21
    assert neighbors_distances(("Adjacent", 5, "adjacent")) == [1, 5, 1]
    assert len(csvout.neighbors_names(("Adjacent", 5))) == n_neighbors(("Adjacent", 5))


def test_plate_tables_place_the_block_last():
    chans = ["DNA", "AGP"]
    base = csvout.PlateTables(chans).cols
    assert csvout.PlateTables(chans, neighbors=()).cols == base == csvout.feature_names(chans)
    on = csvout.PlateTables(chans, neighbors=("Adjacent", 5)).cols
    assert on == base + csvout.neighbors_names(("Adjacent", 5))
    every = csvout.PlateTables(chans, colocalization=True, intensity_ext=True, texture_haralick=True,
                               neighbors=(5,)).cols
    assert every == (base + csvout.colocalization_names(chans) + csvout.intensity_ext_names(chans) +
                     csvout.haralick_names(chans) + csvout.neighbors_names((5,)))


def test_plate_option():
    from cpx import plate
    need = ["--load-data", "x.csv", "--data-path", "d", "--illum-path", "i", "--channels", "DNA", "AGP", "--out", "o"]
    assert plate.parse_args(need).neighbors == ()
    assert plate.parse_args(need + ["--neighbors", "Adjacent,5"]).neighbors == ("Adjacent", 5)
    assert plate.parse_args(need + ["--neighbors", "adjacent"]).neighbors == ("Adjacent",)
    for bad in ("0", "33", "1,2,3,4,5", "near", ""):
        with pytest.raises(SystemExit):
            plate.parse_args(need + ["--neighbors", bad])


def test_pipeline_config_default():
    from cpx.pipeline import PipelineConfig
    assert PipelineConfig(H=8, W=8, C=1).neighbors == ()


def test_constants_mirror_the_header():
    """cpx._lib's copies of the block's constants (the size scenes take the kernel's tile from them)
    are the values include/cpx.h defines."""
    import os
    import re
    from cpx import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "cpx.h")) as f:
        defs = dict(re.findall(r"^#define (CPX_N(?:EIGHBORS_\w+|_NEIGHBORS)) (\d+)", f.read(), re.M))
    want = {"CPX_N_NEIGHBORS": _lib.N_NEIGHBORS, "CPX_NEIGHBORS_MAX_DISTANCE": _lib.NEIGHBORS_MAX_DISTANCE,
            "CPX_NEIGHBORS_MAX_SCALES": _lib.NEIGHBORS_MAX_SCALES, "CPX_NEIGHBORS_BAND_ROWS": _lib.NEIGHBORS_BAND_ROWS,
            "CPX_NEIGHBORS_SEGMENT_COLS": _lib.NEIGHBORS_SEGMENT_COLS,
            "CPX_NEIGHBORS_MAX_LABEL": _lib.NEIGHBORS_MAX_LABEL}
    assert {k: int(v) for k, v in defs.items()} == want
