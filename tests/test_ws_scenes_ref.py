"""CPU: the watershed edge-case scenes (tests/ws_scenes.py) are what they claim to be, so a GPU
mismatch on them (tests/test_gpu_watershed_edges.py) is a kernel bug and not a scene artefact: the
footprints, the label shares, the heap flood against the minimax form, and the Jacobi tile model
whose round count bounds the relax rounds the kernel may use.
"""
import numpy as np
import pytest

import cpx_oracle as orc
import ws_oracle as wo
import ws_scenes as sc

API_ROUNDS = 64  # cpx_watershed_cells: relax_rounds, label_rounds <= 64


def _flood_forms(nuc, corr, d):
    """(footprint, heap-flood Cells, minimax Cells, minimax levels B) of one FOV."""
    foot = orc.expand_labels(nuc, d) > 0
    key = wo.elevation_key(corr)
    heap, _ = wo.cells_watershed(nuc, corr, d, impl="py")
    mm, info = wo.watershed_minimax(key, nuc, foot, return_info=True)
    return foot, heap, mm, info["B"]


@pytest.mark.parametrize("name", sorted(sc.ROUND_SCENES))
def test_serpentine_preconditions(name):
    H, W, pitch, seed = sc.ROUND_SCENES[name]
    nuc, corr, d = sc.serpentine(H, W, pitch, seed)
    assert d == 127 and nuc[0, 0] == 7 and (nuc == 3).sum() == 1
    wall = corr <= 5000
    assert ((corr >= 100) & wall | (corr >= 50000) & (corr <= 60000)).all()
    assert not wall[::pitch].any() and wall[1:pitch, 1:W - 1].all()  # corridor rows, walls between
    foot, heap, mm, B = _flood_forms(nuc, corr, d)
    assert foot.all()
    for lab in (7, 3):
        assert (heap == lab).sum() >= 0.05 * H * W, (lab, (heap == lab).sum())
    np.testing.assert_array_equal(mm, heap)
    np.testing.assert_array_equal(heap, wo.cells_watershed(nuc, corr, d, impl="c")[0])
    rounds, L = sc.jacobi_tile_rounds(nuc, corr, d, return_levels=True)
    print(name, "Jacobi tile rounds:", rounds, "pixels of 7 / 3:", (heap == 7).sum(), (heap == 3).sum())
    assert rounds <= API_ROUNDS
    if pitch == 4:
        assert rounds > 8
    free = foot & (nuc == 0)
    np.testing.assert_array_equal(L[free], B[free])


def test_serpentine_centre_marker():
    """A wall pixel at the plane centre carries the largest label the packed expand pass keeps."""
    nuc, corr, d = sc.serpentine(70, 100, 3, 2)
    assert nuc[35, 50] == sc.BIG_LABEL and corr[35, 50] <= 5000
    cells = wo.cells_watershed(nuc, corr, d)[0]
    assert cells[35, 50] == sc.BIG_LABEL and set(np.unique(cells)) == {3, 7, sc.BIG_LABEL}


def test_jacobi_model_is_one_round_on_one_tile():
    """Within one tile the model is the plain fixed point: a changing round and the confirming one."""
    nuc, corr = sc.heavy_ties(32, 32, 4)
    rounds, L = sc.jacobi_tile_rounds(nuc, corr, 127, return_levels=True)
    assert rounds == 2
    foot, heap, mm, B = _flood_forms(nuc, corr, 127)
    free = foot & (nuc == 0)
    assert free.any()
    np.testing.assert_array_equal(L[free], B[free])


def _cells_with_q(nuc, q, d):
    """The heap flood with another quantisation q of the cell channel."""
    H, W = nuc.shape
    idx = np.arange(H * W, dtype=np.uint64).reshape(H, W)
    key = ((np.uint64(65535) - q.astype(np.uint64)) << np.uint64(wo.KEY_SHIFT)) | idx
    return wo.watershed(key.astype(np.float64), nuc, orc.expand_labels(nuc, d) > 0)


def _wrong_quantisations(corr):
    """Plausible mistakes in q16, each on one class of special value."""
    q = wo.quantise(corr).astype(np.float64)
    fin = np.isfinite(corr)
    with np.errstate(invalid="ignore"):
        return {
            "NaN -> 0": np.where(np.isnan(corr), 0, q),
            "+inf -> 0": np.where(np.isposinf(corr), 0, q),
            "-inf -> 65535": np.where(np.isneginf(corr), 65535, q),
            "finite >= 65535 -> 0": np.where(fin & (corr >= 65535), 0, q),
            "negative -> |v|": np.where(fin & (corr < 0), np.minimum(np.abs(corr), 65535), q),
            "rounding": np.where(fin & (corr > 0) & (corr < 65535), np.minimum(np.rint(corr), 65535), q),
        }


@pytest.mark.parametrize("d", [15, 127])
def test_special_values_decide_labels(d):
    """The reference labels change under every wrong quantisation: the scene would notice it."""
    nuc, corr, _ = sc.special_values(70, 100, sc.SPECIAL_SEED, d)
    ref = wo.cells_watershed(nuc, corr, d)[0]
    np.testing.assert_array_equal(_cells_with_q(nuc, wo.quantise(corr), d), ref)
    for name, q in _wrong_quantisations(corr).items():
        assert (_cells_with_q(nuc, q, d) != ref).sum() >= 100, name


@pytest.mark.parametrize("direction", sc.ONE_WAY)
def test_one_way_preconditions(direction):
    nuc, corr, d = sc.one_way(direction)
    H, W = nuc.shape
    assert (H, W) in ((97, 20), (20, 97)) and (nuc > 0).sum() == 2
    ys, xs = np.nonzero(nuc)
    end = {"down": ys.max() == 0, "up": ys.min() == H - 1, "right": xs.max() == 0, "left": xs.min() == W - 1}
    assert end[direction]
    foot, heap, mm, _ = _flood_forms(nuc, corr, d)
    assert foot.all() and (heap > 0).all()
    np.testing.assert_array_equal(mm, heap)
    far = {"down": heap[-sc.TILE:], "up": heap[:sc.TILE], "right": heap[:, -sc.TILE:], "left": heap[:, :sc.TILE]}
    assert (far[direction] > 0).all()  # an unflooded far tile would show


def test_special_values_preconditions():
    H, W = 70, 100
    nuc, corr, d = sc.special_values(H, W, sc.SPECIAL_SEED)
    foot, heap, mm, _ = _flood_forms(nuc, corr, d)
    free = foot & (nuc == 0)
    assert 4 <= len(np.unique(nuc[nuc > 0])) <= 7
    for v in sc.SPECIAL:
        assert (sc.same_value(corr, v) & free).any(), v
    assert len(sc.SPECIAL) == 15 and sc.SUBNORMAL > 0 and sc.SUBNORMAL < np.finfo(np.float32).tiny
    # the values cross every branch of q16: the clamp from both sides, truncation, <= 0, NaN
    np.testing.assert_array_equal(wo.quantise(sc.SPECIAL),
                                  [65535, 65535, 0, 0, 0, 0, 0, 0, 1, 65534, 65535, 65535, 0, 1000, 2000])
    np.testing.assert_array_equal(mm, heap)
    assert (heap[free] > 0).any() and not foot.all()


def test_plateau_preconditions():
    H, W = 97, 131
    nuc, corr, d = sc.plateau(H, W)
    assert (nuc > 0).sum() == 2 and nuc[0, 0] and nuc[-1, -1] and (corr == corr[0, 0]).all()
    foot, heap, mm, _ = _flood_forms(nuc, corr, d)
    assert foot.all()
    assert set(np.unique(heap)) == {1, 2}
    np.testing.assert_array_equal(mm, heap)
    key = wo.elevation_key(corr)
    np.testing.assert_array_equal(np.diff(key.ravel()), 1)  # the raster index is the whole order


def test_dense_lattice_preconditions():
    nuc, corr, d = sc.dense_lattice()
    assert nuc.shape == (sc.TILE, sc.TILE) and d == 2
    mark = nuc > 0
    assert mark.sum() == 205 and (~mark).sum() == 819
    assert len(np.unique(nuc[mark])) == 205
    pad = np.pad(mark, 1)
    touch = pad[:-2, 1:-1] | pad[2:, 1:-1] | pad[1:-1, :-2] | pad[1:-1, 2:]
    free = ~mark
    assert touch[1:-1, 1:-1][free[1:-1, 1:-1]].all() and (free & touch).sum() == 794
    assert (np.diff(corr[mark]) < 0).all()  # boolean indexing is raster order
    foot, heap, mm, _ = _flood_forms(nuc, corr, d)
    assert foot.all() and (heap > 0).all()
    np.testing.assert_array_equal(mm, heap)


@pytest.mark.parametrize("shape", sc.BATCH_SHAPES)
def test_batch_mixed_preconditions(shape):
    H, W = shape
    nuc, corr, d = sc.batch_mixed(H, W)
    assert nuc.shape == corr.shape == (5, H, W) and nuc.dtype == np.int32 and corr.dtype == np.float32
    for b in range(4):
        assert not np.array_equal(nuc[b], nuc[b + 1])
        assert not np.array_equal(corr[b], corr[b + 1], equal_nan=True)
    assert not nuc[1].any()
    assert (nuc[2] > 0).all() and len(np.unique(nuc[2])) >= 4
    assert (nuc[0] == sc.BIG_LABEL).sum() == 1
    np.testing.assert_array_equal(nuc[4], nuc[0, ::-1, ::-1])
    np.testing.assert_array_equal(corr[4], corr[0, ::-1, ::-1])
    for b in (0, 3, 4):
        foot, heap, mm, _ = _flood_forms(nuc[b], corr[b], d)
        assert foot.all()
        np.testing.assert_array_equal(mm, heap)
        rounds = sc.jacobi_tile_rounds(nuc[b], corr[b], d)
        print(shape, "fov", b, "Jacobi tile rounds:", rounds)
        assert rounds <= API_ROUNDS
    free = nuc[3] == 0
    for v in sc.SPECIAL:
        assert (sc.same_value(corr[3], v) & free).any(), v
