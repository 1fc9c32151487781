"""CPU: the numpy restatement of the Neighbors_* block (tests/neighbors_ref.py) against
scipy.ndimage.binary_dilation with the two structuring elements built as CellProfiler's strel_disk
builds them, against the hand-worked scenes of tests/neighbors_scenes.py and against numpy's
stable argsort."""
import numpy as np
import pytest

import neighbors_ref as nr
import neighbors_scenes as ns


def strel_disk(radius):
    """centrosome.cpmorphology.strel_disk, restated."""
    iradius = int(radius)
    x, y = np.mgrid[-iradius:iradius + 1, -iradius:iradius + 1]
    strel = np.zeros(x.shape, bool)
    strel[x * x + y * y <= radius * radius] = True
    return strel


def test_disks_are_strel_disks():
    for D in range(1, 33):
        for r2, radius in ((D * D, D), (D * D + D, D + 0.5)):
            st = strel_disk(radius)
            mine = np.zeros_like(st)
            for dy, dx in nr.disk_offsets(r2):
                mine[dy + D, dx + D] = True
            assert np.array_equal(st, mine), (D, radius)
    assert strel_disk(1).sum() == 5 and strel_disk(1.5).sum() == 9
    assert max(dy * dy + dx * dx for dy, dx in nr.disk_offsets(30)) == 29  # radius^2 30 at D = 5


@pytest.mark.parametrize("D", [1, 2, 5, 7])
def test_against_binary_dilation(D):
    from scipy.ndimage import binary_dilation
    for seed in (1, 2):
        lab = ns.seeded_blobs(40 + seed, 60, 72, 14, 2, 7) if seed == 1 else ns.seeded_dense(50, 48, 56, 20, 6)
        lab = nr.clean(lab, 32)
        ls, rows = nr.neighbors(lab, 32, (D,))
        assert len(ls) > 8
        for k, L in enumerate(ls):
            grown = binary_dilation(lab == L, structure=strel_disk(D))
            assert rows[k, nr.NUMBER_OF_NEIGHBORS] == len(set(np.unique(lab[grown]).tolist()) - {0, int(L)})
            others = binary_dilation((lab != 0) & (lab != L), structure=strel_disk(D + 0.5))
            edge = nr.edge_mask(lab, L)
            assert edge.sum() > 0
            assert rows[k, nr.PERCENT_TOUCHING] == np.float64((edge & others).sum() * 100) / np.float64(edge.sum())
        assert rows[:, nr.NUMBER_OF_NEIGHBORS].max() > 0


def test_edge_mask_is_the_inner_outline():
    """E_L = L minus its 3 x 3 erosion (the plane's outside eroding too), DESIGN §13."""
    from scipy.ndimage import binary_erosion
    lab = nr.clean(ns.seeded_dense(51, 40, 44, 12, 8), 16)
    for L in np.unique(lab[lab > 0]):
        m = lab == L
        assert np.array_equal(nr.edge_mask(lab, L), m & ~binary_erosion(m, structure=np.ones((3, 3), bool)))


@pytest.mark.parametrize("name", sorted(ns.scenes()))
def test_hand_worked(name):
    lab, ml, scales = ns.scenes()[name]
    ls, rows = nr.neighbors(lab, ml, scales)
    assert rows.shape == (len(ls), 7 * len(scales)) and np.isfinite(rows).all()
    want = sum(1 for h in ns.HAND if h[0] == name)
    assert ns.check_hand(name, ls, rows) == want
    if len(ls) == 1:
        assert (rows == 0).all()
    if len(ls) == 2:
        assert (rows[:, [nr.SECOND_NUMBER, nr.SECOND_DISTANCE, nr.ANGLE]] == 0).all()
    # the closest columns are repeated per scale
    for s in range(1, len(scales)):
        assert np.array_equal(rows[:, 2:7], rows[:, 7 * s + 2:7 * s + 7])
    assert ((rows[:, nr.ANGLE] >= 0) & (rows[:, nr.ANGLE] <= 180)).all()


def test_closest_is_stable_argsort():
    for name in ("ties", "ring", "dense", "d32", "grid"):
        lab, ml, _ = ns.scenes()[name]
        ls, c = nr.centres(nr.clean(lab, ml))
        cl = nr.closest(ls, c)
        for k in range(len(ls)):
            order, d = nr.ranking(c, k)
            ref = np.argsort(d, kind="stable")
            assert list(ref) == order
            assert cl[k, 0] == ls[ref[1]] and cl[k, 1] == d[ref[1]]
            assert cl[k, 2] == ls[ref[2]] and cl[k, 3] == d[ref[2]]
    # the ring's rank 0 is the square that shares its centre, rank 1 the ring itself
    lab, ml, _ = ns.scenes()["ring"]
    ls, c = nr.centres(nr.clean(lab, ml))
    assert c[0].tolist() == c[1].tolist() == [20.0, 20.0]
    assert nr.ranking(c, 1)[0][:2] == [0, 1]


def test_angle_against_arccos():
    """Away from 0 and 180 degrees the atan2 form is CellProfiler's arccos form."""
    lab, ml, scales = ns.scenes()["dense"]
    ls, c = nr.centres(nr.clean(lab, ml))
    cl = nr.closest(ls, c)
    for k in range(len(ls)):
        order, _ = nr.ranking(c, k)
        v1, v2 = c[order[1]] - c[k], c[order[2]] - c[k]
        cos = v1 @ v2 / np.sqrt((v1 @ v1) * (v2 @ v2))
        if abs(cos) < 0.99:
            assert abs(cl[k, 4] - np.degrees(np.arccos(cos))) < 1e-9
