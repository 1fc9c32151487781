"""GPU: cpx_watershed_cells (k_watershed.hip, with the ring pass of k_expand.hip) bit-identical
to the sequential heap flood (oracle/ws_oracle.py cells_watershed) off the shapes, distance and
round settings of tests/test_gpu_watershed.py: planes of 1 to 20 tiles with 1-pixel partial tiles,
distances 0..127, a workspace left by another geometry, round budgets that are too small (status
-1 or exact labels, never silently wrong), NaN / inf / negative / clamped elevations, a plateau, the
densest seeding of one tile, mixed batches and the argument checks.  The scenes and their
preconditions: tests/ws_scenes.py, tests/test_ws_scenes_ref.py.
"""
import functools

import numpy as np
import pytest
import torch

import cpx_oracle as orc
import ws_oracle as wo
import ws_scenes as sc
from cpx._lib import CPX_OK
from cpx.device import _ptr

pytestmark = pytest.mark.gpu

CPX_ERR_ARG = 1  # include/cpx.h
FULL = (64, 64)  # the API's cap on relax / label rounds


def _ws_call(dev, nuc, corr, ch, d, rounds=FULL, shape=None):
    """Raw call (as tests/test_gpu_watershed.py _ws_gpu): (rc, cells, cyto, status); outputs start
    at the sentinel -7.  `shape` overrides the (H, W) passed to the library."""
    B, C, H, W = corr.shape
    td = dev.torch_device
    t_n = torch.from_numpy(np.ascontiguousarray(nuc, np.int32)).to(td)
    t_c = torch.from_numpy(np.ascontiguousarray(corr, np.float32)).to(td)
    cells = torch.full_like(t_n, -7)
    cyto = torch.full_like(t_n, -7)
    status = torch.full((B, 8), -7, dtype=torch.int32, device=td)
    if shape is not None:
        H, W = shape
    rc = dev.lib.cpx_watershed_cells(dev.h, _ptr(t_n), _ptr(t_c), B, C, ch, H, W, d, rounds[0], rounds[1],
                                     _ptr(cells), _ptr(cyto), _ptr(status), 8)
    dev.sync()
    return rc, cells.cpu().numpy(), cyto.cpu().numpy(), status[:, 0].cpu().numpy()


def _ws_gpu(dev, nuc, corr, ch, d, rounds=FULL):
    rc, cells, cyto, st = _ws_call(dev, nuc, corr, ch, d, rounds)
    assert rc == CPX_OK, rc
    return cells, cyto, st


def _ref(nuc, corr, d):
    return [wo.cells_watershed(nuc[b], corr[b], d) for b in range(nuc.shape[0])]


def _check_exact(nuc, d, ref, cells, cyto, st, what):
    """Every FOV converged (status >= 100 exactly when it has free pixels) and equals the flood."""
    for b in range(nuc.shape[0]):
        free = (nuc[b] == 0) & (orc.expand_labels(nuc[b], d) > 0)
        assert st[b] >= 0 and (st[b] >= 100) == bool(free.any()), (what, b, st.tolist())
        np.testing.assert_array_equal(cells[b], ref[b][0], err_msg=f"{what} fov {b} cells")
        np.testing.assert_array_equal(cyto[b], ref[b][1], err_msg=f"{what} fov {b} cyto")


def _run_exact(dev, nuc, corr, d, what, rounds=FULL):
    """nuc [B, H, W], corr [B, H, W] (one channel) -> checked against the flood; returns the bits."""
    cells, cyto, st = _ws_gpu(dev, nuc, corr[:, None], 0, d, rounds)
    _check_exact(nuc, d, _ref(nuc, corr, d), cells, cyto, st, what)
    return cells, cyto, st


SHAPES = [(1, 1), (1, 70), (70, 1), (31, 31), (32, 32), (33, 33), (32, 65), (97, 131), (64, 96)]
DISTANCES = (0, 1, 2, 15, 127)


def _distances(H, W):
    """The distances whose footprint can differ (one past the plane's diagonal adds nothing), and
    always 127: a window wider than the plane is a path of its own in the expand pass."""
    out = []
    for d in DISTANCES:
        if out and out[-1] >= np.hypot(H - 1, W - 1):
            break
        out.append(d)
    return out if out[-1] == 127 else out + [127]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_geometry(dev, shape):
    """1 to 20 tiles (below the 8 XCD ranges, no multiple of the 4 / 16 tile shares), 1-pixel
    partial tiles on either axis, distances from 0 to beyond the plane; heavy-tie elevations."""
    H, W = shape
    for seed in (0, 1):
        nuc, corr = sc.heavy_ties(H, W, 100 * H + W + seed)
        for d in _distances(H, W):
            cells, cyto, st = _run_exact(dev, nuc[None], corr[None], d, f"{shape} seed {seed} d {d}")
            if d == 0:
                np.testing.assert_array_equal(cells[0], nuc)
                assert not cyto.any() and st[0] >= 0


def test_geometry_distances_kept():
    assert _distances(1, 1) == [0, 127] and _distances(1, 70) == [0, 1, 2, 15, 127]
    assert _distances(31, 31) == [0, 1, 2, 15, 127] and _distances(2, 2) == [0, 1, 2, 127]


def test_stale_workspace(dev):
    """The ring, level, flag and list buffers of one Device, filled by a 97 x 131 batch of three,
    are then read with other tile geometries: every call exact, a repeated call the same label bits
    (the status word's round counts may differ between calls: a tile may read a neighbour's ring of
    this round or of the last, a jump a label written in the same round)."""
    calls = [((3, 97, 131), 127), ((1, 33, 33), 15), ((2, 31, 65), 127), ((1, 33, 33), 15)]
    for k, ((B, H, W), d) in enumerate(calls):
        fovs = [sc.heavy_ties(H, W, 40 + 7 * k + b) for b in range(B)]
        nuc, corr = np.stack([f[0] for f in fovs]), np.stack([f[1] for f in fovs])
        first = _run_exact(dev, nuc, corr, d, f"call {k}")
        again = _run_exact(dev, nuc, corr, d, f"call {k} repeated")
        for a, b in zip(first[:2], again[:2]):
            np.testing.assert_array_equal(a, b)


@functools.lru_cache(maxsize=None)
def _round_scenes():
    names = sorted(sc.ROUND_SCENES)
    fovs = [sc.serpentine(*sc.ROUND_SCENES[n]) for n in names]
    nuc, corr = np.stack([f[0] for f in fovs]), np.stack([f[1] for f in fovs])
    jac = [sc.jacobi_tile_rounds(f[0], f[1], f[2]) for f in fovs]
    return names, nuc, corr, _ref(nuc, corr, 127), jac


def test_round_budget_never_silently_wrong(dev):
    """The 96 x 96 serpentines (the corridor crosses a tile per relax round): whatever the budget,
    a FOV is either failed (-1) or exact; one relax round cannot see across a tile edge; the full
    budget converges within the Jacobi tile model's rounds (tests/ws_scenes.py)."""
    names, nuc, corr, ref, jac = _round_scenes()
    budgets = [(r, 64) for r in (1, 2, 4, 8, 16, 32, 64)] + [(64, r) for r in (1, 2, 4, 8)]
    for rounds in budgets:
        cells, cyto, st = _ws_gpu(dev, nuc, corr[:, None], 0, 127, rounds)
        print("rounds", rounds, "status", dict(zip(names, st.tolist())), "Jacobi", jac)
        for b, n in enumerate(names):
            assert st[b] == -1 or st[b] > 0, (n, rounds, st.tolist())
            if st[b] > 0:
                np.testing.assert_array_equal(cells[b], ref[b][0], err_msg=f"{n} {rounds}")
                np.testing.assert_array_equal(cyto[b], ref[b][1], err_msg=f"{n} {rounds}")
                assert st[b] // 100 <= min(rounds[0], jac[b]), (n, rounds, st.tolist(), jac)
                assert st[b] % 100 <= rounds[1]
            if rounds[0] == 1:
                assert st[b] == -1, (n, st.tolist())
            if rounds == (64, 64):
                assert st[b] > 0, (n, st.tolist())


@pytest.mark.parametrize("d", [15, 127])
def test_special_elevations(dev, d):
    """NaN, +-inf, negative, -0.0, subnormal, fractional and clamped elevations on channel 1 of 2
    (a wrong quantisation of any of them changes the labels: tests/test_ws_scenes_ref.py)."""
    H, W = 70, 100
    nuc, corr, d = sc.special_values(H, W, sc.SPECIAL_SEED, d)
    planes = np.random.default_rng(1).uniform(0, 6e4, (1, 2, H, W)).astype(np.float32)
    planes[0, 1] = corr
    cells, cyto, st = _ws_gpu(dev, nuc[None], planes, 1, d)
    _check_exact(nuc[None], d, _ref(nuc[None], corr[None], d), cells, cyto, st, "special_values")
    assert st[0] >= 100


@pytest.mark.parametrize("direction", sc.ONE_WAY)
def test_one_way_flow(dev, direction):
    """Four tiles in a line, markers at one end: every tile but the first is woken by one kind of
    neighbour flag alone (a dropped kUp / kDown / kLeft / kRight leaves the rest unflooded)."""
    nuc, corr, d = sc.one_way(direction)
    _run_exact(dev, nuc[None], corr[None], d, f"one way {direction}")


def test_plateau(dev):
    nuc, corr, d = sc.plateau(97, 131)
    _, _, st = _run_exact(dev, nuc[None], corr[None], d, "plateau")
    print("plateau status", st.tolist())


def test_dense_lattice(dev):
    nuc, corr, d = sc.dense_lattice()
    _, _, st = _run_exact(dev, nuc[None], corr[None], d, "dense_lattice")
    assert st[0] >= 100


@pytest.mark.parametrize("shape", sc.BATCH_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_batch_mixed(dev, shape):
    """Serpentine, blank, all-nuclei, special-value and turned FOVs in one batch: the last tile of a
    FOV and the first of the next never exchange halos or flags."""
    nuc, corr, d = sc.batch_mixed(*shape)
    cells, cyto, st = _run_exact(dev, nuc, corr, d, f"batch {shape}")
    print("batch", shape, "status", st.tolist())
    assert (cells != -7).all() and (cyto != -7).all() and (st != -7).all()
    assert not cells[1].any() and not cyto[1].any() and st[1] >= 0
    np.testing.assert_array_equal(cells[2], nuc[2])
    assert not cyto[2].any()
    assert st[0] >= 100 and st[3] >= 100 and st[4] >= 100


def test_arguments(dev):
    """Bad arguments are CPX_ERR_ARG before any launch, and the next call is right."""
    nuc, corr = sc.heavy_ties(33, 40, 9)
    nuc, corr = nuc[None], corr[None, None]
    ref = _ref(nuc, corr[:, 0], 15)

    def good():
        cells, cyto, st = _ws_gpu(dev, nuc, corr, 0, 15)
        _check_exact(nuc, 15, ref, cells, cyto, st, "after an error")

    good()
    bad = [dict(rounds=(0, 16)), dict(rounds=(65, 16)), dict(rounds=(16, 0)), dict(ch=1), dict(d=128),
           dict(shape=(4096, 2049))]  # H * W = 2^23 + 4096: refused on the sizes alone (tiny buffers)
    for kw in bad:
        rc, cells, cyto, st = _ws_call(dev, nuc, corr, kw.get("ch", 0), kw.get("d", 15),
                                       kw.get("rounds", (16, 16)), kw.get("shape"))
        assert rc == CPX_ERR_ARG, (kw, rc)
        assert (cells == -7).all() and (cyto == -7).all() and (st == -7).all(), kw
        good()
