"""GPU: the mask dynamics of cpx_seg_masks (csrc/k_seg.hip: k_dyn_prep, the k_dyn_follow rounds,
k_hist_init, k_seed_flags, k_seed_expand, k_assign, k_relabel_mark / apply, k_apply_newlab,
k_apply_bad) bit-identical to oracle/seg_oracle.py on the edge scenes of tests/seg_scenes.py, whose
preconditions tests/test_seg_scenes_ref.py proves on the CPU:

  big_boundary   a label of exactly 40 % of the plane (kept) and one pixel more (removed, the
                 other label renumbered): the strict `>` of k_relabel_mark
  seed_ties      equal histogram maxima 1, 2, 3, 5 cells apart: both are seeds (k_seed_flags `>=`)
  seed_overlap   two expansions that share four cells: the later seed keeps them (k_seed_expand's
                 atomicMax), the geodesic radius is exactly 5
  thresholds     h == 10 / 11 (seed or not), h == 2 / 3 (expansion), n_moving == 4 / 5 (the `< 5`
                 early-out of k_dyn_follow, k_hist_moving, k_assign) on a 31 x 35 plane (n % 4 ==
                 nh % 4 == 1: the exact counts pass through the scalar branches); seeds of 11 on all
                 four borders, their columns running along the last plane column (the paired
                 gather's right-edge form (x0 - 1, x0): the neighbouring column's field is zero
                 there), the first column and into the first / last row
  plane_edges    trajectories clamped at all four borders and corners: the right-edge form again,
                 the bottom row's bdy == 0, the literal expression for p < 1
  round_edges    niter on and beside every boundary of the follow loop (k0 = 16, sw = 384,
                 sw + k1 = 512, 1176): `steps`, the `last` flag, the ping-pong lists, the fcnt table
  min_size_edge  final objects of 14 and 15 pixels around min_size
  odd_shapes     n % 4 and nh % 4 in {2, 3} at full resolution: the scalar branches of k_hist_init,
                 k_seed_flags, k_apply_newlab, k_apply_bad; FOV 1 and 2 on unaligned bases

Every call is checked for the label image and for the stats rows n_moving, n_seeds_found, n_masks,
n_final and overflow; the FOVs of a scene are run as one batch and one by one; the workspaces of
one Device are reused by smaller calls after larger ones.

Not tested: k_dyn_follow<2, false>, the non-paired gather path (Dx == 1 or >= 2^28 pixels only).
The `< 5` moving-pixel rule is compared through n_moving and the (empty) labels only: no label
image can tell it from `< 4` or `< 6` (tests/test_seg_scenes_ref.py).

Defects found: none, every scene was bit-identical to the oracle as k_seg.hip stood.  That the
scenes can fail was checked once with ten builds of k_seg.hip that differ in one rule each (`>=` at
40 %, `h > 9`, `h > 3`, first writer wins in the expansion, the value of x0 - 1 at the right edge,
one step more in the last round, a wrong element in the scalar branch of k_hist_init, k_seed_flags,
k_apply_newlab and k_apply_bad): each fails tests of this file.
"""
import ctypes as ct
import functools

import numpy as np
import pytest
import torch

import seg_oracle as so
import seg_scenes as sc
from cpx._lib import check
from cpx.device import _ptr
from cpx.segment import SEG_STATS_DTYPE, make_geom

pytestmark = pytest.mark.gpu

ROWS = ("n_moving", "n_seeds_found", "n_masks", "n_final")
THRESHOLDS = (0.0, 0.4)


def _gpu_masks(dev, yf, g, H, W, flow_threshold=0.4, min_size=15, resample=True, niter=None, max_objects=1024):
    """The call of tests/test_gpu_seg.py (_gpu_masks); the outputs start at a sentinel."""
    B = yf.shape[0]
    yft = torch.from_numpy(np.ascontiguousarray(yf)).to(dev.torch_device)
    labels = torch.full((B, H, W), -7, dtype=torch.int32, device=dev.torch_device)
    stats = torch.full((48 * B,), 0xA5, dtype=torch.uint8, device=dev.torch_device)
    check(dev.lib.cpx_seg_masks(dev.h, _ptr(yft), B, ct.c_void_p(ct.addressof(g)), H, W, niter, float(flow_threshold),
                                min_size, max_objects, int(resample), _ptr(labels), _ptr(stats)), "masks")
    dev.sync()
    return labels.cpu().numpy(), stats.cpu().numpy().view(SEG_STATS_DTYPE)


def _niter(geom, call):
    return call.get("niter", so.default_niter(diameter=geom.get("diameter", 100.0),
                                              resample=call.get("resample", True)))


_SCENES = dict(sc.DIRECT_SCENES, round_edges=sc.round_edges)


@functools.lru_cache(maxsize=None)
def _scene(name, *args):
    return (_SCENES[name] if name in _SCENES else sc.odd_shapes)(*args)


@functools.lru_cache(maxsize=None)
def _oracle_rows(name, args, b, extra):
    yf, H, W, geom, call = _scene(name, *args)
    return sc.oracle_rows(yf[b], H, W, **geom, **{**call, **dict(extra)})


@functools.lru_cache(maxsize=None)
def _oracle(name, args, b, flow_threshold, extra):
    """(so.compute_masks labels, stats rows) of FOV b of a scene, computed once per session."""
    yf, H, W, geom, call = _scene(name, *args)
    ref = sc.oracle_labels(yf[b], H, W, flow_threshold, **geom, **{**call, **dict(extra)})
    rows = _oracle_rows(name, args, b, tuple(kv for kv in extra if kv[0] != "min_size"))
    return ref, dict(rows, n_final=int(ref.max()))


def _run(dev, name, args=(), flow_threshold=0.0, fovs=None, **extra):
    """One cpx_seg_masks call on the FOVs `fovs` (default: all) of a scene, checked against the
    oracle; returns the label bits."""
    yf, H, W, geom, call = _scene(name, *args)
    call = {**call, **extra}
    fovs = list(range(yf.shape[0])) if fovs is None else list(fovs)
    got, st = _gpu_masks(dev, yf[fovs], make_geom(H, W, **geom), H, W, flow_threshold=flow_threshold,
                         min_size=call.get("min_size", 15), resample=call.get("resample", True),
                         niter=_niter(geom, call))
    for i, b in enumerate(fovs):
        ref, rows = _oracle(name, tuple(args), b, flow_threshold, tuple(sorted(extra.items())))
        what = f"{name}{tuple(args)} {extra} fov {b} of {fovs} flow_threshold {flow_threshold}"
        mine = {k: int(st[i][k]) for k in ROWS}
        print(what, "gpu", mine, "oracle", rows)
        np.testing.assert_array_equal(got[i], ref, err_msg=what)
        assert mine == rows, what
        assert st[i]["overflow"] == 0, what
    return got


@pytest.mark.parametrize("flow_threshold", THRESHOLDS)
@pytest.mark.parametrize("name", sorted(sc.DIRECT_SCENES))
def test_direct_scene(dev, name, flow_threshold):
    """The scene as one batch, then FOV by FOV: the same bits (per-FOV bases and counters)."""
    batch = _run(dev, name, flow_threshold=flow_threshold)
    if batch.shape[0] > 1:
        for b in range(batch.shape[0]):
            np.testing.assert_array_equal(_run(dev, name, flow_threshold=flow_threshold, fovs=[b])[0], batch[b])
        back = _run(dev, name, flow_threshold=flow_threshold, fovs=range(batch.shape[0] - 1, -1, -1))
        np.testing.assert_array_equal(back[::-1], batch)


def test_scene_conditions_on_the_gpu(dev):
    """The label facts of the scenes, stated once more on the kernel's own output."""
    big = _run(dev, "big_boundary")
    assert np.bincount(big[0].ravel())[1:].tolist() == [1000, 36] and np.bincount(big[1].ravel())[1:].tolist() == [36]
    ties = _run(dev, "seed_ties")
    assert [sorted(np.bincount(t.ravel())[1:].tolist()) for t in ties] == [[194], [97, 97], [97, 97], [97, 97]]
    over = _run(dev, "seed_overlap")
    assert [sorted(np.bincount(t.ravel())[1:].tolist()) for t in over] == [[19, 31], [19, 31]]
    thr = _run(dev, "thresholds")
    assert [int(t.max()) for t in thr] == [2, 2, 0, 0, 4] and (thr[0] > 0).sum() == 2 * 17 and (thr[4] > 0).sum() == 4 * 17
    assert sorted(np.bincount(_run(dev, "plane_edges")[0].ravel())[1:].tolist()) == [64] * 8


@pytest.mark.parametrize("flow_threshold", THRESHOLDS)
@pytest.mark.parametrize("niter", sc.ROUND_NITER)
def test_round_edges(dev, niter, flow_threshold):
    _run(dev, "round_edges", flow_threshold=flow_threshold, niter=niter)


def test_round_edges_differ(dev):
    """One step fewer or more is visible in the kernel's labels at every round boundary."""
    labs = {n: _run(dev, "round_edges", niter=n)[0] for n in sc.ROUND_NITER}
    for N in sc.ROUND_EDGES:
        assert not np.array_equal(labs[N - 1], labs[N]) and not np.array_equal(labs[N], labs[N + 1])
    assert not np.array_equal(labs[1175], labs[1176])


@pytest.mark.parametrize("min_size", [0, 14, 15, 16])
def test_min_size_edge(dev, min_size):
    got = _run(dev, "min_size_edge", min_size=min_size)
    assert sorted(np.bincount(got[0].ravel())[1:].tolist()) == ([14, 15] if min_size <= 14 else [15] if min_size == 15 else [])


@pytest.mark.parametrize("resample", [True, False], ids=["full", "net"])
@pytest.mark.parametrize("shape", sc.ODD_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_odd_shapes(dev, shape, resample):
    """Pixel counts and padded histogram sizes that are no multiples of 4: the batch, then FOV 1
    alone and second in a batch of two (in the batch of three it starts on an unaligned base)."""
    batch = _run(dev, "odd_shapes", (*shape, resample), flow_threshold=0.4)
    assert batch[0].max() >= 4 and batch[1].max() >= 4 and not batch[2].any()
    np.testing.assert_array_equal(_run(dev, "odd_shapes", (*shape, resample), flow_threshold=0.4, fovs=[1])[0], batch[1])
    _run(dev, "odd_shapes", (*shape, resample), flow_threshold=0.4, fovs=[2, 1])


def test_workspace_reuse(dev):
    """Smaller calls after a larger one on the same Device carve the same workspaces differently,
    over what the larger call left there."""
    first = _run(dev, "odd_shapes", (301, 323, True), flow_threshold=0.4)
    _run(dev, "thresholds", flow_threshold=0.4)
    _run(dev, "thresholds")
    _run(dev, "big_boundary", flow_threshold=0.4)
    _run(dev, "round_edges", niter=513)
    _run(dev, "round_edges", niter=16)
    again = _run(dev, "odd_shapes", (301, 323, True), flow_threshold=0.4)
    np.testing.assert_array_equal(again, first)
