"""GPU: the step loop of k_dyn_follow (csrc/k_seg.hip) bit-identical to oracle/seg_oracle.py on the
scenes of tests/follow_scenes.py, whose preconditions tests/test_follow_scenes_ref.py proves on the
CPU:

  pair_counts   256 / 257 / 512 / 513 moving pixels: no thread, one thread, every thread of a block
                and one thread of the next block has a second item
  partners      items i and i + 256 of one thread that differ: one on its fixed point after step 1
                and one that runs through every round; one in the literal top / left expression and
                one in the fast one; one that stays in a cell (no gather) while the other gathers at
                every step, either way round
  returning     trajectories that leave a cell and come back to it (the kept taps are of the cell
                they are in, not of an earlier visit)
  buffer_edges  trajectories that end on the last column, the last row and the plane's last pixel
                (the 16-byte gather ends with the field), for Dx 2, 34 and 35, as the last FOV of a
                batch and with another FOV behind; NaN in the column beside the last one (flow
                threshold 0 only): the clamped tap is the pixel itself, not its neighbour at weight 0
  scalar_path   Dx == 1, k_dyn_follow<2, false>

Every call is checked for the label image and the stats rows n_moving, n_seeds_found, n_masks,
n_final and overflow, the FOVs of a scene as one batch and one by one; a small call follows a large
one on the same Device.
"""
import ctypes as ct
import functools

import numpy as np
import pytest
import torch

import follow_scenes as fs
import seg_scenes as sc
from cpx._lib import check
from cpx.device import _ptr
from cpx.segment import SEG_STATS_DTYPE, make_geom

pytestmark = pytest.mark.gpu

ROWS = ("n_moving", "n_seeds_found", "n_masks", "n_final")
MIN_SIZE = 15


def _gpu_masks(dev, yf, H, W, geom, flow_threshold):
    B = yf.shape[0]
    g = make_geom(H, W, **geom)
    yft = torch.from_numpy(np.ascontiguousarray(yf)).to(dev.torch_device)
    labels = torch.full((B, H, W), -7, dtype=torch.int32, device=dev.torch_device)
    stats = torch.full((48 * B,), 0xA5, dtype=torch.uint8, device=dev.torch_device)
    check(dev.lib.cpx_seg_masks(dev.h, _ptr(yft), B, ct.c_void_p(ct.addressof(g)), H, W, fs.NITER,
                                float(flow_threshold), MIN_SIZE, 1024, 1, _ptr(labels), _ptr(stats)), "masks")
    dev.sync()
    return labels.cpu().numpy(), stats.cpu().numpy().view(SEG_STATS_DTYPE)


@functools.lru_cache(maxsize=None)
def _scene(name):
    return fs.SCENES[name]()


@functools.lru_cache(maxsize=None)
def _oracle(name, b, flow_threshold):
    """(so.compute_masks labels, stats rows) of FOV b of a scene, computed once per session."""
    yf, H, W, geom, call = _scene(name)
    ref = sc.oracle_labels(yf[b], H, W, flow_threshold, **geom, **call)
    return ref, dict(sc.oracle_rows(yf[b], H, W, **geom, **call), n_final=int(ref.max()))


def _run(dev, name, flow_threshold=0.0, fovs=None):
    yf, H, W, geom, _ = _scene(name)
    fovs = list(range(yf.shape[0])) if fovs is None else list(fovs)
    got, st = _gpu_masks(dev, yf[fovs], H, W, geom, flow_threshold)
    for i, b in enumerate(fovs):
        ref, rows = _oracle(name, b, flow_threshold)
        what = f"{name} fov {b} of {fovs} flow_threshold {flow_threshold}"
        mine = {k: int(st[i][k]) for k in ROWS}
        print(what, "gpu", mine, "oracle", rows)
        np.testing.assert_array_equal(got[i], ref, err_msg=what)
        assert mine == rows, what
        assert st[i]["overflow"] == 0, what
    return got


def _thresholds(name):
    return (0.0,) if "nan" in name else (0.0, 0.4)


@pytest.mark.parametrize("name", sorted(fs.SCENES))
def test_scene(dev, name):
    """The scene as one batch, then FOV by FOV, then the batch in reverse order (every FOV once
    last in the batch and once with another behind it)."""
    for ft in _thresholds(name):
        batch = _run(dev, name, ft)
        B = batch.shape[0]
        if B > 1:
            for b in range(B):
                np.testing.assert_array_equal(_run(dev, name, ft, fovs=[b])[0], batch[b])
            back = _run(dev, name, ft, fovs=range(B - 1, -1, -1))
            np.testing.assert_array_equal(back[::-1], batch)


def test_scene_facts_on_the_gpu(dev):
    """The label facts of the scenes, stated once more on the kernel's own output."""
    def sizes(lab):
        return sorted(np.bincount(lab.ravel())[1:].tolist())
    assert sizes(_run(dev, "pair_counts_257")[0]) == [40, 108, 108]
    assert sizes(_run(dev, "pair_counts_513")[0]) == [81, 108, 108, 108, 108]
    assert [len(sizes(lab)) for lab in _run(dev, "partners")] == [3, 3]
    assert sizes(_run(dev, "buffer_edges_35")[0]) == [15, 15, 15]
    assert sizes(_run(dev, "buffer_edges_2")[0]) == [15, 15]
    assert sizes(_run(dev, "scalar_path")[0]) == [15, 15]


def test_workspace_reuse(dev):
    """Small calls after a larger one on the same Device carve the same workspaces differently,
    over what the larger call left there (positions, item lists, round counters)."""
    first = _run(dev, "partners", 0.4)
    _run(dev, "scalar_path")
    _run(dev, "buffer_edges_2", 0.4)
    _run(dev, "pair_counts_257")
    _run(dev, "returning", 0.4)
    np.testing.assert_array_equal(_run(dev, "partners", 0.4), first)
