"""GPU: the flow-error filter's work lists.  One classifier pass puts every mask of the batch on the
list of its class (cpx_debug_flow_error_class), every kernel claims only its own list, the masks the
fp32 screening leaves undecided and the oversize masks run side by side in one fp64 launch
(k_flow_error_tail), and the fallback kernels return at once on an empty list.  Labels are
bit-identical to the Cellpose restatement (oracle/seg_oracle.py) and the list lengths
(cpx_debug_flow_error_counts) equal the classification of the oracle's masks before the filter.
"""
import ctypes as ct

import numpy as np
import pytest

import seg_oracle as so
import synth_golden as sg
from cpx.segment import make_geom
from test_flow_error_class import LDS, OVER, REG1, REG2, REG3, fe_class_ref
from test_gpu_flowerr_reg import SHAPES, _labels
from test_gpu_seg import _gpu_masks

pytestmark = pytest.mark.gpu


def _counts(dev):
    out = (ct.c_int * 8)()
    assert dev.lib.cpx_debug_flow_error_counts(dev.h, out) == 0
    return np.array(out[:], np.int64)


def _pre_filter_masks(yf, H, W):
    """The oracle's masks before the flow-error filter, and the flows it filters them with."""
    f = so.upsample_flows(yf, H, W)
    p, _ = so.follow_flows(f[:2], f[2] > so.CELLPROB_THRESHOLD, so.default_niter())
    return so.get_masks(p, f[2] > so.CELLPROB_THRESHOLD), f


def _bbox_classes(m):
    cls = []
    for v in range(1, int(m.max()) + 1):
        ys, xs = np.nonzero(m == v)
        if len(ys):
            cls.append(int(fe_class_ref(ys.max() - ys.min() + 1, xs.max() - xs.min() + 1)))
    return np.array(cls, np.int64)


def _flows_of(lab, seed, scales):
    mu = so.masks_to_flows(lab)
    rng = np.random.default_rng(seed)
    scale = np.ones(lab.max() + 1, np.float32)
    scale[1:] = rng.choice(np.float32(scales), lab.max())
    s = scale[lab]
    yf = np.zeros((3,) + lab.shape, np.float32)
    yf[0] = 5.0 * mu[0] * s + 0.02 * rng.standard_normal(lab.shape)
    yf[1] = 5.0 * mu[1] * s + 0.02 * rng.standard_normal(lab.shape)
    yf[2] = np.where(lab > 0, 3.0, -3.0)
    return yf


def test_every_class_in_one_batch(dev):
    """B = 3: the SHAPES ellipses (every register class in both orientations, 153 x 106 for the LDS
    screening, 141 x 141 oversize), an all-background FOV and a FOV with one small mask."""
    H = W = 1040
    g = make_geom(H, W)
    lab0 = _labels(g.Ly, g.Lx, 11)
    assert lab0.max() >= len(SHAPES)
    lab2 = np.zeros((g.Ly, g.Lx), np.int32)
    yy, xx = np.arange(g.Ly)[:, None] - 60, np.arange(g.Lx)[None, :] - 70
    lab2[yy * yy * 25 + xx * xx * 9 <= 225] = 1
    yf = np.stack([_flows_of(lab0, 11, [0.33, 0.37, 0.40, 0.6, 1.0]),
                   np.full((3, g.Ly, g.Lx), -1.0, np.float32),
                   _flows_of(lab2, 3, [1.0])])
    want = np.zeros(5, np.int64)
    for b in range(3):
        cls = _bbox_classes(_pre_filter_masks(yf[b], H, W)[0])
        want += np.bincount(cls, minlength=5)
        if b == 0:
            assert all((cls == c).any() for c in (REG1, REG2, REG3, LDS, OVER)), np.bincount(cls, minlength=5)
        else:
            assert len(cls) == b // 2
    refs = [so.compute_masks(yf[b], H, W) for b in range(3)]
    assert refs[0].max() >= 4 and refs[1].max() == 0 and refs[2].max() == 1
    got, st = _gpu_masks(dev, yf, g, H, W)
    c = _counts(dev)
    print("lists (reg1, reg2, reg3, LDS, oversize, undecided, fallback):", c[:7], "removed:", st["n_bad_flow"])
    for b in range(3):
        np.testing.assert_array_equal(got[b], refs[b], err_msg=f"fov {b}")
    np.testing.assert_array_equal(c[:5], want)
    assert 0 <= c[5] <= want[:4].sum() and 0 <= c[6] <= want[4] and c[7] == 0
    assert st["n_bad_flow"].sum() >= 2 and (st["overflow"] == 0).all()
    # the same batch again on the same context: the lists start empty again
    got2, _ = _gpu_masks(dev, yf, g, H, W)
    np.testing.assert_array_equal(got2, got)
    np.testing.assert_array_equal(_counts(dev), c)


def test_undecided_and_oversize_masks_share_the_tail_launch(dev):
    """Thresholds 1e-7 either side of the fp64 error of the largest mask beyond the register
    classes: the screening must defer, and the same call has oversize masks, so both bodies of the
    fp64 tail run in one launch."""
    H, W = 1400, 1400
    g = make_geom(H, W)
    lab = sg.labels(7, g.Ly, g.Lx, n=14, rmin=6, rmax=24, skip_every=0)
    mu = so.masks_to_flows(lab)
    rng = np.random.default_rng(7)
    yf = np.zeros((3, g.Ly, g.Lx), np.float32)
    yf[0] = 5.0 * mu[0] * 0.37 + 0.02 * rng.standard_normal((g.Ly, g.Lx))
    yf[1] = 5.0 * mu[1] * 0.37 + 0.02 * rng.standard_normal((g.Ly, g.Lx))
    yf[2] = np.where(lab > 0, 3.0, -3.0)
    m, f = _pre_filter_masks(yf, H, W)
    err = so.flow_errors(m, f[:2])
    cls = _bbox_classes(m)
    assert len(cls) == len(err) == m.max()
    area = np.bincount(m.ravel(), minlength=len(err) + 1)[1:]
    beyond = np.nonzero(cls >= LDS)[0]
    assert len(beyond) >= 1 and (cls == OVER).any()
    k = beyond[np.argmax(area[beyond])]
    for d in (-1e-7, 1e-7):
        thr = float(err[k] + d)
        got, st = _gpu_masks(dev, yf[None], g, H, W, flow_threshold=thr)
        c = _counts(dev)
        print(f"mask {k + 1} (class {cls[k]}, area {area[k]}) threshold {thr}: lists", c[:7])
        ref = so.compute_masks(yf, H, W, flow_threshold=thr)
        np.testing.assert_array_equal(got[0], ref, err_msg=f"mask {k + 1} threshold {thr}")
        np.testing.assert_array_equal(c[:5], np.bincount(cls, minlength=5))
        assert c[5] >= 1 and c[4] >= 1, c


def test_empty_lists(dev):
    """No mask at all: every kernel sees empty lists."""
    H, W = 700, 760
    g = make_geom(H, W)
    yf = np.full((1, 3, g.Ly, g.Lx), -1.0, np.float32)
    got, st = _gpu_masks(dev, yf, g, H, W)
    assert not got.any() and st[0]["n_final"] == 0 and st[0]["overflow"] == 0
    assert not _counts(dev).any()
