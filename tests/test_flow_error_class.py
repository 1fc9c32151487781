"""CPU: cpx_debug_flow_error_class (pure host code, the one definition of the flow-error filter's
mask classes that the classifier kernel, the kernels and the host share) against a Python
restatement of the rule: the register classes as tests/test_gpu_flowerr_reg.py states them, then
the LDS screening class by the grid and unit limits of its kernel (512 threads x 2 units of 12
rows x 2 columns, 20224 cells at an even row stride of bw + 2 columns), the rest oversize."""
import numpy as np

from cpx import _lib

REG1, REG2, REG3, LDS, OVER = range(5)
KS, THREADS, UNITS, CELLS = 12, 512, 2, 20224


def fe_class_ref(bh, bw):
    """The list (0 .. 4) of masks with bboxes bh x bw (arrays or scalars)."""
    bh, bw = np.asarray(bh, np.int64), np.asarray(bw, np.int64)
    mn, mx = np.minimum(bh, bw), np.maximum(bh, bw)
    c1 = (mx <= 64) | ((mn <= 64) & (mx <= 80))
    c2 = ~c1 & (mx <= 128) & (mn <= 80)
    c3 = ~c1 & ~c2 & (mx <= 128) & (mn <= 120)
    stride = (bw + 3) & ~1
    fits = ((bh + 2) * stride <= CELLS) & (((bw + 1) // 2) * ((bh + KS - 1) // KS) <= THREADS * UNITS)
    return np.where(c1, REG1, np.where(c2, REG2, np.where(c3, REG3, np.where(fits, LDS, OVER))))


def test_class_matches_restatement_up_to_320():
    lib = _lib.load()
    n = 320
    bh, bw = np.meshgrid(np.arange(1, n + 1), np.arange(1, n + 1), indexing="ij")
    ref = fe_class_ref(bh, bw)
    got = np.array([[lib.cpx_debug_flow_error_class(h, w) for w in range(1, n + 1)] for h in range(1, n + 1)])
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, [(int(h) + 1, int(w) + 1, int(got[h, w]), int(ref[h, w])) for h, w in bad[:10]]
    # every class occurs, in both orientations where it has two
    for c in (REG1, REG2, REG3, LDS, OVER):
        assert (ref[bh > bw] == c).any() and (ref[bh < bw] == c).any(), c
    # the shapes the GPU tests rely on
    assert fe_class_ref(153, 106) == LDS and fe_class_ref(106, 153) == LDS and fe_class_ref(141, 141) == OVER
