"""GPU: the feature kernels (k_obj_stage, k_shape_props, k_tex_band, k_tex_glcm, k_glcm_props and
the fallbacks k_shape / k_intensity_texture) against the exact reference (tests/features_exact.py)
on the edge-case scenes of tests/feature_scenes.py — objects smaller than the GLCM offsets,
objects on the plane's first and last pixels with another FOV / channel behind them, exactly
symmetric objects, rings and multi-component labels, every row-width residue, pair counters near
65,535, |i - j| at the band edge, outlier lists at their cap, bboxes on either side of every
staging limit, and intensities whose variance is tiny beside the square of their mean.

tests/test_features_exact_ref.py (CPU) asserts that each scene is what it claims to be.  The
comparator checks every column by its class (features_exact.compare; DESIGN.md, parity section):
integer-derived columns at 1e-12 / 1e-9, sums by the any-order bound, StdIntensity at the
project's promise of rel 1e-5, abs 1e-9.

StdIntensity of the `intensity` scene measured on an MI355X (relative error against the two-pass
fsum reference; the two objects at 70000 +- 3 ulp have Std 0.01575 and 0.01545):

                                              70000 +- 3 ulp          constant 200 x 200 / 260 x 262
    var = (sum v^2 - (sum v)^2 / n) / n       1.3e-3, 4.6e-4          Std 8.8e-4 / 0 (by luck of the order)
    var from d = v - pivot (now)              0, 1.1e-16              exactly 0 / exactly 0

A later session that wants a tighter StdIntensity assertion than the promise has four to five
decades of room on these inputs.

The scenes also exposed a second defect, fixed with them: for a bbox whose width is 1, 2 or 3
modulo 8, k_obj_stage counted the row padding's 4-pixel group as 15 valid pixels (a negative count
shifted into four bits), so the padding's non-members put a 0 into the scale_to_8bit range.  A crop
with a masked pixel or a value <= 0 has that 0 anyway; an object that fills its bbox (`tiny`,
`widths`, channel 1 of `counters`) was quantised over [0, max] instead of [min, max] and every
texture column was wrong (Contrast 2304 where the reference has 8100).
"""
import numpy as np
import pytest
import torch

import feature_scenes as fs
import features_exact as fx
from cpx.device import as_numpy, n_features

pytestmark = pytest.mark.gpu

MAX_LABEL = 32


def _tables(dev, labs):
    from test_gpu_parity import _objects
    labt, obj, hdr, _, h = _objects(dev, labs, max_label=MAX_LABEL)
    return labt, obj, hdr, [int(x) for x in h["n_objects"]]


def _run(dev, labs, planes):
    """dev.features on labels [B, H, W], planes [B, C, H, W]: one [n_objects, F] array per FOV."""
    B, C = planes.shape[:2]
    labt, obj, hdr, n = _tables(dev, labs)
    feats = torch.zeros((B, MAX_LABEL, n_features(C)), dtype=torch.float64, device=dev.torch_device)
    corr = torch.from_numpy(np.ascontiguousarray(planes)).to(dev.torch_device)
    dev.features(labt, corr, C, MAX_LABEL, obj, hdr, feats)
    dev.sync()
    got = feats.cpu().numpy()
    return [got[b, :n[b]] for b in range(B)]


def _fold(worst, w):
    for k, v in w.items():
        worst[k] = max(worst.get(k, 0.0), v)


@pytest.mark.parametrize("name", fs.SCENES)
def test_scene_matches_exact_reference(dev, name):
    labs, planes = fs.scene(name)
    ref = fs.exact(name)
    got = _run(dev, labs, planes)
    worst = {}
    for b, (rows, diags) in enumerate(ref):
        _fold(worst, fx.compare(got[b], rows, diags, f"{name} FOV {b}"))
    print(name, "largest error per column class:", {k: float(f"{v:.3g}") for k, v in worst.items()})
    if name in fs.TWICE_SCENES:
        # again on the same context: the redo list, the queue and outlier counters start from zero
        again = _run(dev, labs, planes)
        for a, g in zip(again, got):
            np.testing.assert_array_equal(a, g)


def test_intensity_scene_std_figures(dev):
    """The figures of the module docstring: StdIntensity of the constant and the near-constant
    objects (printed; asserted by test_scene_matches_exact_reference[intensity])."""
    labs, planes = fs.scene("intensity")
    got = _run(dev, labs, planes)
    o = fx.N_SHAPE + 2
    for b, (rows, diags) in enumerate(fs.exact("intensity")):
        for k, d in enumerate(diags):
            g, r = got[b][k, o], rows[k, o]
            print(f"intensity FOV {b} label {d['label']} n {d['n']}: Std got {g!r} ref {r!r} "
                  f"rel {abs(g - r) / r if r else abs(g):.3g}")
    assert got[0][0, o] == 0.0 and got[1][0, o] == 0.0  # a constant object: exactly 0


@pytest.mark.parametrize("name", fs.PAIR_SCENES)
def test_pair_path_bit_identical_and_exact(dev, name):
    """Cells = the scene's objects dilated, Cytoplasm = Cells minus the objects: cpx_features_pair
    equals two cpx_features calls bit for bit (as test_gpu_features_pair) and the exact reference."""
    labs, planes = fs.scene(name)
    cells, cyto, ref = fs.pair_sets(name)
    B, C = planes.shape[:2]
    td = dev.torch_device
    corr = torch.from_numpy(np.ascontiguousarray(planes)).to(td)
    cl, oc, hc, nc = _tables(dev, cells)
    cy, oy, hy, ny = _tables(dev, cyto)
    F = n_features(C)
    per_set = [torch.zeros((B, MAX_LABEL, F), dtype=torch.float64, device=td) for _ in range(2)]
    dev.features(cl, corr, C, MAX_LABEL, oc, hc, per_set[0])
    dev.features(cy, corr, C, MAX_LABEL, oy, hy, per_set[1])
    pair = [torch.zeros((B, MAX_LABEL, F), dtype=torch.float64, device=td) for _ in range(2)]
    dev.features_pair(cl, cy, corr, C, MAX_LABEL, (oc, hc, pair[0]), (oy, hy, pair[1]))
    dev.sync()
    for p, s in zip(pair, per_set):
        assert torch.equal(p, s)
    same = 0
    ocn, oyn = as_numpy(oc, "object").reshape(B, MAX_LABEL), as_numpy(oy, "object").reshape(B, MAX_LABEL)
    for s, (p, n) in enumerate(zip(pair, (nc, ny))):
        g = p.cpu().numpy()
        for b in range(B):
            rows, diags = ref[s][b]
            fx.compare(g[b, :n[b]], rows, diags, f"{name} {'Cells' if s == 0 else 'Cytoplasm'} FOV {b}")
    for b in range(B):
        bb = {int(o["label"]): tuple(o["bbox"]) for o in ocn[b, :nc[b]]}
        same += sum(bb.get(int(o["label"])) == tuple(o["bbox"]) for o in oyn[b, :ny[b]])
    assert same >= 3, same  # the twin path (Cytoplasm staged from the Cells pass) was taken
