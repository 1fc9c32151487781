"""CPU: the exact feature reference (tests/features_exact.py) is pinned to skimage 0.18.3 through
the goldens and the oracle, the edge-case scenes (tests/feature_scenes.py) are what they claim to
be, and the per-column comparator rejects a crop with one pixel one level off.
"""
import os

import numpy as np
import pytest

import cpx_oracle as orc
import feature_scenes as fs
import features_exact as fx
import test_gpu_glcm as tg
import test_oracle_golden as tog

# Kernel constants restated (a change there must be a decision here too)
K_BAND_CROP = 16 * 1024          # k_texture.hip: constexpr int kBandCrop = 16 * 1024
K_DENSE_CROP = 160 * 1024 - 4 * 32768 - (256 + 320 + 16 + 2048)  # k_texture.hip: kCrop (kTabW, kSmall)
K_MAX_PX = 65535                 # k_texture.hip k_crop_offsets: bh * bw <= 65535 (u16 pair counters)
K_OUT_CAP = 512                  # k_texture.hip: constexpr int kOutCap = 512
K_BAND_D = 31                    # k_texture.hip: constexpr int kBandD = 31
K_SLACK = 16                     # k_texture.hip: constexpr int kSlack = 16


def crop_bytes(bh, bw):
    """k_texture.hip crop_bytes / crop_stride: rows padded to 8 bytes, kSlack, slot multiple of 16."""
    return (bh * ((bw + 7) & ~7) + K_SLACK + 15) // 16 * 16


def shape_fits(bh, bw):
    """cpx_internal.h cpx_shape_fits: (bh + 4) * ((bw + 4 + 31) >> 5) <= kFastShapeWords (4096)."""
    return (bh + 4) * ((bw + 4 + 31) >> 5) <= 4096


def _class_errors(got, ref):
    """Largest relative difference (absolute where the reference is 0) per column class."""
    C = (ref.shape[1] - fx.N_SHAPE) // fx.PER_CH
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(ref != 0, np.abs(got - ref) / np.abs(ref), np.abs(got - ref))
    cls = {"shape": list(range(fx.N_SHAPE)), "sum": [], "mean": [], "std": [], "minmax": [], "texture": []}
    for ch in range(C):
        o = fx.N_SHAPE + ch * fx.PER_CH
        cls["sum"].append(o)
        cls["mean"].append(o + 1)
        cls["std"].append(o + 2)
        cls["minmax"] += [o + 3, o + 4]
        cls["texture"] += list(range(o + fx.N_INT, o + fx.PER_CH))
    return {k: float(e[:, v].max()) for k, v in cls.items()}


# 10 x the largest difference measured (test_exact_reference_is_pinned); 4 ulp where that was 0
PIN_TOL = {"shape": 1.4e-12, "sum": 1e-15, "mean": 1.5e-6, "std": 2.1e-15, "minmax": 0.0, "texture": 4.6e-14}


def _pin_cases(golden_dir):
    d = np.load(os.path.join(golden_dir, "objects_features.npz"))
    yield "golden", d["feat_labels"], d["feat_planes"], d["feat_expected"]
    lab, planes, exp = tog._boundary_case(golden_dir)
    yield "boundary", lab, planes, exp
    for kind in ("smooth", "step", "noise"):
        lab, planes = tg._scene(kind)
        yield kind, lab, planes, orc.features(lab, planes)


def test_exact_reference_is_pinned(golden_dir):
    """features_exact against the skimage 0.18.3 goldens (objects_features, features_boundary) and
    against cpx_oracle.features on the test_gpu_glcm scenes.  Largest differences measured, over
    all five cases, per column class (relative; absolute where the reference is 0):

        shape    1.33e-13 (float moments / eigvalsh of the reference against exact integers)
        sum      0        (numpy's pairwise fp64 sum against fsum; asserted at 1e-15, 4 ulp, so
                          that another numpy's summation order does not fail it)
        mean     1.43e-7  (skimage's mean_intensity is np.mean of a float32 array: an fp32
                          pairwise sum, so the goldens themselves carry ~1e-7; the exact mean is
                          fsum / n.  The one class above 1e-9, for this reason.)
        std      2.03e-16 (np.std in fp64, two-pass like the exact one)
        min/max  0
        texture  4.51e-15 (fp64 sums over the normalised 256 x 256 matrix against integers)

    Asserted at 10 x those figures (PIN_TOL)."""
    worst = {}
    for name, lab, planes, exp in _pin_cases(golden_dir):
        got, diags = fx.features(lab, planes)
        assert got.shape == exp.shape and len(diags) == len(exp), name
        e = _class_errors(got, exp)
        print(name, e)
        for k, v in e.items():
            worst[k] = max(worst.get(k, 0.0), v)
            assert v <= PIN_TOL[k], (name, k, v)
    print("worst", worst)


def _all_objects():
    for name in fs.SCENES:
        for b, (rows, diags) in enumerate(fs.exact(name)):
            for d in diags:
                yield name, b, d


def test_scene_images_are_odd_sized_and_small():
    for name in fs.SCENES:
        labs, planes = fs.scene(name)
        B, H, W = labs.shape
        assert planes.shape == (B, 2, H, W) and B <= 2, name
        assert W % 2 == 1 and W % 4 != 0, (name, W)
        assert H <= 300 and W <= 300 or name == "mask_words", (name, H, W)  # cpx_shape_fits needs 406 rows
        assert np.isfinite(planes).all(), name


def test_every_object_is_symmetric_or_well_conditioned():
    """No object is skipped by the comparator: each is exactly symmetric (a - c == 0: skimage's
    +-pi/4 rule decides) or its orientation is well-conditioned."""
    kinds = {"symmetric": 0, "conditioned": 0}
    for name, b, d in _all_objects():
        k = fx.orientation_class(d)
        assert k in kinds, (name, b, d["label"], float(d["a_minus_c"]), float(d["b"]))
        kinds[k] += 1
    assert kinds["symmetric"] >= 4 and kinds["conditioned"] >= 40, kinds
    for name in fs.PAIR_SCENES:  # and the Cells / Cytoplasm sets derived from them
        for per_fov in fs.pair_sets(name)[2]:
            for rows, diags in per_fov:
                assert all(fx.orientation_class(d) in kinds for d in diags), name
    # one object is symmetric about its diagonal only: a - c == 0 with b != 0, where skimage's rule
    # (-pi/4 if b < 0 else pi/4) is the opposite of the limit of 0.5 atan2(-2b, c - a); the kernels
    # follow the rule
    d = fs.exact("dense_crop")[0][1][0]
    assert d["a_minus_c"] == 0 and d["b"] > 0 and fs.exact("dense_crop")[0][0][0, fx.ORIENT] == np.pi / 4


def test_scene_tiny_preconditions():
    (rows, diags), = fs.exact("tiny")
    by = {d["label"]: d for d in diags}
    T = lambda L: [a["T"] for a in by[L]["channels"][0]["angles"]]
    for L in (1, 2, 3, 4, 8):       # bbox at most 2 x 2: no pair at any angle
        assert T(L) == [0, 0, 0, 0], L
    assert T(5) == [4, 0, 0, 0]     # 1 x 7: (0,3) only
    assert T(6) == [0, 0, 4, 0]     # 7 x 1: (3,0) only
    assert T(7) == [10, 9, 10, 9]   # the diagonal's 5 x 5 bbox
    assert T(9) == [0, 1, 0, 1] and T(10) == [0, 1, 0, 1]   # 3 x 3: the diagonals' single pair
    assert T(11) == [8, 0, 0, 0] and T(12) == [0, 0, 8, 0]
    assert [by[L]["n"] for L in range(1, 11)] == [1, 2, 2, 4, 7, 7, 5, 3, 5, 9]
    # zero-pair angles read [0, 0, 0, 0, 0, 1] as greycoprops gives
    o = fx.N_SHAPE + fx.N_INT
    assert rows[0, o:o + 6].tolist() == [0, 0, 0, 0, 0, 1]
    labs, _ = fs.scene("tiny")
    assert labs[0, -1, -1] == 13    # an object on the plane's very last pixel


def test_scene_borders_preconditions():
    labs, planes = fs.scene("borders")
    assert labs.shape == (2, 61, 67)
    for b in range(2):
        L = labs[b]
        assert L[0, 0] and L[0, -1] and L[-1, 0] and L[-1, -1]          # the four corners
        mid = slice(15, 45)
        assert L[0, mid].any() and L[-1, mid].any() and L[mid, 0].any() and L[mid, -1].any()  # the four edges
    assert labs[0, -1, -1] == labs[1, 0, 0] != 0  # the same id on either side of the FOV boundary
    assert not np.array_equal(planes[0, :, -1, -8:], planes[1, :, 0, :8])
    assert planes[0, 0, -1].max() * 100 < planes[0, 1, 0].min()  # channel 0's last row, channel 1's first


def test_scene_topology_preconditions():
    (rows, diags), = fs.exact("topology")
    by = {d["label"]: d for d in diags}
    for L in (1, 2, 3, 4):  # disc, square, diamond, annulus
        assert by[L]["a_minus_c"] == 0 and by[L]["b"] == 0 and by[L]["l1_eq_l2"], L
        assert rows[L - 1, fx.ECC] == 0.0 and rows[L - 1, fx.ORIENT] == np.pi / 4
    labs, _ = fs.scene("topology")
    cy, cx = rows[3, 2], rows[3, 3]
    assert labs[0, int(round(cy)), int(round(cx))] == 0  # the annulus' centroid lies outside it
    from scipy import ndimage as ndi
    assert ndi.label(labs[0] == 6, np.ones((3, 3)))[1] == 2   # one label, two components
    assert ndi.label(labs[0] == 7)[1] == by[7]["n"]           # checkerboard: 4-connected singletons
    assert by[7]["perim_counts"] != (0, 0, 0)
    filled = ndi.binary_fill_holes(labs[0] == 5)
    assert ndi.label(filled & (labs[0] != 5))[1] == 3         # three holes
    b8, b9 = by[8]["bbox"], by[9]["bbox"]
    assert b9[0] <= b8[0] and b9[1] <= b8[1] and b9[2] >= b8[2] and b9[3] >= b8[3]  # interleaved


def test_scene_widths_preconditions():
    (rows, diags), = fs.exact("widths")
    ws = [d["bbox"][3] - d["bbox"][1] for d in diags]
    hs = [d["bbox"][2] - d["bbox"][0] for d in diags]
    assert ws == list(range(3, 20)) and {w % 8 for w in ws} == set(range(8))
    assert set(hs) == {3, 4, 5, 6}
    assert all(d["n"] == w * h for d, w, h in zip(diags, ws, hs))


def test_scene_counters_preconditions():
    (r0, d0), (r1, d1) = fs.exact("counters")
    big0, big1 = d0[0], d1[0]
    bh, bw = big0["bbox"][2] - big0["bbox"][0], big0["bbox"][3] - big0["bbox"][1]
    assert (bh, bw) == (255, 257) and bh * bw == K_MAX_PX and big0["n"] == K_MAX_PX
    ang = big0["channels"][0]["angles"]
    assert all(60000 <= a["max_key"] <= 65535 for a in ang), [a["max_key"] for a in ang]
    assert all(a["outliers"] == 0 for a in ang)
    assert big0["channels"][0]["levels"] == [0, 255]
    ang = big1["channels"][0]["angles"]
    assert all(a["outliers"] > K_OUT_CAP for a in ang), [a["outliers"] for a in ang]  # dense redo
    assert len(big1["channels"][0]["levels"]) == 256


def test_scene_steps_preconditions():
    (rows, diags), = fs.exact("steps")
    by = {d["label"]: d["channels"][0] for d in diags}
    assert by[1]["levels"] == [224, 255] and by[2]["levels"] == [223, 255]   # |i - j| = 31 and 32
    assert 255 - 224 == K_BAND_D and 255 - 223 == K_BAND_D + 1
    assert [a["outliers"] for a in by[1]["angles"]] == [0, 0, 0, 0]          # 31: inside the band
    assert max(a["outliers"] for a in by[2]["angles"]) > 0                   # 32: the outlier list
    assert max(a["outliers"] for a in by[2]["angles"]) < K_OUT_CAP
    assert [a["outliers"] for a in by[3]["angles"]] == [512, 512, 512, 512]  # the list exactly full
    assert [a["outliers"] for a in by[4]["angles"]] == [513, 513, 513, 512]  # one too many: redo
    assert K_OUT_CAP == 512


def _limit_boxes(name):
    out = []
    for rows, diags in fs.exact(name):
        assert len(diags) == 1
        r0, c0, r1, c1 = diags[0]["bbox"]
        out.append((r1 - r0, c1 - c0, diags[0]))
    return out


def test_scene_staging_limit_preconditions():
    (h0, w0, _), (h1, w1, _) = _limit_boxes("band_crop")
    assert crop_bytes(h0, w0) == K_BAND_CROP and crop_bytes(h1, w1) > K_BAND_CROP
    (h0, w0, d0), (h1, w1, d1) = _limit_boxes("dense_crop")
    assert crop_bytes(h0, w0) <= K_DENSE_CROP < crop_bytes(h1, w1)
    assert K_DENSE_CROP - crop_bytes(h0, w0) < 176 and K_DENSE_CROP == 30128
    for d in (d0, d1):  # both reach the dense kernel: channel 0 overflows the outlier list
        assert max(a["outliers"] for a in d["channels"][0]["angles"]) > K_OUT_CAP
    (h0, w0, _), (h1, w1, _) = _limit_boxes("px65535")
    assert h0 * w0 == K_MAX_PX and h1 * w1 > K_MAX_PX and shape_fits(h0, w0) and shape_fits(h1, w1)
    (h0, w0, _), (h1, w1, _) = _limit_boxes("mask_words")
    assert shape_fits(h0, w0) and not shape_fits(h1, w1)
    assert (h0 + 4) * ((w0 + 35) >> 5) == 4090 and (h1 + 4) * ((w1 + 35) >> 5) == 4100


def test_scene_intensity_preconditions():
    (r0, d0), (r1, d1) = fs.exact("intensity")
    labs, planes = fs.scene("intensity")
    const = np.float32(65535 / 0.9137)
    assert float(const) != round(float(const))
    o = fx.N_SHAPE
    for rows, diags, b, px in ((r0, d0, 0, 200 * 200), (r1, d1, 1, 260 * 262)):
        assert diags[0]["n"] == px and (px > K_MAX_PX) == (b == 1)
        assert (planes[b, 0][labs[b] == 1] == const).all()
        assert rows[0, o + 2] == 0.0 and rows[0, o + 1] == float(const)  # Std exactly 0
        # A flat object that fills its bbox quantises to all zeros: every pair is (0, 0), and
        # greycoprops of that matrix is [0, 0, 1, 1, 1, 1] (homogeneity, ASM and energy of the single
        # cell P[0, 0] = 1; skimage 0.18.3 and cpx_oracle.greycoprops agree).  [0, 0, 0, 0, 0, 1] is what
        # a zero-pair angle gives (test_scene_tiny_preconditions), not a flat object.
        for a in range(4):
            t = rows[0, o + fx.N_INT + 6 * a:o + fx.N_INT + 6 * a + 6].tolist()
            assert t == [0, 0, 1, 1, 1, 1], t
            assert t == orc.greycoprops(orc.glcm(np.zeros((9, 9), np.uint8), 3, orc.GLCM_ANGLES[a]))
        near = rows[1]
        assert 0 < near[o + 2] < 0.03 and abs(near[o + 1] - 70000.0) < 0.01  # a few fp32 ulps of 70000
        assert (planes[b, 1][labs[b] > 0] < 0).any() and (planes[b, 1][labs[b] == 0] < 0).any()
    v = planes[0, 0][labs[0] == 3]
    assert v.max() / v.min() > 5e5  # six decades


def _rel(got, ref):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.nanmax(np.where(ref != 0, np.abs(got - ref) / np.abs(ref), np.abs(got - ref))))


def test_comparator_rejects_one_level_off():
    """One in-object pixel of the 'smooth' scene is quantised one level off (q8 +-1) on the side
    that plays the kernel; the exact rows of that crop must be rejected against the unmodified
    reference.  Measured: the three cases differ from the reference by 2.1e-4, 7.0e-5 and 4.2e-4
    relative at most (Correlation and Contrast: a smooth object's contrast sum is small), so
    np.allclose(rtol=1e-5, atol=1e-9) — `_feat_close`, what the other feature tests use — rejects these
    rows too: a level-off pixel is not in its blind spot here.  (Neither is one pair moved to the
    background count: 1.4e-3.)  What rtol 1e-5 cannot tell is an exact integer column from a
    nearly exact one; this comparator asserts the former at 1e-9."""
    lab, planes = tg._scene("smooth")
    ref, diags = fx.features(lab, planes)
    assert fx.compare(ref.copy(), ref, diags)["texture"] == 0.0
    for label, ch, s in ((1, 0, 1), (3, 1, -1), (4, 0, -1)):
        def hook(q8, L, c):
            if L == label and c == ch:
                q8 = q8.copy()
                r, x = q8.shape[0] // 2, q8.shape[1] // 2
                assert 0 < q8[r, x] < 255 and lab[lab == L].size  # in the object
                q8[r, x] = int(q8[r, x]) + s
            return q8
        wrong, _ = fx.features(lab, planes, q8_hook=hook)
        assert not np.array_equal(wrong, ref)
        print("one level off: largest relative difference", _rel(wrong, ref))
        with pytest.raises(AssertionError, match=r"\[texture\]"):
            fx.compare(wrong, ref, diags)
