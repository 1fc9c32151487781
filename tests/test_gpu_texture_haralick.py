"""GPU: the opt-in Haralick texture columns (cpx_texture_haralick, csrc/k_haralick.hip) against the
fp64 numpy restatement of their definitions (tests/haralick_ref.py, which takes its count matrices
from cpx_oracle.glcm / texture_input), through every layer: the batch entry, the per-FOV boundary,
FovPipeline and the plate CLI.

The kernel and the restatement share the count matrix N exactly and differ only in the order of
their fp64 sums and in log2's rounding:
  columns 0-6    rtol = atol = 1e-9 (the project's figure for fixed-order fp64 sums)
  InfoMeas1      atol = 1e-9 * max(1, 1 / max(HX, HY)) with the reference's entropies (the quotient
                 magnifies the entropies' errors by 1 / max(HX, HY)); where the reference's max is 0
                 the column is exactly 0.0
  InfoMeas2      the squares f^2 = 1 - exp(-2 x) at atol 1e-9 (|d f^2 / dx| <= 2; near x = 0 the
                 square root turns 1e-15 into ~4e-8), and f >= 0
Largest differences seen on an MI355X over all cases of this file (each comparison prints its
own): columns 0-6 2.1e-15 (absolute / max(1, |ref|)), InfoMeas1 2.9e-15 (absolute / its
tolerance's scale max(1, 1 / max(HX, HY))), InfoMeas2^2 8.8e-15.
"""
import functools
import os

import numpy as np
import pytest
import torch

import haralick_ref as hr
import synth_golden as sg
from cpx.device import as_numpy, n_colocalization, n_features, n_intensity_ext, n_texture_haralick

pytestmark = pytest.mark.gpu

SENTINEL = -7777.25
SEEN = {"cols0_6": 0.0, "infomeas1": 0.0, "infomeas2_sq": 0.0}


def _tables(dev, lab, max_label):
    B = lab.shape[0]
    lst = dev.empty_bytes(64 * B * (max_label + 1))
    obj = dev.empty_bytes(56 * B * max_label)
    hdr = dev.empty_bytes(16 * B)
    dev.objects(lab, max_label, 200, lst, obj, hdr)
    return obj, hdr


def _planes(B, C, H, W):
    return np.stack([np.stack([sg.plane(800 + 10 * b + c, H, W, n_blobs=20, saturate=False).astype(np.float32) /
                               sg.illum(900 + c, H, W) for c in range(C)]) for b in range(B)]).astype(np.float32)


def _gpu(dev, lab, planes, max_label, features=False):
    """(out [B, max_label, 36 C] on the device, pre-filled with SENTINEL, n_objects [B]) and, with
    features=True, the cpx_features rows [B, max_label, F] of the same tables."""
    td = dev.torch_device
    B, C = planes.shape[:2]
    lt = torch.from_numpy(np.ascontiguousarray(lab, dtype=np.int32)).to(td)
    ct = torch.from_numpy(np.ascontiguousarray(planes)).to(td)
    obj, hdr = _tables(dev, lt, max_label)
    out = torch.full((B, max_label, n_texture_haralick(C)), SENTINEL, dtype=torch.float64, device=td)
    dev.texture_haralick(lt, ct, C, max_label, obj, hdr, out)
    feats = None
    if features:
        feats = torch.zeros((B, max_label, n_features(C)), dtype=torch.float64, device=td)
        dev.features(lt, ct, C, max_label, obj, hdr, feats)
    dev.sync()
    n = as_numpy(hdr, "hdr")["n_objects"].astype(int)
    return (out, n, feats) if features else (out, n)


def _compare_rows(got, ref, ent, what=""):
    """got, ref [n, 36 C]; ent [n, C, 4, 3] the reference's (HX, HY, HXY)."""
    assert got.shape == ref.shape and np.isfinite(ref).all()
    assert np.isfinite(got).all()
    n = len(ref)
    g, r = got.reshape(n, -1, hr.N_HAR), ref.reshape(n, -1, hr.N_HAR)
    hmax = np.maximum(ent[..., 0], ent[..., 1]).reshape(n, -1)
    with np.errstate(divide="ignore"):
        scale = np.where(hmax > 0, np.maximum(1.0, 1.0 / hmax), 1.0)
    d06 = np.abs(g[..., :7] - r[..., :7]) / np.maximum(1.0, np.abs(r[..., :7]))
    d1 = np.abs(g[..., hr.INFO_MEAS1] - r[..., hr.INFO_MEAS1]) / scale
    d2 = np.abs(g[..., hr.INFO_MEAS2] ** 2 - r[..., hr.INFO_MEAS2] ** 2)
    SEEN["cols0_6"] = max(SEEN["cols0_6"], d06.max())
    SEEN["infomeas1"] = max(SEEN["infomeas1"], d1.max())
    SEEN["infomeas2_sq"] = max(SEEN["infomeas2_sq"], d2.max())
    print(f"{what}: {n} objects, largest difference: columns 0-6 {d06.max():.3e} (relative to max(1, |ref|)), "
          f"InfoMeas1 {d1.max():.3e} (over its scale), InfoMeas2^2 {d2.max():.3e}; so far {SEEN}")
    np.testing.assert_allclose(g[..., :7], r[..., :7], rtol=1e-9, atol=1e-9)
    assert (d1 <= 1e-9).all(), d1.max()
    assert (g[..., hr.INFO_MEAS1][hmax == 0] == 0.0).all()
    assert (d2 <= 1e-9).all(), d2.max()
    assert (g[..., hr.INFO_MEAS2] >= 0).all()
    # no pair in a direction: nine +0.0, as the reference has them
    empty = (ent == 0).all(axis=-1).reshape(n, -1) & (r == 0).all(axis=-1)
    assert (g[empty] == 0.0).all() and not np.signbit(g[empty]).any()


def _compare(out, n_obj, refs, what=""):
    got = out.cpu().numpy()
    for b, (ref, ent) in enumerate(refs):
        assert n_obj[b] == len(ref) > 0
        _compare_rows(got[b, :len(ref)], ref, ent, f"{what} fov {b}")
        assert (got[b, len(ref):] == SENTINEL).all()  # rows >= n_objects are not touched


def _contrast_identity(out, feats, n_obj, C):
    """The existing Texture_Contrast = DifferenceVariance + Texture_Dissimilarity^2, per object,
    channel and direction: the two blocks count the same matrix."""
    got, f = out.cpu().numpy(), feats.cpu().numpy()
    for b in range(len(n_obj)):
        n = n_obj[b]
        h = got[b, :n].reshape(n, C, 4, hr.N_HAR)
        t = f[b, :n, 15:].reshape(n, C, 29)[:, :, 5:].reshape(n, C, 4, 6)
        con, dis = t[..., 0], t[..., 1]
        np.testing.assert_allclose(con, h[..., hr.DIFFERENCE_VARIANCE] + dis ** 2, rtol=1e-9, atol=1e-9)


@functools.lru_cache(maxsize=None)
def _case_small():
    B, C, H, W = 2, 3, 200, 232
    lab = np.stack([sg.labels(70 + b, H, W, n=30, rmin=3, rmax=30) for b in range(B)])
    planes = _planes(B, C, H, W)
    return lab, planes, [hr.haralick(lab[b], planes[b]) for b in range(B)]


def test_small_random(dev):
    """Width not a multiple of 64, label gaps, overlapping and border-touching objects, two FOVs,
    three channels; FOV 0 holds a 3 x 1 object (no pair in any direction)."""
    lab, planes, refs = _case_small()
    ref0, ent0 = refs[0]
    assert ((ref0 == 0).all(axis=1) & (ent0 == 0).all(axis=(1, 2, 3))).any()
    out, n, feats = _gpu(dev, lab, planes, 64, features=True)
    _compare(out, n, refs, "small")
    _contrast_identity(out, feats, n, 3)


@functools.lru_cache(maxsize=None)
def _crafted():
    """(labels [64, 64], planes [2, 64, 64], {name: label})"""
    H = W = 64
    rng = np.random.default_rng(23)
    planes = np.stack([rng.uniform(100.0, 5000.0, (H, W)), rng.integers(1, 200, (H, W))]).astype(np.float32)
    lab = np.zeros((H, W), np.int32)
    ids = {}

    def put(name, rows, cols):
        ids[name] = len(ids) + 1
        lab[rows, cols] = ids[name]
        return ids[name]

    put("corner", slice(0, 3), slice(0, 5))                  # on the top and left borders
    put("px1", 5, slice(2, 3))                               # no direction has a pair
    put("line17", 5, slice(6, 13))                           # 1 x 7: (0, 3) only
    put("line71", slice(7, 14), slice(1, 2))                 # 7 x 1: (3, 0) only
    put("sq3", slice(7, 10), slice(4, 7))                    # 3 x 3: (2, 2) and (2, -2) only
    put("sq4", slice(7, 11), slice(9, 13))                   # 4 x 4: every direction
    put("zero", slice(5, 10), slice(16, 22))                 # a flat crop: one level
    planes[:, 5:10, 16:22] = 0.0
    put("const", slice(5, 11), slice(24, 30))                # constant, one bbox pixel outside: two levels
    planes[:, 5:11, 24:30] = 777.0
    lab[5, 24] = 0
    put("checker", slice(5, 13), slice(32, 40))
    yy, xx = np.mgrid[0:8, 0:8]
    planes[:, 5:13, 32:40] = 10.0 + 10.0 * ((yy + xx) % 2)
    put("ramp", slice(14, 18), slice(0, 64))                 # all 256 levels, left to right border
    planes[:, 14:18, :] = (np.arange(64)[None, :] * 4 + np.arange(4)[:, None]).astype(np.float32)
    put("outer", slice(20, 40), slice(2, 28))                # encloses "inner": masked pixels inside the bbox
    put("inner", slice(26, 32), slice(10, 18))
    put("negative", slice(20, 26), slice(32, 40))            # negative values, a -0.0, a masked corner
    planes[:, 20:26, 32:40] = -planes[:, 20:26, 32:40]
    planes[0, 22, 35] = -0.0
    lab[20, 32] = 0
    put("signed", slice(20, 26), slice(44, 52))              # both signs
    planes[:, 20:26, 44:52] -= np.float32(100.0)
    put("subnormal", slice(28, 33), slice(32, 39))           # subnormal values and the masked pixel's 0
    planes[:, 28:33, 32:39] = (rng.integers(1, 1 << 20, (2, 5, 7)).astype(np.float64) * 2.0 ** -149).astype(np.float32)
    lab[28, 32] = 0
    put("huge", slice(28, 33), slice(44, 50))                # ~3e38 in a full bbox: 255 (max - min) stays finite
    planes[:, 28:33, 44:50] = (3.0e38 + rng.uniform(0.0, 1.0e36, (2, 5, 6))).astype(np.float32)
    put("right", slice(36, 44), slice(60, 64))               # on the right border
    put("last", slice(60, 64), slice(58, 64))                # on the bottom and right borders
    put("bottom", slice(57, 64), slice(20, 33))              # on the bottom border
    assert np.isfinite(planes).all() and (np.abs(planes[:, 28:33, 32:39]) < 2.0 ** -126).all()
    return lab, planes, ids


def test_crafted_edges(dev):
    lab, planes, ids = _crafted()
    ref, ent = hr.haralick(lab, planes)
    out, n, feats = _gpu(dev, lab[None], planes[None], 32, features=True)
    _compare(out, n, [(ref, ent)], "crafted")
    _contrast_identity(out, feats, n, 2)
    got = out.cpu().numpy()[0, :len(ids)].reshape(len(ids), 2, 4, hr.N_HAR)
    row = {k: got[v - 1] for k, v in ids.items()}
    assert (row["px1"] == 0).all()
    assert (row["line17"][:, 1:] == 0).all() and (row["line17"][:, 0, hr.SUM_AVERAGE] > 0).all()
    assert (row["line71"][:, [0, 1, 3]] == 0).all() and (row["line71"][:, 2, hr.SUM_AVERAGE] > 0).all()
    assert (row["sq3"][:, [0, 2]] == 0).all() and (row["sq3"][:, [1, 3], hr.SUM_AVERAGE] > 0).all()
    assert (row["sq4"][:, :, hr.SUM_AVERAGE] > 0).all()
    assert (row["zero"] == 0).all() and not np.signbit(row["zero"]).any()      # one level: every column +0.0
    # the checkerboard's closed form (tests/test_texture_haralick_ref.py): exact in the kernel too
    im2 = np.sqrt(1.0 - np.exp(-2.0))
    np.testing.assert_array_equal(row["checker"][0, 0, :8], [127.5 ** 2, 255.0, 0.0, 0.0, 1.0, 0.0, 0.0, -1.0])
    np.testing.assert_array_equal(row["checker"][0, 1, :8], [127.5 ** 2, 255.0, 255.0 ** 2, 1.0, 1.0, 0.0, 0.0, -1.0])
    np.testing.assert_allclose(row["checker"][:, :, hr.INFO_MEAS2], im2, rtol=1e-14)
    # the ramp holds every level: its (0, 3) matrix has 4 * 61 distinct cells of one count each
    assert abs(row["ramp"][0, 0, hr.ENTROPY] - np.log2(4 * 61)) < 1e-12
    assert len(np.unique(hr.count_matrices(lab, planes[0])[ids["ramp"] - 1][0].nonzero()[0])) == 244


@functools.lru_cache(maxsize=None)
def _counter_scene(h, w):
    H, W = h + 3, w + 5
    lab = np.zeros((H, W), np.int32)
    lab[2:2 + h, 3:3 + w] = 1
    lab[2, 3] = 0
    lab[0, 0:2] = 2  # a second, tiny object in the same launch
    planes = np.full((1, H, W), 321.5, np.float32)
    return lab, planes


@pytest.mark.parametrize("h, w, peak", [(255, 260, 65534), (256, 259, 65535), (256, 260, 65791)])
def test_counter_width(dev, h, w, peak):
    """A constant h x w rectangle without its top-left pixel puts h (w - 3) - 1 pairs on cell
    (255, 255) of direction 0: T = 65535 is the last item on the packed 16-bit counters, T = 65536
    (one counter at 65535) and 65792 (one at 65791) take the 32-bit passes."""
    lab, planes = _counter_scene(h, w)
    N = hr.count_matrices(lab, planes[0])[0]
    assert N[0].max() == N[0][255, 255] == peak == h * (w - 3) - 1 and N[0].sum() == h * (w - 3)
    out, n = _gpu(dev, lab[None], planes[None], 8)
    _compare(out, n, [hr.haralick(lab, planes)], f"counter {h}x{w}")


def test_large_and_thin_objects(dev):
    """A 400 x 400 blob of 86,815 px, a 2100 x 31 strip and 30 small objects on a 2200 x 720 plane."""
    lab = sg.boundary_objects()
    H, W = lab.shape
    planes = _planes(1, 2, H, W)
    assert (lab == 3).sum() == 86815
    out, n = _gpu(dev, lab[None], planes, 64)
    _compare(out, n, [hr.haralick(lab, planes[0])], "boundary")


def test_argument_checks(dev):
    from cpx._lib import CpxError, check
    from cpx.device import _ptr
    td = dev.torch_device
    lab, planes, _ = _crafted()
    lt = torch.from_numpy(lab[None]).to(td)
    obj, hdr = _tables(dev, lt, 32)
    out = torch.full((1, 32, n_texture_haralick(2)), SENTINEL, dtype=torch.float64, device=td)
    ct = torch.from_numpy(planes[None]).to(td)
    f = dev.lib.cpx_texture_haralick
    good = [dev.h, _ptr(lt), _ptr(ct), 1, 2, 64, 64, 32, _ptr(obj), _ptr(hdr), _ptr(out)]
    for i in (0, 1, 2, 8, 9, 10):                               # a null context or pointer
        a = list(good)
        a[i] = None
        with pytest.raises(CpxError):
            check(f(*a), "cpx_texture_haralick")
    for i, v in ((3, 0), (3, 65536), (4, 0), (4, -1), (5, 0), (6, -3), (7, 0), (5, 1 << 16)):  # sizes; H * W = 2^22 * ... >= 2^31
        a = list(good)
        a[i] = v
        if i == 5 and v == 1 << 16:
            a[6] = 1 << 15
        with pytest.raises(CpxError):
            check(f(*a), "cpx_texture_haralick")
    dev.sync()
    assert (out == SENTINEL).all()
    # nine channels: no channel-count limit
    nine = np.repeat(planes[:1], 9, axis=0)
    o9, n = _gpu(dev, lab[None], nine[None], 32)
    _compare(o9, n, [hr.haralick(lab, nine)], "nine channels")


def test_deterministic_and_fov_boundary(dev):
    """Two calls give the same bits; cpx_fov_texture_haralick (cpx.fov session) equals the batch entry."""
    from cpx import qc
    C, H, W = 3, 200, 232
    lab, planes, refs = _case_small()
    a, n = _gpu(dev, lab, planes, 64)
    b, _ = _gpu(dev, lab, planes, 64)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    raw = [sg.plane(800 + c, H, W, n_blobs=20, saturate=False) for c in range(C)]
    sess = qc.session()
    for c in range(C):
        sess.set_illum(c, sg.illum(900 + c, H, W))
    sess.submit(raw, C=C)
    # the session's corrected planes are the numpy quotient the batch call was given
    np.testing.assert_array_equal(sess.corrected().cpu().numpy(), planes[0])
    got = sess.texture_haralick(lab[0], max_objects=64)
    assert got.shape == (n[0], 36 * C)
    np.testing.assert_array_equal(got.view(np.int64), a.cpu().numpy()[0, :n[0]].view(np.int64))
    _compare_rows(got, *refs[0], "fov session")
    assert len(sess.features(lab[0], max_objects=64)) == len(got)


@functools.lru_cache(maxsize=None)
def _pipeline_inputs():
    from cpx.synth import synth_illum
    H = W = 1040
    C, B, ML = 5, 2, 512
    w = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "image-processing-suite_amd",
                     "cpx", "weights", "cpnet_nuclei_synth.pt")
    return H, W, C, B, ML, w, synth_illum(C, H, W, seed=1)


@pytest.mark.parametrize("coloc", [False, True])
@pytest.mark.parametrize("iext", [False, True])
def test_pipeline_appends_columns(dev, coloc, iext):
    """FovPipeline with texture_haralick, with and without the other two blocks: the leading columns
    are the bytes of the run without it, the appended block is cpx_texture_haralick of the
    pipeline's own label images and corrected planes (for the FOVs the batch run itself measured)."""
    import cpx.pipeline as pl
    from cpx.synth import synth_fovs
    H, W, C, B, ML, w, illum = _pipeline_inputs()
    raw = synth_fovs(B, C, H, W, dev.torch_device, seed=5)
    kw = dict(H=H, W=W, C=C, batch=B, weights=w, max_objects=ML, colocalization=coloc, intensity_ext=iext)
    p_off = pl.FovPipeline(dev, pl.PipelineConfig(**kw), illum)
    off = p_off.fetch(p_off.run(raw))
    p_on = pl.FovPipeline(dev, pl.PipelineConfig(texture_haralick=True, **kw), illum)
    on = p_on.fetch(p_on.run(raw))
    lead = n_features(C) + (n_colocalization(C) if coloc else 0) + (n_intensity_ext(C) if iext else 0)
    T = n_texture_haralick(C)
    assert sum(len(x) for x in on.feats["Nuclei"]) > 0
    same_run = [b for b in range(B) if not on.recovered[b] & ~pl.RECOVER_FILL_SEQ]
    assert same_run  # FOVs measured by the batch run itself (a re-run FOV's labels live elsewhere)
    for s in pl.OBJECT_SETS:
        lt = p_on.labels[s]
        obj, hdr = _tables(dev, lt, ML)
        direct = torch.full((B, ML, T), SENTINEL, dtype=torch.float64, device=dev.torch_device)
        dev.texture_haralick(lt, p_on.corr, C, ML, obj, hdr, direct)
        dev.sync()
        direct = direct.cpu().numpy()
        for b in range(B):
            x, y = off.feats[s][b], on.feats[s][b]
            assert x.shape == (len(x), lead) and y.shape == (len(x), lead + T)
            assert x.tobytes() == np.ascontiguousarray(y[:, :lead]).tobytes(), (s, b)
            np.testing.assert_array_equal(off.objects[s][b], on.objects[s][b])
            h = y[:, lead:]
            assert np.isfinite(h).all()
            if b in same_run:
                assert h.tobytes() == np.ascontiguousarray(direct[b, :len(y)]).tobytes(), (s, b)
            # against the feature block of the same row
            t = y[:, 15:n_features(C)].reshape(len(y), C, 29)[:, :, 5:].reshape(len(y), C, 4, 6)
            q = h.reshape(len(y), C, 4, hr.N_HAR)
            np.testing.assert_allclose(t[..., 0], q[..., hr.DIFFERENCE_VARIANCE] + t[..., 1] ** 2, rtol=1e-9, atol=1e-9)


def _plate_inputs(tmp_path, dev):
    import pandas as pd
    from cpx import tiffio
    from cpx.synth import synth_fovs, synth_illum
    n, C, H, W = 3, 2, 384, 416
    chans = ["DNA", "AGP"]
    raw = synth_fovs(n, C, H, W, dev.torch_device, seed=5).cpu().numpy().view(np.uint16)
    imgdir = tmp_path / "images"
    imgdir.mkdir()
    rows = []
    for f in range(n):
        row = {"Metadata_Plate": "P07", "Metadata_Well": f"B{f + 1:02d}", "Metadata_Site": 1,
               "Metadata_Timepoint": 48, "Metadata_Compound": "cmpd", "Metadata_ConcLevel": 1}
        for c, ch in enumerate(chans):
            name = f"r02c{f + 1:02d}f01p01-ch{c + 1}.tiff"
            tiffio.imwrite(str(imgdir / name), raw[f * C + c])
            row[f"FileName_{ch}"] = name
        rows.append(row)
    ld = tmp_path / "load_data.csv"
    pd.DataFrame(rows).to_csv(ld, index=False)
    ill = tmp_path / "illum"
    ill.mkdir()
    np.save(ill / "DNA_illum.npy", synth_illum(1, H, W, seed=3)[0].astype(np.float32))
    return chans, ["--load-data", str(ld), "--data-path", str(imgdir), "--illum-path", str(ill),
                   "--channels", *chans, "--batch", "2", "--threads", "4"]


def test_plate_flag(tmp_path, dev):
    """cpx.plate --texture-haralick appends the named columns after the other blocks; without it the
    tables are the text they were; the values are those of a run with the flag alone and satisfy
    the identity with the table's own Contrast and Dissimilarity columns."""
    import pandas as pd
    from cpx import plate
    from cpx.csvout import (OBJECT_TABLES, colocalization_names, feature_names, haralick_names,
                            intensity_ext_names)
    chans, argv = _plate_inputs(tmp_path, dev)
    d_off = plate.run(argv + ["--out", str(tmp_path / "off")])
    d_on = plate.run(argv + ["--out", str(tmp_path / "on"), "--texture-haralick"])
    d_all = plate.run(argv + ["--out", str(tmp_path / "all"), "--colocalization", "--intensity-extended",
                              "--texture-haralick"])
    F = len(feature_names(chans))
    with open(os.path.join(d_off, "Image.csv"), "rb") as f, open(os.path.join(d_on, "Image.csv"), "rb") as g:
        assert f.read() == g.read()
    rows = 0
    for s in OBJECT_TABLES:
        on = pd.read_csv(os.path.join(d_on, f"{s}.csv"), float_precision="round_trip")
        al = pd.read_csv(os.path.join(d_all, f"{s}.csv"), float_precision="round_trip")
        assert list(on.columns[3:]) == feature_names(chans) + haralick_names(chans)
        assert list(al.columns[3:]) == feature_names(chans) + colocalization_names(chans) + \
            intensity_ext_names(chans) + haralick_names(chans)
        h = on[haralick_names(chans)].to_numpy(np.float64)
        assert np.isfinite(h).all()
        assert h.tobytes() == al[haralick_names(chans)].to_numpy(np.float64).tobytes()
        for ch in chans:
            for d in range(4):
                con, dis, dv, e, i2 = (on[f"Texture_{n}_{ch}_3_{d:02d}_256"].to_numpy(np.float64) for n in
                                       ("Contrast", "Dissimilarity", "DifferenceVariance", "Entropy", "InfoMeas2"))
                np.testing.assert_allclose(con, dv + dis ** 2, rtol=1e-9, atol=1e-9)
                assert (e >= 0).all() and (e <= 16).all() and (i2 >= 0).all() and (i2 <= 1).all()
        rows += len(on)
        # flag off: the old columns, and in them the same text as the flag-on run's first columns
        with open(os.path.join(d_off, f"{s}.csv")) as f:
            off_lines = f.read().splitlines()
        with open(os.path.join(d_on, f"{s}.csv")) as f:
            on_lines = f.read().splitlines()
        assert off_lines[0].split(",")[3:] == feature_names(chans)
        assert off_lines == [",".join(ln.split(",")[:3 + F]) for ln in on_lines]
    assert rows > 0
