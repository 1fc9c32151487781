"""GPU parity: libcpx HIP kernels (through the C ABI) vs the oracle and the reference goldens.

Tolerances: integer / index / byte outputs bit-exact; PercentMaximal exact (fp64 tie count);
fp32 corrected planes bit-exact to numpy's uint16/float32 division; QC slope and powersum
rel 1e-9 (fp64 FFT); features rel 1e-5 (north_star) with an absolute floor of 1e-9 for
values that are mathematically ~0.
"""
import json
import os

import numpy as np
import pytest
import torch

import cpx_oracle as orc
import synth_golden as sg
from cpx.device import as_numpy, n_features

pytestmark = pytest.mark.gpu


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


def _meta(golden_dir, name):
    with open(os.path.join(golden_dir, name + ".json")) as f:
        return json.load(f)


def _u16(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(dev.torch_device)


def _t(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev.torch_device)


def _run_qc(dev, raw, ill, C=1):
    """raw [n,H,W] u16, ill [C,H,W] or None -> (stats, qc, powersum, corr)."""
    n, H, W = raw.shape
    r = _u16(dev, raw)
    il = None if ill is None else _t(dev, ill)
    corr = torch.empty((n, H, W), dtype=torch.float32, device=dev.torch_device)
    stats = dev.empty_bytes(64 * n)
    qc = dev.empty_bytes(24 * n)
    nr = max(min(H, W) // 8 - 2, 1)
    ps = torch.empty((n, nr), dtype=torch.float64, device=dev.torch_device)
    dev.illum_correct(r, il, C, corr, stats)
    dev.qc_rps(r, il, C, stats, qc, ps)
    dev.sync()
    return as_numpy(stats, "stats"), as_numpy(qc, "qc"), ps.cpu().numpy(), corr.cpu().numpy()


def test_illum_qc_small_cases(dev, golden_dir):
    d = _load(golden_dir, "qc_cases")
    meta = _meta(golden_dir, "qc_cases")
    for name, m in meta.items():
        if name == "full":
            continue
        raw = d[f"{name}_raw"][None]
        ill = d[f"{name}_illum"][None] if f"{name}_illum" in d.files else None
        st, qc, ps, corr = _run_qc(dev, raw, ill)
        assert st[0]["pct_max"] == m["pct_max"], name
        assert qc[0]["pct_max"] == m["pct_max"], name
        if np.isnan(m["slope"]):
            assert np.isnan(qc[0]["slope"]), name
        else:
            assert qc[0]["slope"] == pytest.approx(m["slope"], rel=1e-9, abs=1e-12), name
        gp = d[f"{name}_powersum"]
        if gp.size > 1 and np.all(np.isfinite(gp)) and gp[0] > 0:
            # libcpx skips the median(|img-mean|) normalisation (slope-invariant): the ring sums
            # equal the reference's up to one constant factor per plane
            np.testing.assert_allclose(ps[0, :gp.size] / ps[0, 0], gp / gp[0], rtol=1e-9, err_msg=name)
        if ill is not None and ill.dtype == np.float32:
            with np.errstate(all="ignore"):
                np.testing.assert_array_equal(corr[0], orc.illum_correct_producer(raw[0], ill[0]))


def test_illum_qc_full_fov_batched(dev, golden_dir):
    meta = _meta(golden_dir, "qc_cases")["full"]
    d = _load(golden_dir, "qc_cases")
    raw, ill = sg.full_case(meta["seed"], meta["H"], meta["W"], meta["C"], meta["n_blobs"])
    raw2 = np.concatenate([raw, raw])  # two FOVs -> plane p uses illum[p % C]
    st, qc, ps, corr = _run_qc(dev, raw2, ill, C=meta["C"])
    for p in range(2 * meta["C"]):
        exp = meta["channels"][p % meta["C"]]
        assert qc[p]["pct_max"] == exp["pct_max"]
        assert qc[p]["slope"] == pytest.approx(exp["slope"], rel=1e-9)
        gp = d[f"full_c{p % meta['C']}_powersum"]
        np.testing.assert_allclose(ps[p] / ps[p][0], gp / gp[0], rtol=1e-9)
    np.testing.assert_array_equal(corr[1], orc.illum_correct_producer(raw[1], ill[1]))


def test_qc_rows_2080_matches_generic_fft(dev, monkeypatch):
    """The W = 2080 row pass (k_qc_rows_2080: three register passes, pruned last pass) against the
    generic Stockham row pass on the same planes — ordinary FOVs, an odd row count (H = 2197: the
    last row pair has one row and the last block 3 of its 4 row pairs; the fast kernel needs
    W == 2080 and min(H, W) // 8 == 260, so a shorter odd H such as 2079 would run the generic
    kernel twice), a constant plane, a NaN pixel, a plane that is mostly its mean.  Against
    numpy: tests/test_gpu_qc_shapes.py."""
    rng = np.random.default_rng(31)
    H, W, H_odd = 2080, 2080, 2197
    assert min(H_odd, W) // 8 == 260 and H_odd % 2 == 1 and ((H_odd + 1) // 2) % 4 == 3
    raw_odd = rng.integers(100, 4000, (5, H_odd, W), dtype=np.uint16)
    raw_odd[1] = 1234
    raw_odd[3, :1500] = 777
    ill_odd = (0.7 + 0.6 * rng.random((1, H_odd, W))).astype(np.float32)
    raw, ill = np.ascontiguousarray(raw_odd[:, :H]), np.ascontiguousarray(ill_odd[:, :H])
    ill_nan = ill.copy()
    for case_raw, case_ill, h in ((raw, ill, H), (raw_odd, ill_odd, H_odd), (raw[4:5], ill_nan, H)):
        if case_ill is ill_nan:
            case_ill = case_ill.copy()
            case_ill[0, 17, 33] = np.nan
        monkeypatch.setenv("CPX_QC_GENERIC", "1")
        _, qg, pg, _ = _run_qc(dev, case_raw, case_ill)
        monkeypatch.delenv("CPX_QC_GENERIC")
        _, qs, ps, _ = _run_qc(dev, case_raw, case_ill)
        for p in range(case_raw.shape[0]):
            a, b = qs[p]["slope"], qg[p]["slope"]
            assert (np.isnan(a) and np.isnan(b)) or a == pytest.approx(b, rel=1e-12, abs=1e-14), (h, p, a, b)
            fin = np.isfinite(pg[p]) & (pg[p] > 0)
            np.testing.assert_allclose(ps[p][fin], pg[p][fin], rtol=1e-10, err_msg=f"{h} {p}")


def test_zmax_vs_maximum_reduce(dev, golden_dir):
    d = _load(golden_dir, "maxproj")
    planes = np.stack([d[f"plane{z}"] for z in range(5)])
    out = torch.empty(planes.shape[1:], dtype=torch.int16, device=dev.torch_device)
    dev.zmax(_u16(dev, planes[None]), out[None])
    dev.sync()
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint16), d["expected"])
    # odd size (scalar path) and several groups
    g = np.stack([np.stack([sg.plane(40 + 7 * gi + z, 37, 51, n_blobs=3) for z in range(7)]) for gi in range(3)])
    out = torch.empty((3, 37, 51), dtype=torch.int16, device=dev.torch_device)
    dev.zmax(_u16(dev, g), out)
    dev.sync()
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint16), np.maximum.reduce(g, axis=1))


def _objects(dev, labels, max_label=512, box=200):
    B = labels.shape[0]
    lab = _t(dev, labels.astype(np.int32))
    lst = dev.empty_bytes(64 * B * (max_label + 1))
    obj = dev.empty_bytes(56 * B * max_label)
    hdr = dev.empty_bytes(16 * B)
    dev.objects(lab, max_label, box, lst, obj, hdr)
    dev.sync()
    return lab, obj, hdr, as_numpy(obj, "object").reshape(B, max_label), as_numpy(hdr, "hdr")


def test_objects_match_regionprops(dev, golden_dir):
    d = _load(golden_dir, "objects_features")
    lab = d["objects_labels"]
    exp = d["objects_table"]
    _, _, _, objs, hdr = _objects(dev, lab[None])
    n = hdr[0]["n_objects"]
    assert n == len(exp)
    tab = orc.object_table(lab, 200)
    for k in range(n):
        o, e, t = objs[0, k], exp[k], tab[k]
        assert o["label"] == int(e[0]) and o["area"] == int(e[1])
        assert tuple(o["bbox"]) == tuple(int(x) for x in e[2:6])
        assert o["centroid_r"] == e[6] and o["centroid_c"] == e[7]
        assert (o["yc"], o["xc"]) == (int(e[8]), int(e[9]))
        assert bool(o["kept"]) == t["kept"] and o["cell_idx"] == t["cell_idx"]
    assert hdr[0]["n_kept"] == sum(t["kept"] for t in tab)
    assert hdr[0]["max_label"] == lab.max() and hdr[0]["overflow"] == 0


def test_objects_edge_cases(dev):
    # empty label image, one pixel objects, labels above capacity
    lab = np.zeros((3, 64, 80), np.int32)
    lab[1, 0, 0] = 5
    lab[1, 63, 79] = 2
    lab[2, 10:20, 10:20] = 9
    lab[2, 30, 30] = 70  # > max_label=32 -> overflow flag, ignored
    _, _, _, objs, hdr = _objects(dev, lab, max_label=32, box=8)
    assert hdr[0]["n_objects"] == 0
    assert hdr[1]["n_objects"] == 2 and list(objs[1, :2]["label"]) == [2, 5]
    assert hdr[2]["n_objects"] == 1 and hdr[2]["overflow"] == 1 and hdr[2]["max_label"] == 70
    assert objs[2, 0]["area"] == 100 and objs[2, 0]["kept"] == 1


def test_crops_and_scale8_bit_exact(dev, golden_dir):
    H, W, C, box = 520, 560, 3, 200
    lab = sg.labels(31, H, W, n=25, rmin=10, rmax=70)
    planes = np.stack([sg.plane(700 + c, H, W, n_blobs=20).astype(np.float32) /
                       sg.illum(800 + c, H, W) for c in range(C)]).astype(np.float32)
    labt, obj, hdr, objs, h = _objects(dev, lab[None], max_label=64, box=box)
    nk = int(h[0]["n_kept"])
    assert nk > 0
    corr = _t(dev, planes[None])
    crops = torch.zeros((1, nk, box, box, C), dtype=torch.float32, device=dev.torch_device)
    crops8 = torch.zeros((1, nk, C, box, box), dtype=torch.uint8, device=dev.torch_device)
    dev.crops(labt, corr, C, 64, obj, hdr, box, nk, crops, crops8)
    crops8_only = torch.zeros_like(crops8)  # the embedder's call: no float crops kept
    dev.crops(labt, corr, C, 64, obj, hdr, box, nk, None, crops8_only)
    dev.sync()
    assert torch.equal(crops8_only, crops8)
    tab = orc.object_table(lab, box)
    ref = orc.crops(np.moveaxis(planes, 0, -1), lab, tab, box)
    assert len(ref) == nk
    got = crops.cpu().numpy()[0]
    got8 = crops8.cpu().numpy()[0]
    for k in range(nk):
        np.testing.assert_array_equal(got[k], ref[k])
        for c in range(C):
            np.testing.assert_array_equal(got8[k, c], orc.scale_to_8bit(ref[k][:, :, c]))


def _features(dev, labels, planes, max_label=256):
    C = planes.shape[0]
    labt, obj, hdr, objs, h = _objects(dev, labels[None], max_label=max_label)
    F = n_features(C)
    feats = torch.zeros((1, max_label, F), dtype=torch.float64, device=dev.torch_device)
    dev.features(labt, _t(dev, planes[None]), C, max_label, obj, hdr, feats)
    dev.sync()
    return feats.cpu().numpy()[0, : int(h[0]["n_objects"])]


def _feat_close(got, exp):
    # orientation is ill-conditioned when mu20 ~ mu02 and mu11 ~ 0 (skimage's float moments pick
    # an arbitrary branch); every golden object here is sheared, so compare everything.
    np.testing.assert_allclose(got, exp, rtol=1e-5, atol=1e-9)


def test_features_match_skimage_golden(dev, golden_dir):
    d = _load(golden_dir, "objects_features")
    got = _features(dev, d["feat_labels"], d["feat_planes"])
    _feat_close(got, d["feat_expected"])


def test_features_boundary_objects_golden(dev, golden_dir):
    """skimage 0.18.3 golden for objects straddling the LDS fast-path limits: texture bbox just
    under / over 65535 px, a strip beyond the 4096-word membership mask (both fallbacks although
    its bbox fits the texture limit), a 401 x 317 blob (tools/make_golden_bigobj.py)."""
    import test_oracle_golden as tog
    lab, planes, exp = tog._boundary_case(golden_dir)
    got = _features(dev, lab, planes)
    _feat_close(got, exp)


def test_features_wide_image(dev):
    """W > 4096: crops are not staged (k_obj_stage's 24-bit offsets), texture comes from the
    fallback kernel, AreaShape still from the LDS path; results as the oracle."""
    H, W, C = 96, 4160, 2
    lab = sg.labels(61, H, W, n=12, rmin=5, rmax=40, skip_every=0)
    planes = np.stack([sg.plane(960 + c, H, W, n_blobs=12).astype(np.float32) /
                       sg.illum(970 + c, H, W) for c in range(C)]).astype(np.float32)
    got = _features(dev, lab, planes)
    _feat_close(got, orc.features(lab, planes))


def test_features_match_oracle_larger(dev):
    H, W, C = 700, 760, 2
    lab = sg.labels(41, H, W, n=40, rmin=5, rmax=150, skip_every=0)
    planes = np.stack([sg.plane(900 + c, H, W, n_blobs=30).astype(np.float32) /
                       sg.illum(950 + c, H, W) for c in range(C)]).astype(np.float32)
    got = _features(dev, lab, planes)
    _feat_close(got, orc.features(lab, planes))


def test_expand_labels_bit_exact(dev, golden_dir):
    d = _load(golden_dir, "objects_features")
    lab = d["expand_labels_in"]
    labs = np.stack([lab, sg.labels(51, lab.shape[0], lab.shape[1], n=60, rmin=2, rmax=9),
                     np.zeros_like(lab)])
    B, H, W = labs.shape
    t = _t(dev, labs.astype(np.int32))
    for dist in (1, 5, 15):
        cells = torch.empty_like(t)
        cyto = torch.empty_like(t)
        from cpx._lib import check
        from cpx.device import _ptr
        check(dev.lib.cpx_expand_labels(dev.h, _ptr(t), B, H, W, dist, _ptr(cells), _ptr(cyto)), "expand")
        dev.sync()
        gc, gy = cells.cpu().numpy(), cyto.cpu().numpy()
        np.testing.assert_array_equal(gc[0], d[f"expand_labels_d{dist}"])
        for b in range(B):
            rc, ry = orc.secondary_objects(labs[b], dist)
            np.testing.assert_array_equal(gc[b], rc)
            np.testing.assert_array_equal(gy[b], ry)


def test_features_bit_reproducible(dev):
    """Two runs of cpx_features give identical bits (no order-dependent float sums)."""
    H, W, C = 400, 420, 2
    lab = sg.labels(77, H, W, n=30, rmin=5, rmax=60, skip_every=0)
    planes = np.stack([sg.plane(780 + c, H, W, n_blobs=20).astype(np.float32) for c in range(C)])
    a = _features(dev, lab, planes)
    b = _features(dev, lab, planes)
    np.testing.assert_array_equal(a, b)

