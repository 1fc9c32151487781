"""bench.py --dump-outputs: the .npy files written from one step's FovResults (CPU only)."""
import os

import numpy as np

import bench
from cpx.device import _np_dtypes
from cpx.pipeline import OBJECT_SETS, FovResults


def _results(B=3, C=2, F=7, seed=5):
    rng = np.random.default_rng(seed)
    dt = _np_dtypes()
    qc = np.zeros(B * C, dt["qc"])
    qc["slope"], qc["pct_max"] = rng.normal(size=B * C), rng.random(B * C)
    hdr, objs, feats = {}, {}, {}
    for s in OBJECT_SETS:
        n = rng.integers(0, 40, B)
        n[1] = 0  # an empty FOV
        hdr[s] = np.zeros(B, dt["hdr"])
        hdr[s]["n_objects"] = n
        objs[s], feats[s] = [], []
        for b in range(B):
            o = np.zeros(n[b], dt["object"])
            o["label"] = np.arange(1, n[b] + 1)
            o["area"] = rng.integers(1, 500, n[b])
            o["bbox"] = rng.integers(0, 300, (n[b], 4))
            o["centroid_r"], o["centroid_c"] = rng.random(n[b]), rng.random(n[b])
            objs[s].append(o)
            feats[s].append(rng.normal(size=(n[b], F)))
    return FovResults(qc=qc, hdr=hdr, objects=objs, feats=feats, seg_stats=np.zeros(B),
                      failed=np.zeros(B, bool), recovered=np.zeros(B, np.int32))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_whole_tables(tmp_path):
    res = _results()
    bench.dump_outputs(str(tmp_path / "d"), res)
    got = _load(tmp_path / "d")
    assert set(got) == ({"qc", "failed", "recovered"} |
                        {f"{k}_{s}" for s in OBJECT_SETS for k in ("n_objects", "objects", "features")})
    assert all(v.dtype == np.float64 for v in got.values())
    assert np.array_equal(got["qc"], np.stack([res.qc["slope"], res.qc["pct_max"]], axis=1))
    for s in OBJECT_SETS:
        o = np.concatenate(res.objects[s])
        assert np.array_equal(got[f"n_objects_{s}"], res.hdr[s]["n_objects"])
        assert got[f"objects_{s}"].shape == (len(o), 12)
        assert np.array_equal(got[f"objects_{s}"][:, 0], o["label"])
        assert np.array_equal(got[f"objects_{s}"][:, 2:6], o["bbox"])
        assert np.array_equal(got[f"objects_{s}"][:, 6], o["centroid_r"])
        assert np.array_equal(got[f"features_{s}"], np.concatenate(res.feats[s]))


def test_dump_outputs_sample_is_bounded_and_fixed(tmp_path):
    """Tables beyond the limit: a row sample within it, the same rows of the object and feature
    tables, in order, and the same in every run."""
    res = _results()
    limit = (1 << 20) + 4000
    bench.dump_outputs(str(tmp_path / "a"), res, limit=limit)
    bench.dump_outputs(str(tmp_path / "b"), res, limit=limit)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(v.nbytes for v in a.values()) <= limit
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= limit
    for k in a:
        assert np.array_equal(a[k], b[k])
    for s in OBJECT_SETS:
        full_f = np.concatenate(res.feats[s])
        full_o = np.concatenate(res.objects[s])
        f, o = a[f"features_{s}"], a[f"objects_{s}"]
        assert 0 < len(f) < len(full_f) and len(o) == len(f)
        rows = [int(np.nonzero((full_f == r).all(axis=1))[0][0]) for r in f]
        assert rows == sorted(set(rows))
        assert np.array_equal(o[:, 1], full_o["area"][rows])
