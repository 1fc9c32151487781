"""CPU: the mask-dynamics edge scenes (tests/seg_scenes.py) are what they claim to be, so a GPU
mismatch on them (tests/test_gpu_seg_edges.py) is a kernel bug and not a scene artefact.  Every test
asserts its scene's condition on the oracle's intermediates (seg_scenes.stages, whose restated
get_masks is compared with seg_oracle.get_masks on every FOV it is given) and that the scene
discriminates: the deliberately wrong variant of each rule it pins changes the label image.

One rule cannot be pinned through labels: `fewer than 5 moving pixels -> no masks`.  With 4, 5 (or
up to 9) moving pixels no histogram cell can exceed 10 whatever the flow does, so there is no seed
and the label image is empty under `< 4`, `< 5` and `< 6` alike; the thresholds scene shows that the
variants differ in the positions and the histogram only, and the GPU test compares the labels and
the n_moving row at exactly 4 and 5.

Runs with oracle/liboracle_seg.so and, when that file is absent, on seg_oracle's numpy loops.
"""
import functools

import numpy as np
import pytest

import seg_oracle as so
import seg_scenes as sc

PAD = sc.RPAD


def _stages(scene, b, **kw):
    """stages of FOV b of a scene; the unswitched restatement must equal so.get_masks."""
    yf, H, W, geom, call = scene
    call = {k: v for k, v in {**call, **kw}.items() if k != "min_size"}
    rules = {k: call.pop(k) for k in list(call) if k not in ("niter", "resample")}
    st = sc.stages(yf[b], H, W, **geom, **call, **rules)
    if not rules and st["h"] is not None:
        f = so.upsample_flows(yf[b], H, W) if call.get("resample", True) else yf[b]
        np.testing.assert_array_equal(st["labels"], so.get_masks(st["p"], f[2] > so.CELLPROB_THRESHOLD))
    return st


def _final(scene, b, flow_threshold=0.0, **kw):
    yf, H, W, geom, call = scene
    return so.compute_masks(yf[b], H, W, flow_threshold=flow_threshold, **geom, **{**call, **kw})


def _sizes(lab):
    return sorted(np.bincount(lab.ravel())[1:].tolist())


def _differs(a, b):
    return not np.array_equal(a["labels"], b["labels"])


def _cell(st, y, x):
    return int(st["h"][y + PAD, x + PAD])


def _moving_ends(scene, b, st):
    """(y, x) final positions of the moving pixels of FOV b."""
    yf = scene[0][b]
    mov = np.abs((yf[0] * (yf[2] > 0) / np.float32(5.0)).astype(np.float32)) > 1e-3
    return st["p"][0][mov], st["p"][1][mov]


def test_direct_geometry_is_identity():
    """diameter 17: the dynamics run on yf itself (no resize, 200 steps)."""
    assert so.net_size(45, 53, diameter=17.0) == (45, 53) and so.default_niter(diameter=17.0) == 200
    yf = sc.plane_edges()[0][0]
    np.testing.assert_array_equal(so.upsample_flows(yf, 45, 53), yf)


def test_big_boundary():
    scene = sc.big_boundary()
    yf, H, W, _, _ = scene
    n = H * W
    assert (H, W) == (50, 50) and yf.shape[0] == 2 and n * 0.4 == 1000.0
    keep, drop = _stages(scene, 0), _stages(scene, 1)
    sink = (sc.BIG_SINK[0] + PAD, sc.BIG_SINK[1] + PAD)
    assert keep["seeds"][0] == sink and drop["seeds"][0] == sink
    assert keep["m0_counts"].tolist() == [1000, 36] and drop["m0_counts"].tolist() == [1001, 36]
    # exactly 40 %: kept, label 1 (its first pixel is (0, 0)); one pixel more: removed, and the
    # 36-pixel object is renumbered to 1
    assert keep["n_masks"] == 2 and _sizes(keep["labels"]) == [36, 1000] and keep["labels"][0, 0] == 1
    assert drop["n_masks"] == 1 and _sizes(drop["labels"]) == [36] and drop["labels"][36, 22] == 1
    assert _sizes(_final(scene, 0)) == [36, 1000] and _sizes(_final(scene, 1)) == [36]
    wrong = _stages(scene, 0, big_ge=True)
    assert _differs(keep, wrong) and _sizes(wrong["labels"]) == [36]
    assert not _differs(drop, _stages(scene, 1, big_ge=True))


def test_seed_ties():
    scene = sc.seed_ties()
    yf, H, W, _, _ = scene
    assert (H, W) == (41, 61) and yf.shape[0] == 4
    for b, dist in enumerate(sc.TIE_DIST):
        st = _stages(scene, b)
        (ya, xa), (yb, xb) = sc.tie_sinks(dist)
        assert xb - xa == dist and ya == yb
        assert st["seeds"] == [(ya + PAD, xa + PAD), (yb + PAD, xb + PAD)]
        assert _cell(st, ya, xa) == 97 and _cell(st, yb, xb) == 97
        want = [194] if dist == 1 else [97, 97]
        assert _sizes(st["labels"]) == want and _sizes(_final(scene, b)) == want
        if dist == 1:  # both expansions cover both cells; the later seed takes them all
            assert st["m0_counts"].tolist() == [0, 194]
        # only the first of two equal maxima in one window: at distance 2 the second block loses
        # its label (at distance 1 the first seed's expansion covers both cells anyway)
        wrong = _stages(scene, b, first_of_ties=True)
        assert len(wrong["seeds"]) == (1 if dist <= 2 else 2)
        assert _differs(st, wrong) == (dist == 2)
        if dist == 2:
            assert _sizes(wrong["labels"]) == [97]


def test_seed_overlap():
    scene = sc.seed_overlap()
    for b, ys in enumerate((sc.OVERLAP_ROW, sc.OVERLAP_SHAPE[0] - 1 - sc.OVERLAP_ROW)):
        st = _stages(scene, b)
        x0 = sc.OVERLAP_X
        assert st["seeds"] == [(ys + PAD, x0 + PAD), (ys + PAD, x0 + 7 + PAD)]
        assert [_cell(st, ys, x0 + i) for i in range(8)] == [16, 3, 3, 3, 3, 3, 3, 16]
        # B's ball reaches x0 + 2 .. x0 + 7 (radius 5), A keeps x0 and x0 + 1
        assert st["m0_counts"].tolist() == [16 + 3, 16 + 5 * 3]
        wrong = _stages(scene, b, earlier_wins=True)
        assert wrong["m0_counts"].tolist() == [16 + 5 * 3, 16 + 3] and _differs(st, wrong)


def test_thresholds():
    scene = sc.thresholds()
    yf, H, W, _, _ = scene
    assert (H, W) == (31, 35) and yf.shape[0] == 5
    assert (H * W) % 4 == 1 and ((H + 2 * PAD) * (W + 2 * PAD)) % 4 == 1
    for b in (0, 1):
        st = _stages(scene, b)
        lab = st["labels"]
        mov = np.abs(yf[b, 0]) > 0
        up = -1 if b == 0 else 1  # the columns' side of their sink cells
        groups = [sc.thr_cells(down=b == 0, mirror=m) for m in (True, False)]
        assert st["seeds"] == [(g[1][0] + PAD, g[1][1] + PAD) for g in groups]
        for cells in groups:
            assert [_cell(st, y, x) for y, x in cells] == [10, 11, 2, 3, 3]
            assert [bool(lab[y + up, x]) for y, x in cells] == [False, True, False, True, True]
            assert [bool(lab[y, x]) for y, x in cells] == [False, True, False, True, True]
            # every row of a diagonal sink cell is crossed by the seed's column (a moving pixel)
            assert all(mov[y, cells[1][1]] for y, _ in cells[2:])
        assert _sizes(lab) == [17, 17] and _sizes(_final(scene, b)) == [17, 17]
        for rule in (dict(seed_min=10), dict(seed_min=12), dict(good_min=4), dict(good_min=2)):
            assert _differs(st, _stages(scene, b, **rule)), rule
    # exactly 5 and exactly 4 moving pixels (see the module docstring: labels cannot tell)
    five, four = _stages(scene, 2), _stages(scene, 3)
    assert five["n_moving"] == 5 and four["n_moving"] == 4
    assert _cell(five, 12, 11) == 6 and four["h"] is None and not five["labels"].any()
    skipped, followed = _stages(scene, 2, min_moving=6), _stages(scene, 3, min_moving=4)
    assert skipped["h"] is None and _cell(followed, 12, 11) == 5
    assert not np.array_equal(five["p"], skipped["p"]) and not np.array_equal(four["p"], followed["p"])
    assert not _differs(five, skipped) and not _differs(four, followed)
    # seeds on the four plane borders, their columns along the last / first column and into the
    # last / first row
    edge = _stages(scene, 4)
    assert {s for s, _, _ in sc.THR_EDGE_SEEDS} == {(15, W - 1), (8, 0), (H - 1, 15), (0, 24)}
    assert edge["n_moving"] == 4 * 14 and edge["seeds"] == sorted((y + PAD, x + PAD) for (y, x), _, _ in sc.THR_EDGE_SEEDS)
    for (ys, xs), down, step in sc.THR_EDGE_SEEDS:
        assert [_cell(edge, ys, xs + d * step) for d in (0, 1, 2)] == [11, 3, 3]
        far = ys - 10 if down else ys + 10  # the seed column's far end: no field beside it
        assert yf[4, 0, far, xs] != 0 and yf[4, 0, far, xs + step] == 0 and edge["labels"][far, xs] > 0
    assert _sizes(edge["labels"]) == [17] * 4 and _sizes(_final(scene, 4)) == [17] * 4
    for rule in (dict(seed_min=12), dict(good_min=4)):
        assert _differs(edge, _stages(scene, 4, **rule)), rule


def test_plane_edges():
    scene = sc.plane_edges()
    yf, H, W, _, _ = scene
    assert (H, W) == (45, 53)
    st = _stages(scene, 0)
    assert st["seeds"] == sorted((y + PAD, x + PAD) for y, x in sc.EDGE_SEEDS)
    py, px = _moving_ends(scene, 0, st)
    assert py.size == st["n_moving"] == 8 * 64
    for ends, edge in ((py, 0), (py, H - 1), (px, 0), (px, W - 1)):
        assert (ends == edge).sum() == 3 * 64  # two corners and one edge object on every border
    assert ((py < 1) | (px < 1)).sum() == 5 * 64 and ((py >= 1) & (px >= 1)).sum() == 3 * 64
    lab = st["labels"]
    assert _sizes(lab) == [64] * 8 and _sizes(_final(scene, 0)) == [64] * 8
    for (r, c, _) in sc.EDGE_OBJS:
        assert len(np.unique(lab[r[0]:r[1] + 1, c[0]:c[1] + 1])) == 1


@functools.lru_cache(maxsize=None)
def _round_stages(niter):
    return _stages(sc.round_edges(), 0, niter=niter)


@pytest.mark.parametrize("N", sc.ROUND_EDGES + (1176,))
def test_round_edges(N):
    """One step fewer or more changes the labels at every round boundary of the follow loop."""
    assert sc.ROUND_EDGES == (16, 384, 512)
    scene = sc.round_edges()
    steps = (N - 1, N) if N == 1176 else (N - 1, N, N + 1)
    labs = [_round_stages(n)["labels"] for n in steps]
    fin = [_final(scene, 0, niter=n) for n in steps]
    for i in range(len(steps)):
        for j in range(i):
            assert not np.array_equal(labs[i], labs[j]) and not np.array_equal(fin[i], fin[j]), (steps[i], steps[j])
    for n in steps:  # the timer of step M: its fourth pixel joins the label at step M, not before
        for M in (m for m in steps if m in sc.ROUND_TIMERS):
            x = sc.timer_column(M)
            lab = _round_stages(n)["labels"]
            assert (lab[sc.ROUND_ROW + 4, x] == 1) == (n >= M), (n, M)
            assert lab[sc.ROUND_ROW + 3, x] == 1


def test_round_edges_scene():
    assert set(sc.ROUND_NITER) >= set(sc.ROUND_TIMERS) and sc.ROUND_SHAPE == (40, 43)
    st = _round_stages(1176)
    assert st["seeds"] == [(sc.ROUND_ROW + PAD, sc.ROUND_X + PAD)] and st["n_moving"] == 12 + 10 * 2 + 11 * 4
    assert _sizes(st["labels"]) == [st["n_moving"] + 11]  # every follower and the eleven sink cells


def test_min_size_edge():
    scene = sc.min_size_edge()
    st = _stages(scene, 0)
    assert _sizes(st["labels"]) == [14, 15]
    assert _sizes(_final(scene, 0, min_size=15)) == [15]
    assert _sizes(_final(scene, 0, min_size=0)) == [14, 15]
    assert _sizes(_final(scene, 0, min_size=14)) == [14, 15] and _sizes(_final(scene, 0, min_size=16)) == []


@pytest.mark.parametrize("shape", sc.ODD_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_odd_shapes(shape):
    H, W = shape
    n, nh = H * W, (H + 2 * PAD) * (W + 2 * PAD)
    assert (n % 4, nh % 4) == {(301, 323): (3, 3), (302, 325): (2, 2), (299, 321): (3, 3)}[shape]
    scene = sc.odd_shapes(H, W)
    assert scene[0].shape[0] == 3 and not (scene[0][2, 2] > 0).any()
    touches = False
    for b in (0, 1):
        st = _stages(scene, b)
        fin = _final(scene, b, flow_threshold=so.FLOW_THRESHOLD)
        assert st["n_masks"] >= 4 and fin.max() >= 4, (b, st["n_masks"], fin.max())
        touches |= bool(fin[0].any() or fin[-1].any() or fin[:, 0].any() or fin[:, -1].any())
    assert touches
    assert not _final(scene, 2).any() and _stages(scene, 2)["n_moving"] == 0
    # resample=False: the dynamics at the network size, itself no multiple of 4 for two shapes
    net = sc.odd_shapes(H, W, resample=False)
    Ly, Lx = so.net_size(H, W)
    assert net[4] == {"resample": False} and net[0].shape[2:] == (Ly, Lx)
    for b in (0, 1):
        assert _stages(net, b)["n_masks"] >= 4 and _final(net, b, flow_threshold=so.FLOW_THRESHOLD).max() >= 4


def test_oracle_stats_rows():
    scene = sc.big_boundary()
    yf, H, W, geom, call = scene
    assert sc.oracle_rows(yf[1], H, W, **geom, **call) == {"n_moving": 1036, "n_seeds_found": 2, "n_masks": 1}
    np.testing.assert_array_equal(sc.oracle_labels(yf[1], H, W, 0.0, **geom, **call, min_size=15), _final(scene, 1))
