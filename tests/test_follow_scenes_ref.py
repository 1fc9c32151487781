"""CPU: the follower scenes (tests/follow_scenes.py) are what they claim to be, so a GPU mismatch on
them (tests/test_gpu_follow_pairs.py) is a kernel bug and not a scene artefact.  Every test first
checks that follow_scenes.follow, unswitched, gives seg_oracle.follow_flows' positions bit for bit,
then asserts the scene's condition on the recorded trajectories and that the wrong variant of the
rule the scene is there for changes the label image.

Runs with oracle/liboracle_seg.so and, when that file is absent, on seg_oracle's numpy loops.
"""
import functools

import numpy as np
import pytest

import follow_scenes as fs
import seg_oracle as so

K0 = 16  # k_seg.hip: steps per round while most pixels still move


@functools.lru_cache(maxsize=None)
def _scene(name):
    return fs.SCENES[name]()


@functools.lru_cache(maxsize=None)
def _follow(name, b):
    """The unswitched trajectories of FOV b, checked against the oracle."""
    yf = _scene(name)[0][b]
    f = fs.follow(yf)
    p, _ = so.follow_flows(yf[:2], yf[2] > so.CELLPROB_THRESHOLD, fs.NITER)
    np.testing.assert_array_equal(f["p"], p)
    return f


def _labels(name, b, **switches):
    yf = _scene(name)[0][b]
    f = fs.follow(yf, **switches) if switches else _follow(name, b)
    return fs.labels_of(yf, f["p"])


def _sizes(lab):
    return sorted(np.bincount(lab.ravel())[1:].tolist())


def test_geometry():
    assert so.default_niter(diameter=17.0) == fs.NITER
    for name in fs.SCENES:
        yf, H, W, geom, _ = _scene(name)
        assert yf.shape[2:] == (H, W) == so.net_size(H, W, **geom) and H * W <= 2048 and max(H, W) <= 64


@pytest.mark.parametrize("N", fs.COUNTS)
def test_pair_counts(N):
    name = f"pair_counts_{N}"
    f = _follow(name, 0)
    assert f["iy"].size == N
    # threads with a second item, and whether the last item opens a half of its own
    assert sum(i % (2 * fs.PAIR) >= fs.PAIR for i in range(N)) == {256: 0, 257: 1, 512: 256, 513: 256}[N]
    assert ((N - 1) % fs.PAIR == 0) == (N in (257, 513))
    lab = _labels(name, 0)
    assert len(_sizes(lab)) >= 3 and lab[f["iy"][N - 1], f["ix"][N - 1]] > 0
    # the last item lost: its pixel stays where it is and drops out of its label
    assert not np.array_equal(_labels(name, 0, skip=(N - 1,)), lab)


@pytest.mark.parametrize("b", [0, 1])
def test_partners(b):
    f = _follow("partners", b)
    N, st, g, lit = f["iy"].size, f["stopped"], f["gathered"], f["literal"]
    assert 2 * fs.PAIR < N <= 2048
    pairs = [(i, i + fs.PAIR) for i in range(N) if i % (2 * fs.PAIR) < fs.PAIR and i + fs.PAIR < N]
    rounds3 = 3 * K0
    # one item on its exact fixed point after step 1, its partner moving through three rounds and more
    early = [(i, j) for i, j in pairs if min(st[i], st[j]) == 1 and max(st[i], st[j]) > rounds3]
    assert early, "no pair (stops in step 1, runs on)"
    # one item in the literal top / left expression while its partner takes the fast one
    mixed = [(i, j) for i, j in pairs if (lit[:rounds3, i] & ~lit[:rounds3, j]).all()]
    assert mixed, "no pair (literal, fast)"
    # one item in an unchanged cell for 12 steps in a row while its partner gathers at
    # every one of them: the first of the pair sits (FOV 0) or the second (FOV 1)
    def sits(i, j):
        run = 0
        for s in range(1, fs.NITER):
            run = run + 1 if (not g[s, i] and g[s, j]) else 0
            if run >= 12:
                return True
        return False
    first_sits = [(i, j) for i, j in pairs if sits(i, j)]
    second_sits = [(i, j) for i, j in pairs if sits(j, i)]
    assert (first_sits if b == 0 else second_sits), "no pair (sits, gathers)"
    # a thread that stops both items when one has arrived loses the other's label
    lab = _labels("partners", b)
    assert len(_sizes(lab)) == 3
    assert not np.array_equal(_labels("partners", b, couple=True), lab)


def test_returning():
    f = _follow("returning", 0)
    W = _scene("returning")[2]
    cells = f["pos"][:, 0].astype(np.int64) * W + f["pos"][:, 1].astype(np.int64)
    back = 0
    for i in range(cells.shape[1]):
        c, seen = cells[:, i], {}
        for s, v in enumerate(c):
            if v in seen and c[s - 1] != v:
                back += 1
                break
            seen[v] = s
    assert back >= cells.shape[1] // 2  # most trajectories leave a cell and come back to it
    lab = _labels("returning", 0)
    assert _sizes(lab) and lab.max() == 1
    # taps kept across a move that changes only the other coordinate of the cell: wrong positions
    for key in ("x", "y"):
        assert not np.array_equal(_labels("returning", 0, key=key), lab)


@pytest.mark.parametrize("name", [n for n in fs.SCENES if n.startswith("buffer_edges")])
def test_buffer_edges(name):
    yf, Dy, Dx, _, _ = _scene(name)
    f = _follow(name, 0)
    ends = set(zip(f["pos"][-1, 0].astype(int).tolist(), f["pos"][-1, 1].astype(int).tolist()))
    assert ends == {(15, Dx - 1), (Dy - 1, Dx - 1)} | ({(Dy - 1, Dx // 2)} if Dx > 2 else set())
    assert (f["stopped"] < fs.NITER).all()
    lab = _labels(name, 0)
    assert lab[Dy - 1, Dx - 1] > 0 and _sizes(lab) == [15] * len(ends)
    # the tap on the last column taken from the column beside it: NaN positions, or (a zero
    # field there; for Dx == 2 the other column's followers) pixels that stop short
    wrong = fs.follow(yf[0], right_tap_left=True)["p"]
    if "nan" in name:
        assert np.isnan(fs.dynamics_field(yf[0])[:, :, Dx - 2]).all() and np.isnan(wrong).any()
    else:
        assert not np.array_equal(fs.labels_of(yf[0], wrong), lab)
    _follow(name, 1)


def test_scalar_path():
    yf, Dy, Dx, _, _ = _scene("scalar_path")
    assert Dx == 1
    f = _follow("scalar_path", 0)
    assert f["iy"].size == 2 * fs.EDGE_COL and (f["stopped"] < fs.NITER).all()
    assert _sizes(_labels("scalar_path", 0)) == [15, 15]
