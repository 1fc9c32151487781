"""Procedural edge-case scenes for the feature kernels (k_texture.hip / k_features.hip), shared
by the CPU precondition test and the GPU test.  A scene is (labels [B, H, W] int32,
planes [B, C, H, W] float32) with C = 2; widths are odd and no multiple of 4.

Plain helper module for tests (no fixtures, not collected).
"""
from __future__ import annotations

import functools

import numpy as np

import cpx_oracle as orc

SCENES = ("tiny", "borders", "topology", "widths", "counters", "steps", "band_crop", "dense_crop",
          "px65535", "mask_words", "intensity")
PAIR_SCENES = ("borders", "topology")
TWICE_SCENES = ("counters", "steps", "dense_crop")  # band, list and redo items mixed in one launch


def _field(rng, H, W, lo=200.0, hi=6000.0):
    """Two unrelated positive planes: uniform noise on a smooth ramp."""
    yy, xx = np.mgrid[0:H, 0:W]
    p0 = rng.uniform(lo, hi, (H, W)) + 3.0 * yy + 2.0 * xx
    p1 = rng.uniform(lo, hi, (H, W)) * (1.0 + 0.5 * np.sin(xx / 7.0) * np.cos(yy / 5.0))
    return np.stack([p0, p1]).astype(np.float32)


def tiny():
    """Objects smaller than the GLCM offsets (0,3), (2,2), (3,0), (2,-2) in one or both directions."""
    H, W = 41, 67
    lab = np.zeros((H, W), np.int32)
    lab[3, 5] = 1                      # 1 px
    lab[3, 12:14] = 2                  # 1 x 2
    lab[3:5, 20] = 3                   # 2 x 1
    lab[3:5, 27:29] = 4                # 2 x 2
    lab[3, 35:42] = 5                  # 1 x 7 line
    lab[10:17, 5] = 6                  # 7 x 1 line
    for k in range(5):                 # 5-px diagonal, 8-connected only
        lab[10 + k, 12 + k] = 7
    lab[10, 24] = lab[11, 24] = lab[11, 25] = 8   # 3-px L
    lab[10:13, 32] = 9                 # plus
    lab[11, 31:34] = 9
    lab[10:13, 40:43] = 10             # 3 x 3
    lab[20:22, 5:12] = 11              # 2 x 7: wide enough for (0,3) only
    lab[20:27, 20:22] = 12             # 7 x 2: tall enough for (3,0) only
    lab[38:41, 62:67] = 13             # 3 x 5 in the plane's last pixels
    return lab[None], _field(np.random.default_rng(11), H, W)[None]


def borders():
    """Objects on all four corners and edges of a 61 x 67 image, two FOVs.  FOV 1 is FOV 0
    turned by 180 degrees, so the last pixels of FOV 0 and the first pixels of FOV 1 carry the same
    label with other intensities; channel 0's last row (~1e2) and channel 1's first row (~5e4)
    differ strongly."""
    H, W = 61, 67
    yy, xx = np.mgrid[0:H, 0:W]
    lab = np.zeros((H, W), np.int32)
    lab[(yy < 6) & (xx < 9) & (yy + xx < 12)] = 1                      # top-left corner
    lab[(yy < 7) & (xx >= W - 5)] = 2                                  # top-right corner
    lab[(yy >= H - 4) & (xx < 11) & (xx - (yy - (H - 4)) < 9)] = 3     # bottom-left corner
    lab[(yy >= H - 9) & (xx >= W - 6) & ((H - 1 - yy) + (W - 1 - xx) < 11)] = 4  # bottom-right corner
    lab[((yy - 0) / 7.0) ** 2 + ((xx - 30 + 0.4 * yy) / 11.0) ** 2 <= 1.0] = 5   # top edge
    lab[((yy - (H - 1)) / 9.0) ** 2 + ((xx - 36) / 6.0) ** 2 <= 1.0] = 6        # bottom edge
    lab[((yy - 30 - 0.3 * xx) / 10.0) ** 2 + (xx / 8.0) ** 2 <= 1.0] = 7        # left edge
    lab[((yy - 28) / 6.0) ** 2 + ((xx - (W - 1)) / 12.0) ** 2 <= 1.0] = 8       # right edge
    labs = np.stack([lab, lab[::-1, ::-1]]).astype(np.int32)
    rng = np.random.default_rng(12)
    planes = np.stack([np.stack([rng.uniform(50.0, 150.0, (H, W)), rng.uniform(40000.0, 60000.0, (H, W))])
                       for _ in range(2)]).astype(np.float32)
    return labs, planes


def topology():
    """Exactly symmetric objects (disc, square, diamond, annulus), holes, one label in two distant
    components, a checkerboard-labelled object, two labels interleaved in one bbox."""
    H, W = 150, 263
    yy, xx = np.mgrid[0:H, 0:W]
    lab = np.zeros((H, W), np.int32)
    lab[(yy - 24) ** 2 + (xx - 24) ** 2 <= 400] = 1                    # disc r = 20
    lab[4:25, 52:73] = 2                                               # 21 x 21 square
    lab[np.abs(yy - 20) + np.abs(xx - 96) <= 15] = 3                   # 31 x 31 diamond
    d2 = (yy - 24) ** 2 + (xx - 140) ** 2
    lab[(d2 <= 18 ** 2) & (d2 > 10 ** 2)] = 4                          # annulus: centroid outside
    lab[60:90, 5:45] = 5                                               # holes
    lab[65:70, 10:18] = 0
    lab[75:86, 30:33] = 0
    lab[80, 12] = 0
    lab[(yy - 60) ** 2 + (xx - 170) ** 2 <= 49] = 6                    # two distant components
    lab[((yy - 135) / 9.0) ** 2 + ((xx - 250) / 11.0) ** 2 <= 1.0] = 6
    cb = (yy >= 100) & (yy < 116) & (xx >= 60) & (xx < 81)
    lab[cb & ((yy + xx) % 2 == 0)] = 7                                 # every pixel a border pixel
    il = (yy >= 100) & (yy < 118) & (xx >= 100) & (xx < 131)
    lab[il & (xx % 3 == 0)] = 8                                        # two labels in one bbox
    lab[il & (xx % 3 != 0) & (yy % 4 < 2)] = 9
    lab[il & (yy == 100)] = 9
    lab[il & (xx == 130)] = 9
    return lab[None], _field(np.random.default_rng(13), H, W)[None]


def widths():
    """Filled rectangles 3..19 wide, 3..6 high: every row-width residue mod 8."""
    H, W = 53, 131
    lab = np.zeros((H, W), np.int32)
    for k, w in enumerate(range(3, 20)):
        r0, c0 = 2 + 12 * (k // 5), 1 + 26 * (k % 5)
        lab[r0:r0 + 3 + k % 4, c0:c0 + w] = k + 1
    return lab[None], _field(np.random.default_rng(14), H, W)[None]


def _levels_plane(rng, lab, ch0):
    """Channel 0 holds the wanted 8-bit levels as values (an object with one masked or zero pixel
    in its bbox and one at 255 quantises 255 * (v - 0) / 255 == v in fp32); channel 1 is noise."""
    return np.stack([ch0, rng.uniform(100.0, 9000.0, lab.shape)]).astype(np.float32)


def counters():
    """FOV 0: a filled 255 x 257 object, all 255 but one pixel: almost every pair on one u16
    counter.  FOV 1: the same with a uniform-noise patch that pushes every angle's outlier list
    past 512: the dense redo path."""
    H, W = 259, 263
    rng = np.random.default_rng(15)
    lab = np.zeros((H, W), np.int32)
    lab[2:257, 3:260] = 1
    lab[0, 0:2] = 2  # a second, tiny object in the same launch
    p0 = np.full((H, W), 255.0)
    p0[130, 100] = 0.0
    p1 = p0.copy()
    p1[40:90, 60:120] = rng.integers(1, 256, (50, 60))
    return (np.stack([lab, lab]),
            np.stack([_levels_plane(rng, lab, p0), _levels_plane(rng, lab, p1)]))


def steps():
    """Two-level objects with level differences exactly 31 (in the band) and 32 (outliers), and
    objects with exactly 512 (the outlier list full) and 513 (overflow: redo) outliers in the
    worst angle: 256 isolated low pixels on a 4-px grid in a field of 255 give two outlier pairs
    each in every angle; the 513th comes from a low pixel in the bbox's last corner (one pair in
    three angles, none in the fourth)."""
    H, W = 90, 179
    rng = np.random.default_rng(16)
    lab = np.zeros((H, W), np.int32)
    p0 = np.full((H, W), 255.0)
    for k, lo in enumerate((224.0, 223.0)):  # |i - j| = 31, 32
        r0, c0 = 2, 3 + 30 * k
        lab[r0:r0 + 13, c0:c0 + 21] = k + 1
        lab[r0, c0] = 0                      # the masked pixel
        p0[r0:r0 + 13, c0:c0 + 10] = lo
    for k in range(2):
        r0, c0 = 18, 2 + 88 * k
        lab[r0:r0 + 70, c0:c0 + 71] = 3 + k
        lab[r0, c0] = 0
        p0[r0 + 4:r0 + 66:4, c0 + 4:c0 + 66:4][:16, :16] = 100.0
        if k == 1:
            p0[r0 + 69, c0 + 70] = 100.0
    return lab[None], _levels_plane(rng, lab, p0)[None]


def _limit_scene(seed, sizes, H, W, noise):
    """One object per FOV with the bbox sizes given, a corner cut off (masked pixels, no symmetry);
    noise: uniform noise inside (thousands of outliers: the dense kernel), else a smooth blob."""
    rng = np.random.default_rng(seed)
    labs, planes = [], []
    for bh, bw in sizes:
        yy, xx = np.mgrid[0:H, 0:W]
        lab = np.zeros((H, W), np.int32)
        lab[1:1 + bh, 2:2 + bw] = 1
        lab[(yy - 1) + (xx - 2) < 9] = 0
        lab[1, 2 + 9:2 + bw] = 1  # the bbox stays bh x bw
        lab[1:1 + bh, 2] = np.where(np.arange(bh) >= 9, 1, lab[1:1 + bh, 2])
        p = _field(rng, H, W)
        if noise:
            p[0] = rng.uniform(100.0, 20000.0, (H, W))
        else:
            p[0] = 300.0 + 5000.0 * np.exp(-(((yy - bh / 2) / bh) ** 2 + ((xx - bw / 3) / bw) ** 2) * 4.0) \
                + rng.normal(0.0, 15.0, (H, W))
        labs.append(lab)
        planes.append(p.astype(np.float32))
    return np.stack(labs), np.stack(planes)


def band_crop():
    """k_tex_band stages crops of up to kBandCrop = 16384 bytes in LDS: 93 x 171 is exactly
    16384 (rows of 176), 94 x 171 reads from global memory."""
    return _limit_scene(17, [(93, 171), (94, 171)], 99, 179, noise=False)


def dense_crop():
    """k_tex_glcm (the redo path) holds crops of up to kCrop = 30128 bytes in LDS: 171 x 171 is
    30112, 172 x 171 is 30288."""
    return _limit_scene(18, [(171, 171), (172, 171)], 177, 179, noise=True)


def px65535():
    """bbox of 65535 px (the LDS paths' u16 counters hold it) and of 65792 px (fallback)."""
    return _limit_scene(19, [(255, 257), (256, 257)], 259, 263, noise=False)


def mask_words():
    """cpx_shape_fits: (bh + 4) * ceil((bw + 4) / 32) <= 4096 words: 405 x 285 fits (4090), 406 x 285
    does not (4100): AreaShape from k_shape."""
    return _limit_scene(20, [(405, 285), (406, 285)], 409, 291, noise=False)


def intensity():
    """Channel 0: objects whose variance is tiny beside mean^2.  FOV 0: a constant non-integer
    fp32 value over 200 x 200 (LDS path), 70000 + k ulp noise, six decades in one object.  FOV 1:
    the constant over 260 x 262 (> 65535 px: fallback), 70000 + k ulp noise.  Channel 1: a signed
    plane, negative inside and outside every object."""
    H, W = 300, 263
    rng = np.random.default_rng(21)
    const = np.float32(65535 / 0.9137)
    ulp = float(np.spacing(np.float32(70000.0)))
    labs = np.zeros((2, H, W), np.int32)
    p = rng.uniform(100.0, 900.0, (2, 2, H, W))
    p[:, 1] = rng.normal(0.0, 1000.0, (2, H, W))
    labs[0, 3:203, 2:202] = 1
    p[0, 0, 3:203, 2:202] = const
    labs[0, 10:130, 206:259] = 2
    labs[0, 10, 206] = 0
    p[0, 0, 10:130, 206:259] = 70000.0 + ulp * rng.integers(-3, 4, (120, 53))
    labs[0, 210:290, 10:87] = 3
    labs[0, 210:215, 10:30] = 0
    p[0, 0, 210:290, 10:87] = 10.0 ** rng.uniform(0.0, 6.0, (80, 77))
    labs[1, 0:260, 0:262] = 1
    p[1, 0, 0:260, 0:262] = const
    labs[1, 264:298, 5:142] = 2
    labs[1, 264, 5:9] = 0
    p[1, 0, 264:298, 5:142] = 70000.0 + ulp * rng.integers(-3, 4, (34, 137))
    return labs, p.astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene(name):
    """(labels, planes) of a scene, built once per process; treat as read-only."""
    assert name in SCENES, name
    labs, planes = globals()[name]()
    labs, planes = np.ascontiguousarray(labs, np.int32), np.ascontiguousarray(planes, np.float32)
    labs.setflags(write=False)
    planes.setflags(write=False)
    return labs, planes


@functools.lru_cache(maxsize=None)
def exact(name):
    """Per FOV (rows, diags) of the exact reference, computed once per process."""
    import features_exact as fx
    labs, planes = scene(name)
    return [fx.features(labs[b], planes[b]) for b in range(labs.shape[0])]


@functools.lru_cache(maxsize=None)
def pair_sets(name):
    """Cells = the objects dilated by 3 px (skimage expand_labels), Cytoplasm = Cells minus the
    objects, per FOV, and their exact references."""
    import features_exact as fx
    labs, planes = scene(name)
    cells = np.stack([orc.expand_labels(labs[b], 3) for b in range(labs.shape[0])]).astype(np.int32)
    cyto = np.where(labs == 0, cells, 0).astype(np.int32)
    ref = [[fx.features(s[b], planes[b]) for b in range(labs.shape[0])] for s in (cells, cyto)]
    return cells, cyto, ref
