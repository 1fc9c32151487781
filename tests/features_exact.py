"""Exact reference of the AreaShape / Intensity / Texture columns, and the per-column comparator.

`features(labels, planes)` returns the layout of `cpx_oracle.features` ([n_objects, 15 + 29 C],
ascending label order) computed without floating-point sums: every AreaShape and Texture column
is a function of integer sums, formed here as Python ints / `fractions.Fraction` and converted
to float only at the last sqrt / atan2; the Intensity columns come from `math.fsum` (the
correctly rounded sum) and a two-pass variance.  The 8-bit quantiser (`cpx_oracle.texture_input`,
fp32 by definition) and the erosion / convolution that classify perimeter pixels are the
oracle's.  Alongside every row comes a dict of diagnostics that the scene tests assert on.

`compare(got, ref, diags)` checks a kernel result column class by column class with tolerances
derived from the arithmetic, not from what the kernels give (parity section).

Plain helper module for tests (no fixtures, not collected).
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np
from scipy import ndimage as ndi

import cpx_oracle as orc

OFFS = [(0, 3), (2, 2), (3, 0), (2, -2)]  # (dr, dc) of the four GLCM angles at distance 3
BAND_D = 31                                # k_tex_band's band half-width (k_texture.hip kBandD)
N_SHAPE, N_INT, N_TEX = 15, 5, 24
PER_CH = N_INT + N_TEX
_K = 80                                    # fractional bits of the integer square root below


def _sqrt_frac(num: int, den: int = 1) -> Fraction:
    """sqrt(num / den) to 2^-_K relative, as a Fraction (num, den non-negative ints)."""
    if num == 0:
        return Fraction(0)
    s = max(0, 2 * _K - num.bit_length() + den.bit_length())
    s += s & 1
    return Fraction(math.isqrt((num << s) // den if den != 1 else num << s), 1 << (s // 2))


def perimeter_counts(img: np.ndarray):
    """The three Benkrid-Crookes code counts of skimage's perimeter (oracle's erosion and
    convolution): weights 1, sqrt 2, (1 + sqrt 2) / 2."""
    image = img.astype(np.uint8)
    eroded = ndi.binary_erosion(image, orc._STREL_4, border_value=0)
    border = image - eroded
    pimg = ndi.convolve(border, np.array([[10, 2, 10], [2, 1, 2], [10, 2, 10]]), mode="constant", cval=0)
    hist = np.bincount(pimg.ravel(), minlength=50)
    return (int(hist[[5, 7, 15, 17, 25, 27]].sum()), int(hist[[21, 33]].sum()), int(hist[[13, 23]].sum()))


def shape_row(img: np.ndarray, sl):
    rr, cc = np.nonzero(img)
    rr, cc = rr.astype(object), cc.astype(object)  # Python ints from here on
    n = len(rr)
    sr, sc = int(rr.sum()), int(cc.sum())
    srr, scc, src = int((rr * rr).sum()), int((cc * cc).sum()), int((rr * cc).sum())
    m20 = n * srr - sr * sr  # n^2 mu20 / mu0 (rows)
    m02 = n * scc - sc * sc  # columns
    m11 = n * src - sr * sc
    # skimage inertia tensor [[a, b], [b, c]] = [[mu02, -mu11], [-mu11, mu20]] / mu0, all * n^2 here
    S, D = m02 + m20, (m02 - m20) ** 2 + 4 * m11 * m11
    rtD = _sqrt_frac(D)
    n2 = n * n
    l1 = (S + rtD) / (2 * n2)
    l2 = Fraction(4 * (m02 * m20 - m11 * m11)) / (2 * n2 * (S + rtD)) if S else Fraction(0)
    ecc2 = 2 * rtD / (S + rtD) if S else Fraction(0)  # 1 - l2 / l1
    if m02 - m20 == 0:  # skimage: a - c == 0 -> -pi/4 if b < 0 else pi/4 (b = -mu11 / mu0)
        orient = -math.pi / 4.0 if m11 > 0 else math.pi / 4.0
    else:
        orient = 0.5 * math.atan2(float(2 * m11), float(m20 - m02))
    n1, nq, nh = perimeter_counts(img)
    r0, c0, r1, c1 = sl[0].start, sl[1].start, sl[0].stop, sl[1].stop
    bba = (r1 - r0) * (c1 - c0)
    row = [float(n), n1 + nq * math.sqrt(2.0) + nh * ((1.0 + math.sqrt(2.0)) / 2.0),
           float(Fraction(sr, n) + r0), float(Fraction(sc, n) + c0), float(bba), float(Fraction(n, bba)),
           math.sqrt(4.0 * n / math.pi), 4.0 * math.sqrt(float(l1)), 4.0 * math.sqrt(float(l2)),
           math.sqrt(float(ecc2)), orient, float(r0), float(c0), float(r1), float(c1)]
    diag = dict(n=n, bbox=(r0, c0, r1, c1), a_minus_c=Fraction(m02 - m20, n2), b=Fraction(-m11, n2),
                a_plus_c=Fraction(S, n2), l1_eq_l2=(D == 0), ecc2=float(ecc2), perim_counts=(n1, nq, nh))
    return row, diag


def glcm_pairs(q8: np.ndarray, dr: int, dc: int):
    """The (i, j) values of every pair of skimage's greycomatrix at offset (dr, dc), dr >= 0."""
    h, w = q8.shape
    r1 = h - dr
    c0, c1 = (0, w - dc) if dc >= 0 else (-dc, w)
    if r1 <= 0 or c1 <= c0:
        z = np.zeros(0, np.int64)
        return z, z
    a = q8[:r1, c0:c1].astype(np.int64).ravel()
    b = q8[dr:dr + r1, c0 + dc:c1 + dc].astype(np.int64).ravel()
    return a, b


def texture_angle(q8: np.ndarray, dr: int, dc: int):
    """greycoprops [contrast, dissimilarity, homogeneity, ASM, energy, correlation] of one angle
    from integer sums, and the angle's diagnostics."""
    a, b = glcm_pairs(q8, dr, dc)
    T = int(a.size)
    if T == 0:
        return [0.0, 0.0, 0.0, 0.0, 0.0, 1.0], dict(T=0, max_key=0, outliers=0)
    P = np.bincount(a * 256 + b, minlength=65536)
    si, sj = int(a.sum()), int(b.sum())
    sii, sjj, sij = int((a * a).sum()), int((b * b).sum()), int((a * b).sum())
    nd = np.bincount(np.abs(a - b), minlength=256)
    sabs = int(np.abs(a - b).sum())
    sc2 = int((P.astype(object) ** 2).sum()) if P.max() > 3_000_000_000 else int((P * P).sum())
    hom = sum(Fraction(int(c), 1 + d * d) for d, c in enumerate(nd) if c)
    vi, vj, cv = T * sii - si * si, T * sjj - sj * sj, T * sij - si * sj
    if vi == 0 or vj == 0:
        cor = 1.0
    else:
        cor = math.copysign(math.sqrt(float(Fraction(cv * cv, vi * vj))), cv) if cv else 0.0
    asm = Fraction(sc2, T * T)
    Pn = P.copy()
    Pn[0] = 0  # the background key (0, 0) has no counter in the kernels
    diag = dict(T=T, max_key=int(Pn.max()),
                outliers=int(((a > 0) & (b > 0) & (np.abs(a - b) > BAND_D)).sum()))
    return [float(Fraction(sii + sjj - 2 * sij, T)), float(Fraction(sabs, T)), float(hom / T), float(asm),
            math.sqrt(float(asm)), cor], diag


def intensity_row(vals32: np.ndarray):
    v = vals32.astype(np.float64)
    n = v.size
    s = math.fsum(v.tolist())
    mean = s / n
    var = math.fsum(((v - mean) ** 2).tolist()) / n
    return ([s, mean, math.sqrt(var), float(vals32.min()), float(vals32.max())],
            dict(sum_abs=math.fsum(np.abs(v).tolist())))


def features(labels: np.ndarray, planes: np.ndarray, q8_hook=None):
    """(rows [n_objects, 15 + 29 C] float64, diags: one dict per object).  q8_hook(q8, label, ch)
    may return a modified 8-bit crop (the teeth test's deliberately wrong kernel)."""
    C = planes.shape[0]
    rows, diags = [], []
    for i, sl in enumerate(ndi.find_objects(labels)):
        if sl is None:
            continue
        label = i + 1
        img = labels[sl] == label
        row, diag = shape_row(img, sl)
        diag.update(label=label, channels=[])
        for ch in range(C):
            ir, idiag = intensity_row(planes[ch][sl][img])
            row += ir
            q8 = orc.texture_input(planes[ch], labels, sl, label)
            if q8_hook is not None:
                q8 = q8_hook(q8, label, ch)
            idiag.update(levels=sorted(int(x) for x in np.unique(q8[img])), angles=[])
            for dr, dc in OFFS:
                tr, tdiag = texture_angle(q8, dr, dc)
                row += tr
                idiag["angles"].append(tdiag)
            diag["channels"].append(idiag)
        rows.append(row)
        diags.append(diag)
    C29 = N_SHAPE + C * PER_CH
    return np.array(rows, dtype=np.float64).reshape(len(rows), C29), diags


# ----------------------------------------------------------------------------------------------
# comparator

EQUAL_SHAPE = [0, 4, 11, 12, 13, 14]  # Area, BoundingBoxArea, BoundingBox*
CENTER = [2, 3]
TIGHT_SHAPE = [1, 5, 6, 7, 8]         # Perimeter, Extent, EquivalentDiameter, Major/MinorAxisLength
ECC, ORIENT = 9, 10
CLASSES = ("equal", "center", "shape", "ecc2", "orient", "texture", "sum", "std")


def orientation_class(diag) -> str:
    """'symmetric' (a - c == 0 exactly), 'conditioned' (|a - c| + |b| > 1e-6 (a + c)), or
    'ill' — the scenes hold none of the last kind."""
    if diag["a_minus_c"] == 0:
        return "symmetric"
    if abs(diag["a_minus_c"]) + abs(diag["b"]) > Fraction(1, 10 ** 6) * diag["a_plus_c"]:
        return "conditioned"
    return "ill"


def compare(got: np.ndarray, ref: np.ndarray, diags, what: str = "") -> dict:
    """Assert `got` against the exact reference, every column by its class; returns the largest
    error seen per class (relative for shape / texture / std, in units of the bound for sum)."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    C = (ref.shape[1] - N_SHAPE) // PER_CH
    worst = dict.fromkeys(CLASSES, 0.0)
    bad = []

    def note(cls, err, ok, k, col, g, r):
        worst[cls] = max(worst[cls], float(err))
        if not ok:
            bad.append(f"{what} object {k} (label {diags[k]['label']}) column {col} [{cls}]: got {g!r} ref {r!r}")

    def rel(g, r):
        return abs(g - r) / abs(r) if r != 0 else abs(g)

    for k, d in enumerate(diags):
        g, r = got[k], ref[k]
        for c in EQUAL_SHAPE:
            note("equal", 0.0 if g[c] == r[c] else 1.0, g[c] == r[c], k, c, g[c], r[c])
        for c in CENTER:
            note("center", 0.0 if g[c] == r[c] else 1.0, g[c] == r[c], k, c, g[c], r[c])
        for c in TIGHT_SHAPE:
            note("shape", rel(g[c], r[c]), abs(g[c] - r[c]) <= 1e-12 + 1e-12 * abs(r[c]), k, c, g[c], r[c])
        e = abs(g[ECC] ** 2 - d["ecc2"])
        note("ecc2", e, e <= 1e-12, k, ECC, g[ECC], r[ECC])
        dd = abs(g[ORIENT] - r[ORIENT])
        if orientation_class(d) == "symmetric":  # skimage's rule on the exact b: +-pi/4, no other branch
            note("orient", dd, g[ORIENT] == r[ORIENT], k, ORIENT, g[ORIENT], r[ORIENT])
        else:  # an axis: modulo pi (a horizontal line is +-pi/2 by the sign of a zero)
            e = min(dd, abs(math.pi - dd))
            note("orient", e, e <= 1e-12, k, ORIENT, g[ORIENT], r[ORIENT])
        for ch in range(C):
            o = N_SHAPE + ch * PER_CH
            bound = 4.0 * d["n"] * 2.0 ** -53 * d["channels"][ch]["sum_abs"]
            for c, b in ((o, bound), (o + 1, bound / d["n"])):
                e = abs(g[c] - r[c])
                note("sum", e / b if b else e, e <= b, k, c, g[c], r[c])
            e = abs(g[o + 2] - r[o + 2])
            note("std", rel(g[o + 2], r[o + 2]), e <= 1e-9 + 1e-5 * abs(r[o + 2]), k, o + 2, g[o + 2], r[o + 2])
            for c in (o + 3, o + 4):
                note("equal", 0.0 if g[c] == r[c] else 1.0, g[c] == r[c], k, c, g[c], r[c])
            for c in range(o + N_INT, o + PER_CH):
                note("texture", rel(g[c], r[c]), abs(g[c] - r[c]) <= 1e-12 + 1e-9 * abs(r[c]), k, c, g[c], r[c])
    assert not bad, f"{len(bad)} mismatches:\n" + "\n".join(bad[:40])
    return worst
