"""CPU: per-instance co-occurrence matrices and Haralick features as texture.py states them in NumPy -- glcm_host against a per-pixel
Python loop, closed forms, the transpose identity, the pair count identity with measure_host's integers, additivity over row bands, the
level rule, range="object"; haralick() against an independent evaluation in fractions.Fraction / math.fsum; the route rule `fits`, the
keyword defaults, and the host-side argument validation of kg_label_glcm.  Every integer is compared exactly."""
import ctypes
import inspect
import math
import os
import re
from fractions import Fraction as F

import numpy as np
import pytest

from kg_instance_segmentation_amd import _lib, inference, instances, tiling
from kg_instance_segmentation_amd import measure as ms
from kg_instance_segmentation_amd import texture as tx
from kg_instance_segmentation_amd.labelmetrics import split_jobs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def blob_map(H, W, n, seed):
    """A seeded ragged map: ellipses and rectangles with ids 1 .. n painted over each other, some cut by the frame, some touching."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    lab = np.zeros((H, W), np.int32)
    for i in range(1, n + 1):
        cy, cx = rng.integers(0, H), rng.integers(0, W)
        ry, rx = rng.integers(1, max(H // 4, 2) + 1), rng.integers(1, max(W // 6, 2) + 1)
        sel = (np.abs(yy - cy) <= ry) & (np.abs(xx - cx) <= rx) if i % 2 else ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
        lab[sel & (rng.random((H, W)) < 0.93)] = i
    return lab


def seeded_image(shape, C, dtype, seed, smooth=False):
    top = np.iinfo(dtype).max
    rng = np.random.default_rng(seed)
    if smooth:                                                         # neighbouring pixels correlate: a texture, not noise
        yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
        base = np.sin(yy / 3.0)[..., None] + np.cos(xx[..., None] / 2.0 + np.arange(C))
        img = ((base + 2.0) / 4.0 * top * 0.9 + rng.random(tuple(shape) + (C,)) * top * 0.1).astype(dtype)
    else:
        img = rng.integers(0, top + 1, tuple(shape) + (C,)).astype(dtype)
    img.reshape(-1)[::7] = 0
    img.reshape(-1)[3::11] = top
    return img


def level(v, lo, span, L):
    return min(max(int(v) - lo, 0) * L // span, L - 1)


def brute(lab, jobs10, img, L):
    """rows of ten-column jobs on ONE map: a loop over every pixel of the box and every direction, in Python integers"""
    H, W = lab.shape
    out = np.zeros((len(jobs10), 4, L, L), np.int64)
    for a, (_, v, y1, x1, y2, x2, ch, d, lo, span) in enumerate(np.asarray(jobs10).tolist()):
        for y in range(max(y1, 0), min(y2, H)):
            for x in range(max(x1, 0), min(x2, W)):
                if lab[y, x] != v:
                    continue
                for k, (oy, ox) in enumerate(((0, 1), (1, 1), (1, 0), (1, -1))):
                    qy, qx = y + oy * d, x + ox * d
                    if 0 <= qy < H and 0 <= qx < W and lab[qy, qx] == v:
                        out[a, k, level(img[y, x, ch], lo, span, L), level(img[qy, qx, ch], lo, span, L)] += 1
    return out


def full_jobs(lab, ids, chans, ds, lo, span):
    H, W = lab.shape
    return np.array([[0, v, 0, 0, H, W, c, d, lo, span] for v in ids for c in chans for d in ds], np.int64)


@pytest.mark.parametrize("dtype,C,L,span", [(np.uint8, 3, 16, 256), (np.uint16, 2, 5, 65536)])
def test_host_against_a_per_pixel_loop(dtype, C, L, span):
    H, W, n = 40, 61, 14
    lab, img = blob_map(H, W, n, 3), seeded_image((H, W), C, dtype, 4)
    ds = (1, 2, 7)
    got = tx.glcm_host(lab, n, img, levels=L, distance=ds)
    assert got.counts.shape == (n, C, len(ds), 4, L, L) and got.distances == ds and got.channels == tuple(range(C))
    stats = tx.labelmetrics.label_stats_host(lab, n)
    jobs6 = ms.jobs_from_stats(stats)
    jobs10 = tx.texture_jobs(jobs6, range(C), ds, np.zeros((n, C)), np.full((n, C), span))
    want = brute(lab, jobs10, img, L).reshape(n, C, len(ds), 4, L, L)
    assert np.array_equal(got.counts, want) and want.any((1, 2, 3, 4, 5)).sum() >= n - 2
    assert np.array_equal(tx.glcm_rows_host(lab, jobs10, img, L), want.reshape(-1, 4, L, L))
    # an object's own box holds the whole object: the full-map box gives the same matrices
    whole = brute(lab, full_jobs(lab, range(1, n + 1), range(C), ds, 0, span), img, L).reshape(want.shape)
    assert np.array_equal(whole, want)
    # one channel, one distance, explicit jobs
    one = tx.glcm_host(lab, jobs6, img, levels=L, distance=2, channels=C - 1)
    assert one.channels == (C - 1,) and np.array_equal(one.counts[:, 0, 0], want[:, C - 1, 1])


def test_closed_forms():
    L = 16
    lab = np.zeros((9, 12), np.int32)
    lab[2:7, 3:11] = 1                                                  # a 5 x 8 rectangle
    img = np.full((9, 12, 1), 0x53, np.uint8)
    g = tx.glcm_host(lab, 1, img, levels=L).counts[0, 0, 0]
    want = np.zeros((4, L, L), np.int64)
    want[:, 5, 5] = (5 * 7, 4 * 7, 4 * 8, 4 * 7)                        # a constant object: every pair in one bin
    assert np.array_equal(g, want)
    d3 = tx.glcm_host(lab, 1, img, levels=L, distance=3).pairs()[0, 0, 0]
    assert d3.tolist() == [5 * 5, 2 * 5, 2 * 8, 2 * 5]
    yy, xx = np.mgrid[0:9, 0:12]
    chk = (((yy + xx) & 1) * 255).astype(np.uint8)[..., None]           # a two-level checkerboard
    g = tx.glcm_host(lab, 1, chk, levels=2).counts[0, 0, 0]
    # direction 0: 7 alternating pairs per row; 2 + 3 is odd, so level 1 starts rows 2, 4, 6 (four (1, 0), three (0, 1)) and level 0 rows 3, 5
    assert g[0].tolist() == [[0, 17], [18, 0]] and g[2].tolist() == [[0, 16], [16, 0]]
    assert g[1].tolist() == [[14, 0], [0, 14]] and g[3].tolist() == [[14, 0], [0, 14]]
    g2 = tx.glcm_host(lab, 1, chk, levels=2, distance=2).counts[0, 0, 0]
    assert (g2[:, 0, 1] == 0).all() and (g2[:, 1, 0] == 0).all() and g2.sum() == 5 * 6 + 3 * 6 + 3 * 8 + 3 * 6
    ramp = (xx * 16).astype(np.uint8)[..., None]                        # a horizontal ramp: level == x
    g = tx.glcm_host(lab, 1, ramp, levels=L).counts[0, 0, 0]
    want = np.zeros((4, L, L), np.int64)
    for x in range(3, 11):
        want[2, x, x] = 4
        if x + 1 < 11:
            want[0, x, x + 1], want[1, x, x + 1] = 5, 4
        if x - 1 >= 3:
            want[3, x, x - 1] = 4
    assert np.array_equal(g, want)
    one = np.zeros((5, 5), np.int32); one[2, 2] = 7
    c = tx.glcm_host(one, [[0, 7, 0, 0, 5, 5]], np.ones((5, 5, 2), np.uint8))
    assert not c.counts.any() and np.isnan(c.haralick()).all() and all(np.isnan(v).all() for k, v in c.props().items() if k != "pairs")
    thin = np.zeros((8, 8), np.int32); thin[1:7, 3:5] = 1               # two columns wide, six rows high
    p = tx.glcm_host(thin, 1, np.ones((8, 8, 1), np.uint8), distance=(1, 2, 5, 6)).pairs()[0, 0]
    assert p.tolist() == [[6, 5, 10, 5], [0, 0, 8, 0], [0, 0, 2, 0], [0, 0, 0, 0]]   # narrower than d: only direction 2 is left


def test_transpose_identity_and_pair_count():
    H, W, n, L = 33, 47, 9, 8
    lab, img = blob_map(H, W, n, 11), seeded_image((H, W), 1, np.uint8, 12)
    for d in (1, 3):
        g = tx.glcm_host(lab, n, img, levels=L, distance=d).counts[:, 0, 0]
        # the offset -o on the same map: rotate map and image by 180 degrees, where -o becomes +o
        r = tx.glcm_host(lab[::-1, ::-1].copy(), n, img[::-1, ::-1].copy(), levels=L, distance=d).counts[:, 0, 0]
        assert np.array_equal(r, np.swapaxes(g, -1, -2)) and g.any()
    g = tx.glcm_host(lab, n, img, levels=L)
    raw = ms.measure_host(lab, n)
    pairs = g.pairs()[:, 0, 0]
    # every pixel has 4 sides; a side is an edge or joins two pixels of the object (counted twice)
    assert np.array_equal(2 * (pairs[:, 0] + pairs[:, 2]), 4 * raw[:, 0] - raw[:, 6])
    assert np.array_equal(g.symmetric(), g.counts + np.swapaxes(g.counts, -1, -2))


def test_additivity_over_row_bands():
    H, W, L = 50, 40, 16
    lab = blob_map(H, W, 5, 21)
    lab[5:45, 4:36][lab[5:45, 4:36] == 0] = 6                           # one large ragged object around the others
    img = seeded_image((H, W), 2, np.uint8, 22)
    whole = tx.glcm_host(lab, [[0, 6, 0, 0, H, W]], img, levels=L, distance=(1, 4)).counts[0]
    for cut in (1, 7, 25, 44, 49):                                      # 25 cuts through the object; 1 and 49 leave a band without it
        parts = tx.glcm_host(lab, [[0, 6, 0, 0, cut, W], [0, 6, cut, 0, H, W]], img, levels=L, distance=(1, 4)).counts
        assert np.array_equal(parts.sum(0), whole) and whole.any()
    for cap in (64, 333, 1000):                                         # the band rule of the device route, on the host
        pieces, owner = split_jobs(np.array([[0, 6, 0, 0, H, W]]), cap)
        assert len(pieces) > 1
        assert np.array_equal(tx.glcm_host(lab, pieces, img, levels=L, distance=(1, 4)).counts.sum(0), whole)
    cols = tx.glcm_host(lab, [[0, 6, 0, 0, H, 13], [0, 6, 0, 13, H, W]], img, levels=L, distance=(1, 4)).counts
    assert np.array_equal(cols.sum(0), whole)                           # and over column bands: the partner comes from the map


@pytest.mark.parametrize("L", [2, 3, 16, 32])
def test_level_rule(L):
    v8 = np.arange(256)
    assert np.array_equal(tx.levels_of(v8, 0, 256, L), v8 * L // 256)
    if L == 16:
        assert np.array_equal(tx.levels_of(v8, 0, 256, 16), v8 >> 4)
    got = tx.levels_of(v8, 40, 100, L)                                  # below lo: level 0; at and above lo + span: L - 1
    assert (got[:41] == 0).all() and (got[140:] == L - 1).all() and got[139] == 99 * L // 100
    assert [int(x) for x in got] == [level(v, 40, 100, L) for v in v8]
    v16 = np.array([0, 1, 4095, 4096, 40000, 65535], np.uint16)
    assert tx.levels_of(v16, 0, 4096, L).tolist() == [0, 0, L - 1, L - 1, L - 1, L - 1]
    assert tx.levels_of(v16, 0, 65536, L).tolist() == [int(v) * L // 65536 for v in v16]
    assert tx.levels_of(v16, -2 ** 31, 2 ** 31 - 1, L).tolist() == [L - 1] * 6    # exact where int32 would overflow
    lab = np.ones((6, 7), np.int32)
    for dtype, rng_ in ((np.uint8, (40, 139)), (np.uint16, (1000, 50000))):
        img = seeded_image((6, 7), 2, dtype, 5 + L)
        g = tx.glcm_host(lab, 1, img, levels=L, range=rng_)
        lo, span = rng_[0], rng_[1] - rng_[0] + 1
        assert np.array_equal(g.counts[0, :, 0], brute(lab, full_jobs(lab, [1], (0, 1), (1,), lo, span), img, L))
        per = tx.glcm_host(lab, 1, img, levels=L, range=[rng_, (0, 9)])
        assert np.array_equal(per.counts[0, 0], g.counts[0, 0])
        assert np.array_equal(per.counts[0, 1, 0], brute(lab, full_jobs(lab, [1], (1,), (1,), 0, 10), img, L)[0])


def test_range_object():
    H, W, n, L = 30, 41, 6, 8
    lab, img = blob_map(H, W, n, 31), seeded_image((H, W), 2, np.uint16, 32, smooth=True)
    img[lab == 2] = img[lab == 2] // 7 + 900                            # an object that uses a small part of the range
    got = tx.glcm_host(lab, n, img, levels=L, range="object", channels=(1, 0))
    raw = ms.measure_host(lab, n, img)
    jobs6 = ms.jobs_from_stats(tx.labelmetrics.label_stats_host(lab, n))
    for i in range(n):
        for a, c in enumerate((1, 0)):
            lo, hi = int(raw[i, 12 + 4 * c]), int(raw[i, 13 + 4 * c])
            j10 = np.array([list(jobs6[i]) + [c, 1, lo, hi - lo + 1]])
            want = brute(lab, j10, img, L)[0]
            assert np.array_equal(got.counts[i, a, 0], want)
            if raw[i, 0] > 1 and hi > lo and want.sum():
                lev = tx.levels_of(img[lab == i + 1][:, c], lo, hi - lo + 1, L)
                assert lev.min() == 0 and lev.max() == L - 1            # the object's own range fills the levels
    with pytest.raises(tx.KGLibraryError):
        tx.glcm_host(lab, n, img, range="image")


# ---- Haralick ---------------------------------------------------------------------------------------------------------------------------

def haralick_exact(G):
    """f1 .. f13 of one integer matrix G by plain loops: Fractions for the rational features, math.fsum / math.log2 for the entropies"""
    L = len(G)
    S = [[int(G[i][j]) + int(G[j][i]) for j in range(L)] for i in range(L)]
    tot = sum(map(sum, S))
    if tot == 0:
        return [math.nan] * 13
    p = [[F(S[i][j], tot) for j in range(L)] for i in range(L)]
    px = [sum(p[i]) for i in range(L)]
    mu = sum(i * px[i] for i in range(L))
    var = sum((i - mu) ** 2 * px[i] for i in range(L))
    psum = [sum(p[i][k - i] for i in range(L) if 0 <= k - i < L) for k in range(2 * L - 1)]
    pdif = [sum(p[i][j] for i in range(L) for j in range(L) if abs(i - j) == k) for k in range(L)]

    def ent(ps):
        return -math.fsum(float(q) * math.log2(float(q)) for q in ps if q > 0)
    f = [0.0] * 13
    f[0] = float(sum(q * q for r in p for q in r))
    f[1] = float(sum((i - j) ** 2 * p[i][j] for i in range(L) for j in range(L)))
    f[2] = float(sum((i - mu) * (j - mu) * p[i][j] for i in range(L) for j in range(L)) / var) if var > 0 else 1.0
    f[3] = float(var)
    f[4] = float(sum(p[i][j] / (1 + (i - j) ** 2) for i in range(L) for j in range(L)))
    f6 = sum(k * psum[k] for k in range(2 * L - 1))
    f[5] = float(f6)
    f[6] = float(sum((k - f6) ** 2 * psum[k] for k in range(2 * L - 1)))
    f[7] = ent(psum)
    hxy = ent(q for r in p for q in r)
    f[8] = hxy
    md = sum(k * pdif[k] for k in range(L))
    f[9] = float(sum((k - md) ** 2 * pdif[k] for k in range(L)))
    f[10] = ent(pdif)
    hx = ent(px)
    hxy1 = -math.fsum(float(p[i][j]) * math.log2(float(px[i] * px[j])) for i in range(L) for j in range(L) if p[i][j] > 0)
    hxy2 = -math.fsum(float(px[i] * px[j]) * math.log2(float(px[i] * px[j])) for i in range(L) for j in range(L) if px[i] * px[j] > 0)
    f[11] = (hxy - hxy1) / hx if hx > 0 else 0.0
    f[12] = math.sqrt(max(0.0, 1.0 - math.exp(-2.0 * (hxy2 - hxy))))
    return f


RATIONAL = [0, 1, 2, 3, 4, 5, 6, 9]                                     # f1 .. f7, f10
LOGS = [7, 8, 10, 11, 12]
# rtol 1e-12 holds for every rational feature (largest relative deviation seen: 1.6e-13, f3) except where f3 is EXACTLY 0: a covariance
# that cancels to 0 in Fractions comes out as 3.6e-17 in float64, which no relative bound admits.  f3 lies in [-1, 1]; the largest
# absolute deviation of f3 seen over all cases below is 1.67e-16, and the bound is 4 x that, for f3 alone.
F3_ATOL = 7e-16


def test_haralick_against_an_independent_evaluation():
    H, W, n = 36, 44, 7
    lab = blob_map(H, W, n, 41)
    cases = []
    for L, dtype, smooth in ((16, np.uint8, True), (32, np.uint16, True), (3, np.uint8, False), (2, np.uint8, False), (8, np.uint8, False)):
        img = seeded_image((H, W), 1, dtype, 42 + L, smooth)
        cases.append(tx.glcm_host(lab, n, img, levels=L, distance=(1, 3)))
    const = np.zeros((H, W, 1), np.uint8) + 77                          # var == 0: f3 = 1, f12 = 0
    cases.append(tx.glcm_host(lab, n, const, levels=16))
    yy, xx = np.mgrid[0:H, 0:W]
    cases.append(tx.glcm_host(lab, n, (((yy + xx) & 1) * 255).astype(np.uint8)[..., None], levels=2))
    cases.append(tx.glcm_host(np.zeros((4, 4), np.int32), [[0, 5, 0, 0, 4, 4]], np.zeros((4, 4, 1), np.uint8)))   # no pairs: NaN
    worst_r, worst_l, seen = 0.0, 0.0, 0
    for c in cases:
        got = c.haralick()
        assert got.shape == c.counts.shape[:4] + (13,) and got.dtype == np.float64
        flat, G = got.reshape(-1, 13), c.counts.reshape(-1, c.levels, c.levels)
        for a in range(len(G)):
            want = np.array(haralick_exact(G[a]))
            if np.isnan(want).all():
                assert np.isnan(flat[a]).all() and G[a].sum() == 0
                continue
            seen += 1
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.abs(flat[a] - want) / np.abs(want)
            worst_r = max(worst_r, float(np.nanmax(np.where(want[RATIONAL] != 0, rel[RATIONAL], 0.0))))
            worst_l = max(worst_l, float(np.max(np.abs(flat[a] - want)[LOGS])))
            rest = [k for k in RATIONAL if k != 2]
            np.testing.assert_allclose(flat[a][rest], want[rest], rtol=1e-12, atol=0)
            np.testing.assert_allclose(flat[a][2], want[2], rtol=1e-12, atol=F3_ATOL)
            np.testing.assert_allclose(flat[a][LOGS], want[LOGS], rtol=1e-10, atol=1e-9)
    print(f"haralick: {seen} matrices, worst relative deviation (rational) {worst_r:.3e}, worst absolute (log) {worst_l:.3e}")
    assert seen > 100
    g = cases[5]                                                        # the constant image
    live = g.pairs() > 0
    h = g.haralick()
    assert (h[live][:, 2] == 1.0).all() and (h[live][:, 11] == 0.0).all() and (h[live][:, 0] == 1.0).all() and (h[live][:, 8] == 0.0).all()
    p = cases[0].props()
    assert set(p) == set(tx.FEATURES) | {"pairs"} and p["contrast"].shape == (n, 1, 2) and p["pairs"].shape == (n, 1, 2, 4)
    h0 = cases[0].haralick()
    assert np.array_equal(np.isnan(p["entropy"]), np.isnan(h0[..., 8]).any(-1))          # NaN where a direction has no pairs
    ok = ~np.isnan(p["entropy"])
    assert ok.any() and np.allclose(p["entropy"][ok], h0[..., 8].mean(-1)[ok], rtol=1e-15)


def test_comatrices_arguments():
    with pytest.raises(tx.KGLibraryError):
        tx.CoMatrices(np.zeros((2, 1, 1, 4, 3, 4)))
    with pytest.raises(tx.KGLibraryError):
        tx.CoMatrices(np.zeros((2, 1, 1, 3, 4, 4)))
    with pytest.raises(tx.KGLibraryError):
        tx.CoMatrices(np.zeros((2, 1, 2, 4, 4, 4)), distances=(1,))
    lab, img = np.ones((3, 3), np.int32), np.zeros((3, 3, 1), np.uint8)
    for kw in ({"levels": 1}, {"levels": 33}, {"levels": 4.0}, {"distance": 0}, {"distance": 33}, {"distance": ()}, {"distance": (1, 40)},
               {"channels": 1}, {"channels": -1}, {"channels": ()}, {"range": (5, 4)}, {"range": (1.0, 2.0)}, {"range": [(0, 1), (0, 1)]},
               {"range": "min"}):
        with pytest.raises(tx.KGLibraryError):
            tx.glcm_host(lab, 1, img, **kw)
    with pytest.raises(tx.KGLibraryError):
        tx.glcm_host(lab, 1, None)
    with pytest.raises(tx.KGLibraryError):
        tx.glcm_host(lab, 1, img.astype(np.float32))
    with pytest.raises(tx.KGLibraryError):
        tx.glcm(lab, 1, image=img)                                     # the device route refuses a host map
    # bad ten-column jobs: zeros, between good ones
    H = W = 3
    jobs = [[0, 1, 0, 0, H, W, 0, 1, 0, 256], [1, 1, 0, 0, H, W, 0, 1, 0, 256], [-1, 1, 0, 0, H, W, 0, 1, 0, 256], [0, 1, 0, 0, H, W, 1, 1, 0, 256],
            [0, 1, 0, 0, H, W, -1, 1, 0, 256], [0, 1, 0, 0, H, W, 0, 0, 0, 256], [0, 1, 0, 0, H, W, 0, 33, 0, 256], [0, 1, 0, 0, H, W, 0, 1, 0, 0],
            [0, 1, 0, 0, H, W, 0, 1, 0, -5], [0, 1, 2, 2, 1, 1, 0, 1, 0, 256], [0, 1, 0, 0, 0, W, 0, 1, 0, 256], [0, 1, -9, -9, 99, 99, 0, 1, 0, 256]]
    rows = tx.glcm_rows_host(lab, jobs, img, 4)
    assert rows[0].sum() == 6 + 4 + 6 + 4 and np.array_equal(rows[-1], rows[0]) and not rows[1:-1].any()


def test_texture_keyword_defaults_to_none():
    for fn in (inference.predict_instances, tiling.predict_tiled):
        assert inspect.signature(fn).parameters["texture"].default is None
    a = instances.Instances(None, np.zeros((0, 5), np.float32), None, None)
    b = tiling.TiledInstances(None, np.zeros((0, 5), np.float32), None, None, None, None)
    assert a.texture is None and b.texture is None and not hasattr(a, "__dict__")


def test_fits_on_both_sides_of_its_boundary():
    assert tx.fits(126, 126, 1) and tx.fits(127, 126, 1) and not tx.fits(128, 126, 1)           # 127 * 128, 128 * 128 = 16384, 129 * 128
    assert not tx.fits(127, 127, 1) and not tx.fits(126, 128, 1)        # 128 * 129, 127 * 130
    assert tx.fits(1, 8190, 1) and not tx.fits(1, 8191, 1)              # 2 * 8192 = 16384
    assert tx.fits(96, 64, 32) and not tx.fits(97, 64, 32) and not tx.fits(96, 65, 32)          # 128 * 128
    for h, w, d in ((126, 126, 1), (127, 126, 1), (1, 8190, 1), (1, 8191, 1), (96, 64, 32), (97, 64, 32), (300, 300, 2), (1, 1, 32)):
        assert tx.fits(h, w, d) == ((h + d) * (w + 2 * d) <= 16384)


# ---- the C entry ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from kg_instance_segmentation_amd import build
    build.build()
    return _lib.load()


def test_entry_is_declared_bound_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "kgnet_hip.h")).read()
    m = re.search(r"\bint\s+kg_label_glcm\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m and len(m.group(1).split(",")) == 12
    assert "kg_label_glcm" in _lib.SYMBOLS and hasattr(lib, "kg_label_glcm") and len(_lib._SIGS["kg_label_glcm"]) == 12


def check_entry_arguments(lib):
    """every host check of kg_label_glcm, on host memory: the entry may never get as far as a launch"""
    name = "kg_label_glcm"
    buf = (ctypes.c_longlong * 4096)()
    p = ctypes.addressof(buf)
    P, IMG, JOBS, OUT = (ctypes.c_void_p(p + k * 4096) for k in range(4))

    def call(labels=P, nimg=1, H=8, W=8, image=IMG, channels=3, elem=1, jobs=JOBS, m=3, levels=16, out=OUT):
        return lib.kg_label_glcm(labels, nimg, H, W, image, channels, elem, jobs, m, levels, out, None)

    def err(rc, text):
        msg = lib.kg_last_error().decode()
        assert rc != 0 and name in msg and text in msg, (rc, msg)

    err(call(labels=None), "null pointer")
    err(call(jobs=None), "null pointer")
    err(call(out=None), "null pointer")
    err(call(image=None), "null pointer")
    err(call(channels=0), "channels 0")
    err(call(channels=5), "channels 5")
    err(call(channels=-1), "channels -1")
    err(call(elem=3), "elem_bytes 3")
    err(call(elem=0), "elem_bytes 0")
    err(call(levels=1), "levels 1")
    err(call(levels=33), "levels 33")
    err(call(levels=0), "levels 0")
    err(call(levels=-16), "levels -16")
    err(call(H=32769), "32768")
    err(call(W=32769), "32768")
    err(call(nimg=0), "bad size")
    err(call(H=0), "bad size")
    err(call(W=-1), "bad size")
    err(call(m=-1), "bad size")
    err(call(nimg=3, H=32768, W=32768), "exceeds 2^31 - 1")
    err(call(out=ctypes.c_void_p(p + 3 * 4096 + 2)), "misaligned")
    err(call(labels=ctypes.c_void_p(p + 2)), "misaligned")
    err(call(jobs=ctypes.c_void_p(p + 2 * 4096 + 1)), "misaligned")
    err(call(image=ctypes.c_void_p(p + 4097), elem=2), "misaligned")
    assert call(m=0) == 0 and call(m=0, jobs=None, out=None) == 0
    assert call(m=0, image=ctypes.c_void_p(p + 4097), elem=1) == 0    # a byte image needs no alignment
    assert call(m=0, levels=2) == 0 and call(m=0, levels=32) == 0


def test_entry_refuses_bad_arguments_before_any_launch(lib):
    check_entry_arguments(lib)
