"""CPU: per-instance intensity quantiles and histograms as intensity.py states them in NumPy -- quantiles_host against a per-pixel Python
loop and against np.percentile, closed forms, Histograms against brute force in fractions.Fraction, the large-job route over host
histograms, the quantile arguments, and the host-side argument validation of kg_label_quantiles / kg_label_histograms.  Every integer is
compared exactly; linear() against numpy's default percentile at rtol 1e-9 (numpy forms its virtual index in float64)."""
import ctypes
import inspect
import math
import os
import re
from fractions import Fraction as F

import numpy as np
import pytest

from kg_instance_segmentation_amd import _lib, inference, instances, tiling
from kg_instance_segmentation_amd import intensity as iq
from kg_instance_segmentation_amd import measure as ms

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


def seeded_image(shape, C, dtype, seed):
    top = np.iinfo(dtype).max
    img = np.random.default_rng(seed).integers(0, top + 1, tuple(shape) + (C,)).astype(dtype)
    img.reshape(-1)[::7] = 0
    img.reshape(-1)[3::11] = top
    return img


def brute(lab, n, img, qs):
    """rows of the ids 1 .. n: a loop over every pixel collects, Python sorts, the rank rule in Python integers indexes"""
    H, W = lab.shape
    C = img.shape[2]
    vals = [[[] for _ in range(C)] for _ in range(n)]
    for y in range(H):
        for x in range(W):
            v = int(lab[y, x])
            if 1 <= v <= n:
                for c in range(C):
                    vals[v - 1][c].append(int(img[y, x, c]))
    out = np.zeros((n, C, 1 + 2 * len(qs)), np.int64)
    for i in range(n):
        for c in range(C):
            s = sorted(vals[i][c])
            if not s:
                continue
            out[i, c, 0] = len(s)
            for k, q in enumerate(qs):
                t = q.numerator * (len(s) - 1)
                lo = t // q.denominator
                out[i, c, 1 + 2 * k], out[i, c, 2 + 2 * k] = s[lo], s[lo + (t % q.denominator != 0)]
    return out


@pytest.mark.parametrize("dtype,C", [(np.uint8, 3), (np.uint16, 2)])
def test_host_against_a_per_pixel_loop(dtype, C):
    H, W, n = 40, 61, 14
    lab = blob_map(H, W, n, 3)
    img = seeded_image((H, W), C, dtype, 4)
    qs = iq.as_fractions([F(0), F(1, 20), F(1, 3), F(1, 2), F(3, 4), F(999, 1000), F(1), F(1, 2)])
    got = iq.quantiles_host(lab, n, img, qs)
    assert got.dtype == np.int64 and got.shape == (n, C, 17) and np.array_equal(got, brute(lab, n, img, qs))
    assert (got[:, 0, 0] > 0).sum() >= 8 and (got[:, :, 1::2] != got[:, :, 2::2]).any()
    assert np.array_equal(got[:, :, 0], ms.measure_host(lab, n, img)[:, :1].repeat(C, 1))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_host_against_numpy_lower_and_higher(dtype):
    H, W, n = 50, 70, 12
    lab = blob_map(H, W, n, 8)
    img = seeded_image((H, W), 2, dtype, 9)
    qs = [F(0), F(1, 4), F(1, 2), F(3, 4), F(1)]                      # exact in binary: numpy's float index is the rational one
    got = iq.Quantiles(iq.quantiles_host(lab, n, img, qs), qs)
    seen = 0
    for i in range(n):
        for c in range(2):
            v = img[..., c][lab == i + 1]
            if len(v) == 0:
                assert not got.raw[i, c].any() and np.isnan(got.lower()[i, c]).all() and np.isnan(got.linear()[i, c]).all()
                continue
            seen += 1
            p = [float(q) * 100 for q in qs]
            assert np.array_equal(got.lower()[i, c], np.percentile(v, p, method="lower"))
            assert np.array_equal(got.higher()[i, c], np.percentile(v, p, method="higher"))
    assert seen >= 12


def test_linear_against_numpy_default_percentile():
    """n = 1 .. 69, 255, 256, 257, 1000 and nine quantiles: 657 cases, none beyond rtol 1e-9 of numpy's default method."""
    qs = [F(0), F(1, 100), F(1, 4), F(1, 2), F(3, 4), F(99, 100), F(1), F(1, 3), F(999, 1000)]
    rng = np.random.default_rng(21)
    cases = 0
    for n in list(range(1, 70)) + [255, 256, 257, 1000]:
        lab = np.ones((1, n), np.int32)
        img = rng.integers(0, 65536, (1, n, 1)).astype(np.uint16)
        for part in (qs[:8], qs[8:]):                                 # at most 8 per call
            got = iq.Quantiles(iq.quantiles_host(lab, 1, img, part), part)
            want = np.percentile(img[0, :, 0].astype(np.float64), [float(q) * 100 for q in part])
            np.testing.assert_allclose(got.linear()[0, 0], want, rtol=1e-9, atol=0)
            cases += len(part)
    assert cases == 657


def test_closed_forms():
    lab = np.zeros((20, 40), np.int32)
    lab[2:10, 3:35] = 1                                               # 256 pixels: a ramp 0 .. 255
    lab[12:15, 0:7] = 2                                               # 21 pixels: constant
    lab[16:18, 10:15] = 3                                             # 10 pixels: 3 x 10, 7 x 200
    img = np.zeros((20, 40, 1), np.uint8)
    img[2:10, 3:35, 0] = np.random.default_rng(0).permutation(256).reshape(8, 32)
    img[12:15, 0:7] = 77
    img[16:18, 10:15] = 200
    img[16, 10:13] = 10
    q = iq.Quantiles(iq.quantiles_host(lab, 3, img), None)            # the default 1/20, 1/4, 1/2, 3/4, 19/20
    assert q.q == iq.DEFAULT_Q and q.counts().tolist() == [256, 21, 10]
    # ramp: t = num * 255 / den: 12.75, 63.75, 127.5, 191.25, 242.25
    assert q.raw[0, 0].tolist() == [256, 12, 13, 63, 64, 127, 128, 191, 192, 242, 243]
    np.testing.assert_allclose(q.linear()[0, 0], [12.75, 63.75, 127.5, 191.25, 242.25], rtol=1e-12)
    assert q.median()[0, 0] == 127.5 and q.iqr()[0, 0] == 127.5
    assert q.raw[1, 0].tolist() == [21] + [77] * 10 and q.iqr()[1, 0] == 0
    # two values, sorted 10 10 10 200 x 7: ranks 0.45, 2.25, 4.5, 6.75, 8.55
    assert q.raw[2, 0].tolist() == [10, 10, 10, 10, 200, 200, 200, 200, 200, 200, 200]
    np.testing.assert_allclose(q.linear()[2, 0], [10, 10 + 190 * 0.25, 200, 200, 200], rtol=1e-12)
    p = q.props()
    assert set(p) == {"count", "lower", "higher", "linear", "median", "iqr"} and p["linear"].shape == (3, 1, 5)
    one = iq.Quantiles(iq.quantiles_host(lab, 3, img, [F(1, 3)]), [F(1, 3)])
    assert "median" not in one.props() and "iqr" not in one.props()
    with pytest.raises(iq.KGLibraryError):
        one.median()


def host_histograms(lab, n, img, shift=0):
    """Histograms of the ids 1 .. n through histograms_host, every channel"""
    C = img.shape[-1]
    jobs = ms.jobs_from_stats(ms.labelmetrics.label_stats_host(lab, n))
    j9 = iq._hist_jobs(np.repeat(jobs, C, 0), np.tile(np.arange(C), n), shift, -1)
    return iq.Histograms(iq.histograms_host(lab, j9, img).reshape(n, C, 256), shift)


def test_histograms_against_measure_and_quantiles():
    H, W, n = 45, 66, 13
    lab = blob_map(H, W, n - 1, 5)                                    # id 13 is absent: an empty histogram
    img = seeded_image((H, W), 3, np.uint8, 6)
    h = host_histograms(lab, n, img)
    m = ms.measure_host(lab, n, img)
    assert np.array_equal(h.totals(), m[:, :1].repeat(3, 1)) and (h.totals() > 0).any() and (h.totals() == 0).any()
    occupied = h.counts > 0
    lo, hi = occupied.argmax(-1), 255 - occupied[..., ::-1].argmax(-1)
    live = h.totals() > 0
    assert np.array_equal(lo[live], m[:, 12::4][live]) and np.array_equal(hi[live], m[:, 13::4][live])
    qs = [F(0), F(1, 20), F(1, 3), F(1, 2), F(999, 1000), F(1)]
    want = iq.quantiles_host(lab, n, img, qs)
    for k, q in enumerate(qs):
        assert np.array_equal(h.quantile(q.numerator, q.denominator), want[:, :, 1 + 2 * k:3 + 2 * k])
    # 16-bit: shift 8 is the high byte, shift 4 the exact histogram of 12-bit data; a prefix selects the low bytes under one high byte
    wide = (seeded_image((H, W), 1, np.uint16, 7) >> 4).astype(np.uint16)
    h12 = host_histograms(lab, n, wide, 4)
    assert np.array_equal(h12.totals()[:, 0], m[:, 0])
    v = wide[..., 0][lab == 1]
    assert np.array_equal(h12.counts[0, 0], np.bincount(v >> 4, minlength=256))
    job = [[0, 1, 0, 0, H, W, 0, 0, 3], [0, 1, 0, 0, H, W, 0, 0, -1], [0, 1, 0, 0, H, W, 1, 0, -1], [0, 1, 0, 0, H, W, 0, 9, -1],
           [0, 1, 0, 0, H, W, -1, 0, -1], [1, 1, 0, 0, H, W, 0, 0, -1], [0, 1, 5, 5, 5, 9, 0, 0, -1], [0, 99, 0, 0, H, W, 0, 0, -1]]
    rows = iq.histograms_host(lab, job, wide)
    assert np.array_equal(rows[0], np.bincount(v[(v >> 8) == 3] & 255, minlength=256)) and rows[0].sum() > 0
    assert rows[1, 255] == np.count_nonzero(v >= 255) and rows[1].sum() == len(v) and not rows[2:].any()


def otsu_brute(counts):
    """all 255 thresholds in Fractions: the smallest t with the largest between-class variance"""
    N = int(counts.sum())
    best, arg = F(0), 0
    for t in range(255):
        n0 = int(counts[:t + 1].sum())
        n1 = N - n0
        if n0 == 0 or n1 == 0:
            continue
        mu0 = F(int((counts[:t + 1] * np.arange(t + 1)).sum()), n0)
        mu1 = F(int((counts[t + 1:] * np.arange(t + 1, 256)).sum()), n1)
        var = F(n0, N) * F(n1, N) * (mu0 - mu1) ** 2
        if var > best:
            best, arg = var, t
    return arg


def test_otsu_entropy_mode():
    rng = np.random.default_rng(12)
    c = np.zeros((7, 1, 256), np.int64)
    c[0, 0] = rng.integers(0, 50, 256)
    c[1, 0, 20:60] = rng.integers(1, 400, 40); c[1, 0, 180:230] = rng.integers(1, 300, 50)      # bimodal
    c[2, 0, [10, 200]] = 5                                            # two equal spikes: every t in 10 .. 199 ties, the smallest wins
    c[3, 0, 99] = 1000                                                # one bin
    c[5, 0, :4] = [2 ** 29, 2 ** 29, 2 ** 29, 2 ** 29]                # counts at the size limit: the squares pass 2^64
    c[6, 0, [0, 255]] = [3, 1]
    h = iq.Histograms(c)
    assert h.otsu()[:, 0].tolist() == [otsu_brute(c[i, 0]) for i in range(7)]
    assert h.otsu()[2, 0] == 10 and h.otsu()[3, 0] == 0 and h.otsu()[4, 0] == 0 and h.otsu()[5, 0] == 1 and 20 <= h.otsu()[1, 0] < 230
    assert h.mode()[:, 0].tolist()[2:] == [10, 99, 0, 0, 0] and h.mode()[0, 0] == int(c[0, 0].argmax())
    e = h.entropy()[:, 0]
    assert e[2] == 1.0 and e[3] == 0.0 and math.isnan(e[4]) and e[5] == 2.0
    assert e[6] == pytest.approx(2 - 0.75 * math.log2(3), rel=1e-12)
    flat = iq.Histograms(np.ones((1, 1, 256), np.int64))
    assert flat.entropy()[0, 0] == 8.0 and flat.mode()[0, 0] == 0 and flat.otsu()[0, 0] == 127
    with pytest.raises(iq.KGLibraryError):
        iq.Histograms(np.zeros((2, 255), np.int64))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("cap", [1, 37, 500, 10 ** 6])
def test_large_job_route_over_host_histograms(dtype, cap):
    H, W, n = 30, 53, 9
    lab = blob_map(H, W, n, 15)
    img = seeded_image((H, W), 2, dtype, 16)
    if dtype == np.uint16:
        img[lab == 2] = (img[lab == 2] & 0x00ff) | 0x1200             # every high byte equal
        img[lab == 3] &= 0x0fff                                       # 12-bit data
    qs = [F(0), F(1, 20), F(1, 3), F(1, 2), F(1, 2), F(3, 4), F(999, 1000), F(1)]
    jobs = np.concatenate([ms.jobs_from_stats(ms.labelmetrics.label_stats_host(lab, n)),
                           [[0, 4, 10, 20, 5, 30], [3, 1, 0, 0, H, W], [0, 77, 0, 0, H, W]]]).astype(np.int64)
    calls = []

    def rows(j9):
        calls.append(len(j9))
        return iq.histograms_host(lab, j9, img)
    got = iq.quantiles_from_histograms(jobs, 2, dtype == np.uint16, qs, cap, rows)
    assert np.array_equal(got, iq.quantiles_host(lab, jobs, img, qs)) and got[:n, 0, 0].any() and not got[n:].any()
    assert len(calls) == (2 if dtype == np.uint16 else 1)            # the number of launches does not depend on the data
    if cap == 1:                                                      # one piece per pixel and channel
        assert calls[0] == 2 * int(np.maximum((jobs[:, 4] - jobs[:, 2]) * (jobs[:, 5] - jobs[:, 3]), 1).sum())


def test_quantile_arguments():
    assert iq.as_fractions(None) == (F(1, 20), F(1, 4), F(1, 2), F(3, 4), F(19, 20))
    assert iq.as_fractions([0.5, 0.25, (1, 3), F(2, 7), 1, 0, 1 / 3]) == (F(1, 2), F(1, 4), F(1, 3), F(2, 7), F(1), F(0), F(1, 3))
    assert iq.as_fractions([0.1])[0] == F(1, 10) and iq.as_fractions(0.95) == (F(19, 20),)
    assert iq.as_fractions([math.pi / 4])[0].denominator <= 10 ** 6
    assert iq.q_table([(2, 4), 0.999]).tolist() == [[1, 2], [999, 1000]] and iq.q_table(None).dtype == np.int32
    for bad in ([0.1] * 9, [], [1.5], [-0.25], [(3, 2)], [(1, 0)], [F(1, 10 ** 6 + 1)], ["x"], [float("nan")]):
        with pytest.raises(iq.KGLibraryError):
            iq.as_fractions(bad)
    k_lo, k_hi, rem = iq.ranks([1, 2, 10, 0], [F(1, 2), F(1, 3)])
    assert k_lo.tolist() == [[0, 0], [0, 0], [4, 3], [0, 0]] and k_hi.tolist() == [[0, 0], [1, 1], [5, 3], [0, 0]]
    assert rem.tolist() == [[0, 0], [1, 1], [1, 0], [0, 0]]
    lab, img = np.ones((3, 3), np.int32), np.zeros((3, 3, 1), np.uint8)
    with pytest.raises(iq.KGLibraryError):
        iq.quantiles_host(lab, 1, None)
    with pytest.raises(iq.KGLibraryError):
        iq.quantiles_host(lab, 1, img.astype(np.float32))
    with pytest.raises(iq.KGLibraryError):
        iq.quantiles_host(lab, 1, img, [0.1] * 9)
    with pytest.raises(iq.KGLibraryError):
        iq.quantiles(lab, 1, image=img)                               # the device route refuses a host map


def test_quantiles_keyword_defaults_to_none():
    for fn in (inference.predict_instances, tiling.predict_tiled):
        assert inspect.signature(fn).parameters["quantiles"].default is None
    a = instances.Instances(None, np.zeros((0, 5), np.float32), None, None)
    b = tiling.TiledInstances(None, np.zeros((0, 5), np.float32), None, None, None, None)
    assert a.quantiles is None and b.quantiles is None and not hasattr(a, "__dict__")


# ---- the C entries ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from kg_instance_segmentation_amd import build
    build.build()
    return _lib.load()


def test_entries_are_declared_bound_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "kgnet_hip.h")).read()
    for name, nargs in (("kg_label_quantiles", 13), ("kg_label_histograms", 11)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m and len(m.group(1).split(",")) == nargs
        assert name in _lib.SYMBOLS and hasattr(lib, name) and len(_lib._SIGS[name]) == nargs


@pytest.mark.parametrize("name", ["kg_label_quantiles", "kg_label_histograms"])
def test_entries_refuse_bad_arguments_before_any_launch(lib, name):
    buf = (ctypes.c_longlong * 4096)()                      # host memory: the entry may never get as far as a launch
    p = ctypes.addressof(buf)
    P, IMG, JOBS, OUT, QT = (ctypes.c_void_p(p + k * 4096) for k in range(5))
    quant = name == "kg_label_quantiles"

    def call(labels=P, nimg=1, H=8, W=8, image=IMG, channels=3, elem=1, jobs=JOBS, m=3, qtab=QT, Q=5, out=OUT):
        extra = (qtab, Q) if quant else ()
        return getattr(lib, name)(labels, nimg, H, W, image, channels, elem, jobs, m, *extra, out, None)

    def err(rc, text):
        msg = lib.kg_last_error().decode()
        assert rc != 0 and name in msg and text in msg, (rc, msg)

    err(call(labels=None), "null pointer")
    err(call(jobs=None), "null pointer")
    err(call(out=None), "null pointer")
    err(call(image=None), "null pointer")                   # an image that is NULL with C > 0
    err(call(channels=0), "channels 0")
    err(call(channels=5), "channels 5")
    err(call(channels=-1), "channels -1")
    err(call(elem=3), "elem_bytes 3")
    err(call(elem=0), "elem_bytes 0")
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
    if quant:
        err(call(Q=0), "Q 0")
        err(call(Q=9), "Q 9")
        err(call(Q=-1), "Q -1")
        err(call(qtab=None), "null pointer")
        err(call(qtab=ctypes.c_void_p(p + 4 * 4096 + 2)), "misaligned")
    assert call(m=0) == 0 and call(m=0, jobs=None, out=None) == 0
    assert call(m=0, image=ctypes.c_void_p(p + 4097), elem=1) == 0    # a byte image needs no alignment
