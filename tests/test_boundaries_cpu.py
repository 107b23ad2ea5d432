"""CPU: the host statements of the boundary distances (boundaries.border_d2_host, pair_jobs, merge_pieces, PairDistances) against per-pixel
plain-Python loops, scipy's erosion and distance transform, closed forms, and LabelEvaluator's boundary= option on host maps; the
host-side argument checks of kg_label_border_counts / kg_label_border_d2 (nothing is launched).  Every distance is an exact integer."""
import ctypes
import math

import numpy as np
import pytest

from kg_instance_segmentation_amd import _lib
from kg_instance_segmentation_amd import boundaries as bd
from kg_instance_segmentation_amd import labelmetrics as lm

from boundaries_cases import (MODES, all_pair_jobs, blob_maps, boxes_of, disc_in_ring, ellipse_pair, job, plain_border, plain_job, plain_metrics,
                              stripes, thick_row, unsplit_d2, whole)

E = _lib.KGLibraryError


@pytest.fixture(scope="module")
def blobs():
    a, b = blob_maps(37, 53, 9, 5)
    return a, b, 9


def test_host_statement_equals_the_plain_loops_in_all_modes(blobs):
    a, b, n = blobs
    jobs = np.concatenate([all_pair_jobs(a, b, n), all_pair_jobs(a, b, n, grow=2)[:6],
                           [job(0, whole(a), 3, whole(a)), job(2, (5, 5, 30, 40), 2, (0, 0, 20, 53), 1),      # boxes that cut their object
                            job(1, whole(a), 1, (3, 3, 3, 9)), job(1, (9, 2, 4, 8), 1, whole(a)),              # empty, inverted
                            job(1, whole(a), 1, whole(a), img=1), job(1, whole(a), 1, whole(a), img=-1)]])
    for mode in MODES:
        counts, vals = bd.border_d2_host(a, b, jobs, mode)
        assert counts.dtype == np.int32 and counts.shape == (len(jobs), 3) and all(v.dtype == np.int32 for v in vals)
        for k, row in enumerate(jobs):
            c, d = plain_job(a, b, row, mode)
            assert counts[k].tolist() == c and vals[k].tolist() == d, (mode, k)
        assert counts[:, 0].sum() > 200 and (counts[-4:] == 0).all()
    for v in (0, 1, 4):
        assert np.argwhere(bd.border_host(a, v)).tolist() == [list(p) for p in plain_border(a, v)]


def test_border_and_distances_equal_scipy(blobs):
    ndi = pytest.importorskip("scipy.ndimage")
    a, b, n = blobs
    big_a, big_b = blob_maps(300, 420, 30, 11)
    for A, B, k in ((a, b, n), (big_a, big_b, 30)):
        for v in range(0, k + 1):
            mask = A == v
            assert np.array_equal(bd.border_host(A, v), mask & ~ndi.binary_erosion(mask))
        sa, sb = boxes_of(A, k), boxes_of(B, k)
        pairs = [(i, i) for i in range(1, k + 1) if sa[i - 1, 0] and sb[i - 1, 0]]
        got = bd.pair_distances_host(A, B, pairs, sa, sb)
        assert len(got) == len(pairs) > k // 2
        for r, (i, _) in enumerate(pairs):
            ea, eb = bd.border_host(A, i), bd.border_host(B, i)
            assert np.array_equal(got.of(r, 0), np.rint(ndi.distance_transform_edt(~eb)[ea] ** 2).astype(np.int64))
            assert np.array_equal(got.of(r, 1), np.rint(ndi.distance_transform_edt(~ea)[eb] ** 2).astype(np.int64))


def _one(a, b, mode=0, direction=0):
    return bd.border_d2_host(a, b, [job(1, whole(a), 1, whole(b), direction)], mode)[1][0]


def test_closed_forms():
    a, b = blob_maps(40, 40, 4, 3)
    for i in (1, 2, 3, 4):
        for mode in MODES:                                             # two equal objects
            d2 = bd.border_d2_host(a, a, [job(i, whole(a), i, whole(a))], mode)[1][0]
            if mode == 1:                                              # all sources to the border: zero on the border only
                assert np.array_equal(d2 == 0, bd.border_host(a, i)[a == i]) and len(d2)
            else:
                assert not d2.any() and len(d2)
    rect = np.zeros((40, 50), np.int32)
    rect[5:20, 7:30] = 1
    moved = np.roll(rect, (3, 4), (0, 1))
    d = bd.pair_distances_host(rect, moved, [(1, 1)], n_a=1, n_b=1)
    assert d.hausdorff().tolist() == [5.0] and d.directed_hausdorff().tolist() == [[5.0, 5.0]]
    blob = (a == 1).astype(np.int32)
    assert blob.any() and not blob[:, -4:].any() and not blob[-3:].any()
    assert bd.pair_distances_host(blob, np.roll(blob, (3, 4), (0, 1)), [(1, 1)], n_a=1, n_b=1).hausdorff()[0] <= 5.0
    r, R = 4, 11
    sq = np.zeros((2, 31, 31), np.int32)
    sq[0, 15 - r:16 + r, 15 - r:16 + r] = 1
    sq[1, 15 - R:16 + R, 15 - R:16 + R] = 1
    d = bd.pair_distances_host(sq[0], sq[1], [(1, 1)], n_a=1, n_b=1)
    # from the inner outline every pixel is R - r from the outer one or closer at a corner's flank: the directed distance is R - r exactly;
    # the other way the outer corner's nearest inner pixel is the inner corner, (R - r) * sqrt(2), which is the symmetric maximum
    assert d.directed_hausdorff()[0].tolist() == [R - r, math.sqrt(2 * (R - r) ** 2)] and d.of(0, 0).max() == (R - r) ** 2
    assert d.hausdorff()[0] == math.sqrt(2 * (R - r) ** 2) and d.of(0, 1).min() == (R - r) ** 2
    disc, ring = disc_in_ring()
    inner = _one(disc, ring, 0).max()
    centre = _one(disc, ring, 3).max()                                 # region targets, all sources: the disc's centre is the farthest
    assert centre == 12 ** 2 and centre > inner and _one(disc, ring, 1).max() == centre
    filled = (ring | (np.hypot(*(np.mgrid[0:41, 0:41] - 20)) <= 12)).astype(np.int32)
    assert not _one(disc, filled, 3).any() and _one(disc, filled, 1).max() > 12 ** 2                        # inside the region: 0
    none = bd.border_d2_host(disc, ring, [job(1, whole(disc), 7, whole(ring))], 0)
    assert none[0].tolist() == [[int(bd.border_host(disc, 1).sum()), 0, 0]] and (none[1][0] == -1).all()
    empty = np.zeros_like(disc)
    d = bd.pair_distances_host(disc, empty, [(1, 1)], n_a=1, n_b=1)
    assert (d.of(0, 0) == -1).all() and len(d.of(0, 0)) and len(d.of(0, 1)) == 0
    assert d.hausdorff()[0] == math.inf and d.hd95()[0] == math.inf and d.assd()[0] == math.inf and d.nsd(1e9)[0] == 0.0


def test_size_rule_and_arguments():
    lab = thick_row(5, 8193, 2, 1)
    ok, over = job(1, whole(lab), 1, (2, 0, 3, 8192)), job(1, whole(lab), 1, (2, 0, 3, 8193))
    counts, vals = bd.border_d2_host(lab, lab, [ok, over])
    assert counts.tolist() == [[8193, 8192, 0], [0, 0, 1]] and vals[0][-1] == 1 and not vals[0][:-1].any() and len(vals[1]) == 0
    assert bd.border_d2_store_host(lab, lab, [job(1, (2, 0, 3, 4), 1, (2, 0, 3, 2), first=-2)], 0, 3, fill=-7).tolist() == [1, 4, -7]
    for bad in (lambda: bd.border_d2_host(lab, lab[:, :-1], [ok]), lambda: bd.border_d2_host(lab, lab, [ok[:-1]]),
                lambda: bd.border_d2_host(lab, lab, [ok], 4), lambda: bd.border_d2_host(lab.astype(np.float32), lab, [ok]),
                lambda: bd.pair_distances_host(lab, lab, [(1, 1)]), lambda: bd.pair_distances_host(lab, lab, [(2, 1)], n_a=1, n_b=1),
                lambda: bd.pair_distances_host(lab, lab, [(1, 1)], n_a=1, n_b=1, sources="edge"),
                lambda: bd.pair_jobs([(1, 1)], [[1, 0, 0, 1, 1]], [[1, 0, 0, 1, 1]], 4, 4, max_job_pixels=0)):
        with pytest.raises(E):
            bad()


@pytest.fixture(scope="module")
def split_pairs():
    """{size: (a, b, stats_a, stats_b, {(mode, direction): the unsplit distances})}: a 300 x 300 pair in border mode, and a 110 x 110 pair in
    border mode and with all sources against the region -- the plain minimum over all target pixels, computed once"""
    out = {}
    for size, modes in ((300, (0,)), (110, (0, 3))):
        a, b = ellipse_pair(size)
        out[size] = (a, b, boxes_of(a, 1), boxes_of(b, 1), {(m, d): unsplit_d2(a, b, m, d) for m in modes for d in (0, 1)})
    return out


@pytest.mark.parametrize("cap", [4096, 65536])
def test_pair_jobs_and_merge_equal_the_unsplit_statement(split_pairs, cap):
    """A 300 x 300 pair: 24 source bands of 13 rows at 4096, two bands at 65536; its target boxes always split (12 rectangles of 27 rows).
    A 110 x 110 pair: its target boxes split in two, its sources in four bands at 4096 only."""
    for size, bands, rects in ((300, 24 if cap == 4096 else 2, 12), (110, 4 if cap == 4096 else 1, 2)):
        a, b, sa, sb, want = split_pairs[size]
        assert sa[0, 3] - sa[0, 1] >= size and sa[0, 4] - sa[0, 2] >= size
        pj = bd.pair_jobs([(1, 1)], sa, sb, *a.shape, max_job_pixels=cap)
        boxes = pj.jobs[:, 8:12].astype(np.int64)
        assert ((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]) <= 8192).all()
        assert pj.order.max() == bands - 1 and len(pj) == bands * rects * 2, (size, pj.order.max(), len(pj))
        for mode, d in want:
            got = bd.pair_distances_host(a, b, [(1, 1)], sa, sb, sources="all" if mode & 1 else "border", targets="region" if mode & 2 else "border",
                                         max_job_pixels=cap)
            assert np.array_equal(got.of(0, d), want[mode, d]), (size, mode, d)


def test_target_box_of_91_by_91_splits():
    a = np.zeros((100, 100), np.int32)
    a[3:94, 5:96] = stripes(91, 91)
    b = np.zeros_like(a)
    b[40:43, 10:90] = 1
    sa, sb = boxes_of(a, 1), boxes_of(b, 1)
    pj = bd.pair_jobs([(1, 1)], sb, sa, 100, 100)                      # b's object is the source of direction 0: the 91 x 91 box is the target
    assert pj.direction.tolist() == [0, 0, 1] and pj.jobs[:2, 8:12].tolist() == [[3, 5, 93, 96], [93, 5, 94, 96]]
    counts, vals = bd.border_d2_host(b, a, pj.jobs)
    assert counts[:, 2].tolist() == [0, 0, 0] and counts[0, 1] + counts[1, 1] == (a == 1).sum() == 91 * 46
    whole_box = bd.border_d2_host(b, a, [job(1, sb[0, 1:], 1, sa[0, 1:])])[0]
    assert whole_box.tolist() == [[0, 0, 1]]                           # the unsplit job breaks the size rule
    got = bd.merge_pieces(pj, counts, np.concatenate(vals))
    yt, xt = np.nonzero(a == 1)
    ys, xs = np.nonzero(bd.border_host(b, 1))
    assert np.array_equal(got.of(0, 0), [((y - yt) ** 2 + (x - xt) ** 2).min() for y, x in zip(ys, xs)])
    with pytest.raises(E):
        bd.merge_pieces(pj, counts[:2], np.concatenate(vals))


def test_metrics_equal_plain_restatements(blobs):
    a, b, n = blobs
    sa, sb = boxes_of(a, n), boxes_of(b, n)
    pairs = [(i, j) for i in range(1, n + 1) for j in (i, i % n + 1)]
    d = bd.pair_distances_host(a, b, pairs, sa, sb)
    empty_b = [k for k, (_, j) in enumerate(pairs) if sb[j - 1, 0] == 0]
    hd, hd95, assd = d.hausdorff(), d.hd95(), d.assd()
    for tol in (0, 1, 1.5, 2, 3.7):
        nsd = d.nsd(tol)
        for k in range(len(pairs)):
            want = plain_metrics(d.of(k, 0).tolist(), d.of(k, 1).tolist(), tol)
            got = (hd[k], hd95[k], assd[k], nsd[k])
            assert all(g == w or (math.isnan(g) and math.isnan(w)) for g, w in zip(got, want)), (k, tol, got, want)
    assert np.isfinite(hd).sum() >= n - 2 and all(hd[k] == math.inf for k in empty_b)
    assert np.array_equal(d.directed_hausdorff().max(1), hd) and d.counts().shape == (len(pairs), 2)
    # nothing depends on the order of a list
    rng = np.random.default_rng(0)
    shuffled = d.d2.copy()
    for r in range(len(d.indptr) - 1):
        rng.shuffle(shuffled[d.indptr[r]:d.indptr[r + 1]])
    s = bd.PairDistances(d.indptr, shuffled)
    assert np.array_equal(s.hd95(), hd95, equal_nan=True) and np.array_equal(s.assd(), assd, equal_nan=True)
    with pytest.raises(E):
        bd.PairDistances([0, 1], [1])


TODAY = ["thresholds", "seg_ap", "seg_iou", "kaggle", "pq", "sq", "dq", "aji", "dice", "images"]


def test_label_evaluator_boundary_option(blobs):
    a, b, n = blobs
    plain = lm.LabelEvaluator(boundary=None)
    plain.add((a, n), (b, n))
    assert list(plain.summary()) == TODAY and list(lm.LabelEvaluator().summary()) == TODAY
    ev = lm.LabelEvaluator(boundary=True)
    c = ev.add((a, n), (b, n))
    s = ev.summary()
    assert list(s) == TODAY + ["hd", "hd95", "assd", "nsd", "boundary_pairs"]
    tp = lm.panoptic(c)["tp"]
    assert s["boundary_pairs"] == tp > 3 and all(s[k] == plain.summary()[k] or k in ("thresholds",) for k in TODAY[3:])
    d = bd.pair_distances_host(a, b, c.pairs[c.iou() > 0.5], n_a=n, n_b=n)
    assert s["hd"] == math.fsum(d.hausdorff()) / tp and s["nsd"] == math.fsum(d.nsd(2)) / tp and 0 < s["nsd"] <= 1
    assert s["assd"] == math.fsum(d.assd()) / tp and s["hd95"] <= s["hd"] and s["assd"] <= s["hd"]
    opt = lm.LabelEvaluator(boundary=dict(tolerance=1, sources="all", targets="region"))
    opt.add((a, n), (b, n))
    d = bd.pair_distances_host(a, b, c.pairs[c.iou() > 0.5], n_a=n, n_b=n, sources="all", targets="region")
    assert opt.summary()["nsd"] == math.fsum(d.nsd(1)) / tp and opt.summary()["hd"] <= s["hd"]
    none = lm.LabelEvaluator(boundary=True).summary()
    assert none["hd"] is None and none["boundary_pairs"] == 0
    for bad in (dict(tol=1), "yes", dict(sources="edge"), dict(tolerance=-1)):
        with pytest.raises(E):
            lm.LabelEvaluator(boundary=bad)


def test_entries_are_declared_and_refuse_bad_arguments_on_the_host():
    """Invalid arguments only: the checks run before any HIP call, so nothing is launched."""
    from kg_instance_segmentation_amd import build
    assert {"kg_label_border_counts", "kg_label_border_d2"} <= set(_lib._SIGS)
    lib = ctypes.CDLL(build.build())
    lib.kg_last_error.restype = ctypes.c_char_p
    P = ctypes.c_void_p
    for name in ("kg_label_border_counts", "kg_label_border_d2"):
        getattr(lib, name).argtypes = _lib._SIGS[name]
    good = dict(a=0x1000, b=0x100000, nimg=1, H=8, W=8, jobs=0x200000, m=1, mode=0, out=0x300000, D=4)

    def call(d2, **kw):
        v = dict(good, **kw)
        args = [P(v["a"]), P(v["b"]), v["nimg"], v["H"], v["W"], P(v["jobs"]), v["m"], v["mode"], P(v["out"])]
        return lib.kg_label_border_d2(*args, v["D"], None) if d2 else lib.kg_label_border_counts(*args, None)
    cases = [dict(a=0), dict(b=0), dict(nimg=0), dict(H=0), dict(W=32769), dict(H=32768, W=32768, nimg=3), dict(jobs=0), dict(m=-1),
             dict(mode=4), dict(mode=-1), dict(out=0), dict(out=0x300002), dict(a=0x1002), dict(jobs=0x200001), dict(out=0x1000 + 16),
             dict(out=0x100000), dict(out=0x200000 + 48)]
    for kw in cases:
        for d2 in (False, True):
            assert call(d2, **kw) != 0 and (b"kg_label_border_d2" if d2 else b"kg_label_border_counts") in lib.kg_last_error(), (kw, d2)
    assert call(True, D=-1) != 0 and b"kg_label_border_d2" in lib.kg_last_error()
    assert call(False, m=0, jobs=0, out=0) == 0 and call(True, m=0, jobs=0, out=0, D=0) == 0       # nothing to do: nothing launched
