"""CPU: label-map evaluation as labelmetrics.py states it in NumPy -- the contingency of two label maps, the candidate pairs and their
bands, the Kaggle score, PQ, AJI, Dice on hand-made cases whose expected values are written out here, the AP part against
evaluation.Evaluator on the same masks -- and the host-side argument validation of kg_label_stats / kg_label_inter_jobs.  Every count is
compared exactly."""
import ctypes
import os

import numpy as np
import pytest
import torch

from kg_instance_segmentation_amd import _lib, evaluation, instances
from kg_instance_segmentation_amd import labelmetrics as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def blocky_map(H, W, n, seed, fill=0.6):
    """A seeded label map of rectangles with ids 1 .. n painted over each other (later ids on top; some ids end up hidden or absent)"""
    rng = np.random.default_rng(seed)
    lab = np.zeros((H, W), np.int32)
    for i in range(1, n + 1):
        if rng.random() > fill + 0.3:
            continue                                                             # an id with no pixel
        y, x = rng.integers(0, H), rng.integers(0, W)
        lab[y:y + rng.integers(1, H // 2 + 2), x:x + rng.integers(1, W // 2 + 2)] = i
    return lab


def brute_contingency(p, g, n_pred, n_gt):
    table = np.zeros((n_pred + 1, n_gt + 1), np.int64)
    for y in range(p.shape[0]):
        for x in range(p.shape[1]):
            table[p[y, x], g[y, x]] += 1
    pairs = [(i, j) for i in range(1, n_pred + 1) for j in range(1, n_gt + 1) if table[i, j]]
    return table[1:].sum(1), table[:, 1:].sum(0), np.array(pairs, np.int32).reshape(-1, 2), np.array([table[i, j] for i, j in pairs], np.int64)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_contingency_host_equals_the_double_loop(seed):
    n_pred, n_gt = (5, 4) if seed else (0, 3)
    p, g = blocky_map(6, 7, n_pred, 10 + seed), blocky_map(6, 7, n_gt, 20 + seed)
    c = lm.contingency_host(p, g, n_pred, n_gt)
    ap, ag, pairs, inter = brute_contingency(p, g, n_pred, n_gt)
    assert c.area_pred.dtype == np.int64 and c.pairs.dtype == np.int32 and c.inter.dtype == np.int64
    assert np.array_equal(c.area_pred, ap) and np.array_equal(c.area_gt, ag) and np.array_equal(c.pairs, pairs) and np.array_equal(c.inter, inter)
    assert c == lm.Contingency(ap, ag, pairs, inter)
    if seed:
        assert len(pairs) > 1
    with pytest.raises(_lib.KGLibraryError, match="2 pixel"):
        bad = p.copy()
        bad[0, 0], bad[5, 6] = n_pred + 1, -3
        lm.contingency_host(bad, g, n_pred, n_gt)
    with pytest.raises(_lib.KGLibraryError):
        lm.contingency_host(p, g[:, :6], n_pred, n_gt)


def test_label_stats_host():
    lab = np.zeros((5, 9), np.int32)
    lab[1:3, 2:6] = 1
    lab[4, 8] = 3
    lab[0, 0] = 3
    want = [[8, 1, 2, 3, 6], [0, 0, 0, 0, 0], [2, 0, 0, 5, 9], [0, 0, 0, 0, 0]]
    got = lm.label_stats_host(lab, 4)
    assert got.dtype == np.int64 and got.tolist() == want
    assert lm.label_stats_host(lab * 0, 0).shape == (0, 5)
    lab[2, 2], lab[3, 3] = 5, -3
    stats, invalid = lm.label_stats_counts_host(lab, 4)
    want[0] = [7, 1, 2, 3, 6]
    assert invalid == 2 and stats.tolist() == want                              # the valid ids stay exact
    with pytest.raises(_lib.KGLibraryError, match="2 pixel"):
        lm.label_stats_host(lab, 4)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_candidate_pairs_hold_every_meeting_pair(seed):
    n_pred, n_gt = 30, 25
    p, g = blocky_map(40, 50, n_pred, seed), blocky_map(40, 50, n_gt, 50 + seed)
    sp, sg = lm.label_stats_host(p, n_pred), lm.label_stats_host(g, n_gt)
    jobs = lm.candidate_pairs(sp, sg)
    assert jobs.dtype == np.int32 and jobs.shape[1] == 6
    c = lm.contingency_host(p, g, n_pred, n_gt)
    listed = {(int(a), int(b)) for a, b in jobs[:, :2]}
    assert len(listed) == len(jobs) and {(int(a), int(b)) for a, b in c.pairs} <= listed and len(listed) > len(c.pairs) > 5
    assert np.all(jobs[:, 4] > jobs[:, 2]) and np.all(jobs[:, 5] > jobs[:, 3])              # no pair with an empty box
    assert [tuple(r) for r in jobs[:, :2]] == sorted(listed)                                  # lexicographic
    plain = [(i + 1, j + 1) for i in range(n_pred) for j in range(n_gt) if sp[i, 0] and sg[j, 0]            # the rule as stated, over all pairs
             and max(sp[i, 1], sg[j, 1]) < min(sp[i, 3], sg[j, 3]) and max(sp[i, 2], sg[j, 2]) < min(sp[i, 4], sg[j, 4])]
    assert [tuple(r) for r in jobs[:, :2]] == plain
    assert np.all(sp[jobs[:, 0] - 1, 0] > 0) and np.all(sg[jobs[:, 1] - 1, 0] > 0)            # no id without area
    for ia, ib, y1, x1, y2, x2 in jobs:                                                       # the box is the intersection of the two boxes
        assert (y1, x1, y2, x2) == (max(sp[ia - 1, 1], sg[ib - 1, 1]), max(sp[ia - 1, 2], sg[ib - 1, 2]), min(sp[ia - 1, 3], sg[ib - 1, 3]),
                                    min(sp[ia - 1, 4], sg[ib - 1, 4]))
    # the jobs counted on the host are the contingency
    inter = lm.inter_jobs_host(p, g, jobs)
    assert np.array_equal(jobs[inter > 0, :2], c.pairs) and np.array_equal(inter[inter > 0], c.inter)
    assert lm.candidate_pairs(sp[:0], sg).shape == (0, 6) and lm.candidate_pairs(sp, sg[:0]).shape == (0, 6)


@pytest.mark.parametrize("cap", [1, 7, 5 * 9, 10 ** 6])
def test_bands_tile_the_box_exactly(cap):
    jobs = np.array([[1, 2, 3, 4, 8, 13], [2, 1, 0, 0, 1, 1], [3, 3, 2, 2, 2, 9], [4, 5, 10, 0, 13, 20]], np.int32)        # 5 x 9, 1 x 1, empty, 3 x 20
    pieces, owner = lm.split_jobs(jobs, cap)
    assert pieces.dtype == np.int32 and owner.dtype == np.int64 and np.all(np.diff(owner) >= 0)
    for k, (ia, ib, y1, x1, y2, x2) in enumerate(jobs):
        mine = pieces[owner == k]
        cover = np.zeros((20, 30), np.int64)
        for pa, pb, a1, b1, a2, b2 in mine:
            assert (pa, pb) == (ia, ib) and (a2 - a1) * (b2 - b1) <= cap
            assert (a2 > a1 and b2 > b1) or len(mine) == 1                                    # only a job that was empty has an empty piece
            cover[a1:a2, b1:b2] += 1
        want = np.zeros_like(cover)
        want[y1:y2, x1:x2] = 1
        assert np.array_equal(cover, want), k                                                 # every pixel of the box exactly once, none outside
    if cap >= 60:
        assert np.array_equal(pieces, jobs)
    if cap == 5 * 9:
        assert (owner == 0).sum() == 1 and (owner == 3).sum() == 2
    if cap == 1:
        assert len(pieces) == 45 + 1 + 1 + 60
    # the band counts add up to the job's count
    a, b = blocky_map(20, 30, 5, 4), blocky_map(20, 30, 5, 5)
    got = np.zeros(len(jobs), np.int64)
    np.add.at(got, owner, lm.inter_jobs_host(a, b, pieces))
    assert np.array_equal(got, lm.inter_jobs_host(a, b, jobs))
    with pytest.raises(_lib.KGLibraryError):
        lm.split_jobs(jobs, 0)


# ---- metrics on hand-made cases ---------------------------------------------------------------------------------------------------------

def strip(runs, n=16):
    """a 1 x n label map from (id, start, stop) runs"""
    lab = np.zeros((1, n), np.int32)
    for i, a, b in runs:
        lab[0, a:b] = i
    return lab


def score(pred, n_pred, gt, n_gt, conf=None):
    ev = lm.LabelEvaluator()
    c = ev.add((pred, n_pred), (gt, n_gt), np.linspace(0.9, 0.5, n_pred) if conf is None else conf)
    return c, ev.summary()


def test_identical_maps_score_one():
    lab = np.zeros((4, 5), np.int32)
    lab[0:2, 0:2], lab[3, 1:4] = 1, 2
    c, s = score(lab, 2, lab, 2)
    assert c.pairs.tolist() == [[1, 1], [2, 2]] and c.inter.tolist() == [4, 3]
    assert lm.kaggle_score(c) == 1.0 and lm.panoptic(c) == {"tp": 2, "fp": 0, "fn": 0, "sum_iou": 2.0} and lm.aji(c) == (7, 7) and lm.dice(c) == (14, 14)
    assert s["kaggle"] == 1.0 and s["pq"] == 1.0 and s["sq"] == 1.0 and s["dq"] == 1.0 and s["aji"] == 1.0 and s["dice"] == 1.0 and s["images"] == 1
    assert np.array_equal(s["seg_ap"], np.ones(10)) and np.array_equal(s["seg_iou"], np.ones(10))


def test_disjoint_maps_score_zero():
    c, s = score(strip([(1, 0, 3)]), 1, strip([(1, 5, 9)]), 1)
    assert len(c.pairs) == 0 and c.area_pred.tolist() == [3] and c.area_gt.tolist() == [4]
    assert lm.kaggle_score(c) == 0.0 and lm.panoptic(c) == {"tp": 0, "fp": 1, "fn": 1, "sum_iou": 0.0} and lm.aji(c) == (0, 7) and lm.dice(c) == (0, 7)
    assert s["kaggle"] == 0.0 and s["pq"] == 0.0 and s["sq"] == 0.0 and s["dq"] == 0.0 and s["aji"] == 0.0 and s["dice"] == 0.0
    assert np.array_equal(s["seg_ap"], np.zeros(10))


def test_an_empty_side():
    gt = strip([(1, 2, 6), (2, 8, 10)])
    c, s = score(strip([]), 0, gt, 2)                                           # nothing predicted
    assert lm.kaggle_score(c) == 0.0 and lm.panoptic(c) == {"tp": 0, "fp": 0, "fn": 2, "sum_iou": 0.0} and lm.aji(c) == (0, 6) and lm.dice(c) == (0, 6)
    assert s["kaggle"] == 0.0 and s["pq"] == 0.0 and s["dq"] == 0.0 and s["aji"] == 0.0 and s["dice"] == 0.0
    c, s = score(gt, 2, strip([]), 0)                                           # nothing to find
    assert lm.kaggle_score(c) == 0.0 and lm.panoptic(c) == {"tp": 0, "fp": 2, "fn": 0, "sum_iou": 0.0} and lm.aji(c) == (0, 6) and lm.dice(c) == (0, 6)
    assert s["kaggle"] == 0.0 and s["pq"] == 0.0 and s["aji"] == 0.0 and s["dice"] == 0.0
    c, s = score(strip([]), 0, strip([]), 0)                                    # neither: the image has no score
    assert lm.kaggle_score(c) is None and lm.aji(c) == (0, 0) and lm.dice(c) == (0, 0)
    assert s["kaggle"] is None and s["pq"] is None and s["aji"] is None and s["dice"] is None and s["images"] == 1 and s["seg_ap"] is None


def test_one_prediction_over_two_objects():
    pred, gt = strip([(1, 0, 11)]), strip([(1, 0, 8), (2, 8, 11)])            # IoU 8 / 11 = 0.727 and 3 / 11
    c, s = score(pred, 1, gt, 2)
    assert c.pairs.tolist() == [[1, 1], [1, 2]] and c.inter.tolist() == [8, 3] and c.iou().tolist() == [8 / 11, 3 / 11]
    # TP_t = 1 at t = 0.5 .. 0.7 (five thresholds): 1 / (1 + 2 - 1) each, 0 at the other five
    assert lm.kaggle_score(c) == pytest.approx(0.25, abs=1e-15) and s["kaggle"] == lm.kaggle_score(c)
    assert lm.panoptic(c) == {"tp": 1, "fp": 0, "fn": 1, "sum_iou": 8 / 11}
    assert s["pq"] == (8 / 11) / 1.5 and s["sq"] == 8 / 11 and s["dq"] == 1 / 1.5
    assert lm.aji(c) == (11, 22) and s["aji"] == 0.5                            # both objects take prediction 1: C = 8 + 3, U = 11 + 11
    assert lm.dice(c) == (22, 22) and s["dice"] == 1.0
    with pytest.raises(ValueError):
        lm.kaggle_score(c, [0.4, 0.5])
    with pytest.raises(ValueError):
        lm.panoptic(c, 0.3)


def test_iou_of_exactly_one_half_is_no_match():
    c, s = score(strip([(1, 2, 4)]), 1, strip([(1, 2, 6)]), 1)                  # 2 / (2 + 4 - 2)
    assert c.iou().tolist() == [0.5]
    assert lm.kaggle_score(c) == 0.0 and lm.panoptic(c) == {"tp": 0, "fp": 1, "fn": 1, "sum_iou": 0.0} and lm.kaggle_score(c, [0.5]) == 0.0
    assert s["pq"] == 0.0 and lm.aji(c) == (2, 4) and lm.dice(c) == (4, 6)
    # the reference's AP matching is `>=`: there the pair is a true positive at 0.5 and at no other threshold
    m = lm.match(c, [0.9])
    assert [r["tp"].tolist() for r in m["per_threshold"]] == [[1.0]] + [[0.0]] * 9


def test_aji_tie_goes_to_the_smallest_id():
    gt = strip([(1, 0, 6)])
    pred = strip([(1, 0, 2), (2, 2, 5), (2, 8, 11)])                           # 2 / (6 + 2 - 2) == 3 / (6 + 6 - 3) == 1 / 3
    c, _ = score(pred, 2, gt, 1)
    assert c.iou()[0] == c.iou()[1] and c.inter.tolist() == [2, 3]
    assert lm.aji(c) == (2, 12)                                                 # with prediction 2 it would be (3, 11)
    swapped = strip([(2, 0, 2), (1, 2, 5), (1, 8, 11)])
    assert lm.aji(lm.contingency_host(swapped, gt, 2, 1)) == (3, 11)


def test_hidden_prediction_is_a_false_positive_and_not_in_P():
    lab = strip([(1, 3, 9)])
    c, s = score(lab, 2, lab, 1, conf=[0.8, 0.9])                               # id 2 has no pixel and the higher confidence
    assert c.area_pred.tolist() == [6, 0]
    assert lm.kaggle_score(c) == 1.0 and lm.panoptic(c) == {"tp": 1, "fp": 0, "fn": 0, "sum_iou": 1.0} and lm.aji(c) == (6, 6)
    m = lm.match(c, [0.8, 0.9])
    assert m["order"].tolist() == [1, 0]
    assert all(r["fp"].tolist() == [1.0, 0.0] and r["tp"].tolist() == [0.0, 1.0] for r in m["per_threshold"])
    assert np.allclose(s["seg_ap"], 0.5) and s["kaggle"] == 1.0 and s["pq"] == 1.0          # precision 0 then 1 / 2 at recall 1


def test_summary_over_two_images():
    ev = lm.LabelEvaluator()
    ev.add((strip([(1, 0, 11)]), 1), (strip([(1, 0, 8), (2, 8, 11)]), 2), [0.9])
    ev.add((strip([(1, 0, 4)]), 1), (strip([(1, 0, 4)]), 1), [0.8])
    ev.add((strip([]), 0), (strip([]), 0), [])
    s = ev.summary()
    assert s["images"] == 3 and s["kaggle"] == pytest.approx((0.25 + 1) / 2, abs=1e-15) and s["aji"] == 0.75
    assert s["sq"] == (8 / 11 + 1) / 2 and s["dq"] == 2 / 2.5 and s["pq"] == (8 / 11 + 1) / 2.5 and s["dice"] == (22 + 8) / (22 + 8)
    assert ev.seg.npos == 3
    with pytest.raises(_lib.KGLibraryError):
        ev.add((strip([]), 0), (np.zeros((2, 16), np.int32), 0))              # a size mismatch
    with pytest.raises(ValueError):
        ev.add((strip([(1, 0, 4)]), 1), (strip([]), 0), [0.5, 0.4])          # one confidence per id


# ---- the AP part against Evaluator --------------------------------------------------------------------------------------------------------

def cell_masks(H, W, cell, shift, seed):
    """one seeded rectangle inside every cell of a grid shifted by `shift`: masks that do not overlap, uint8 [n, H, W]"""
    rng = np.random.default_rng(seed)
    out = []
    for y0 in range(shift, H - cell + 1, cell):
        for x0 in range(shift, W - cell + 1, cell):
            if rng.random() < 0.15:
                continue
            h, w = rng.integers(cell // 3, cell + 1, 2)
            y, x = y0 + rng.integers(0, cell - h + 1), x0 + rng.integers(0, cell - w + 1)
            m = np.zeros((H, W), np.uint8)
            m[y:y + h, x:x + w] = 1
            out.append(m)
    return np.stack(out)


def tight(masks):
    out = np.zeros((len(masks), 4), np.float32)
    for k, m in enumerate(masks):
        ys, xs = np.nonzero(m)
        out[k] = ys.min(), xs.min(), ys.max() + 1, xs.max() + 1
    return out


def shrunk(masks, rng):
    """every rectangle trimmed by 0 or 1 pixel per side (at least one pixel stays): IoUs from 1 down, still no overlap"""
    out = np.zeros_like(masks)
    for k, (y1, x1, y2, x2) in enumerate(tight(masks).astype(np.int64)):
        t = rng.integers(0, 3, 4) // 2
        a1, b1 = min(y1 + t[0], y2 - 1), min(x1 + t[1], x2 - 1)
        out[k, a1:max(y2 - t[2], a1 + 1), b1:max(x2 - t[3], b1 + 1)] = 1
    return out


def same(a, b):
    if a is None or b is None:
        return a is b
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def test_ap_part_equals_evaluator():
    ref, ev = evaluation.Evaluator(), lm.LabelEvaluator()
    ev_masks = lm.LabelEvaluator()
    for img in range(3):
        rng = np.random.default_rng(100 + img)
        det = cell_masks(48, 72, 12, img, img)
        gt = shrunk(det, rng)
        det, gt = det[rng.random(len(det)) < 0.85], gt[rng.random(len(gt)) < 0.85]            # detections without object and the reverse
        conf = rng.random(len(det)).astype(np.float32)
        conf[1] = conf[0]                                                                     # a tie
        dets = np.concatenate([tight(det), conf[:, None]], 1)
        inter = (det[:, None].astype(np.int64) * gt[None]).sum((2, 3))
        area_d, area_g = det.sum((1, 2), dtype=np.int64), gt.sum((1, 2), dtype=np.int64)
        iou = inter / (area_d[:, None] + area_g[None] - inter).astype(np.float64)
        ref.add_batch([[det, dets]], [gt], [tight(gt)], iou_tables=[iou])
        pl, gl = instances.label_map_host(det), instances.label_map_host(gt)
        assert np.array_equal(lm.label_stats_host(pl, len(det))[:, 0], area_d)               # nothing overlaps: the maps hold the masks
        c = ev.add((pl, len(det)), (gl, len(gt)), conf)
        assert np.array_equal(c.inter, inter[inter > 0]) and np.array_equal(c.pairs, np.argwhere(inter > 0) + 1)
        ev_masks.add((pl, len(det)), gt, conf)                                                # GT as dense masks: the same map
    want, got, got2 = ref.summary(), ev.summary(), ev_masks.summary()
    assert ev.seg.npos == ref.seg.npos
    assert len(want["seg_ap"]) == 10 and 0 < want["seg_ap"][-1] < want["seg_ap"][0] < 1
    assert np.array_equal(got["seg_ap"], want["seg_ap"]) and np.array_equal(got["seg_iou"], want["seg_iou"])
    for k in got:
        assert same(got[k], got2[k]), k


# ---- the C entries ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from kg_instance_segmentation_amd import build
    lib = ctypes.CDLL(build.build())
    lib.kg_last_error.restype = ctypes.c_char_p
    for name in ("kg_label_stats", "kg_label_inter_jobs"):
        assert name in _lib.SYMBOLS
        getattr(lib, name).argtypes = _lib._SIGS[name]
        getattr(lib, name).restype = ctypes.c_int
    return lib


def test_entry_points_validate_on_the_host(lib):
    buf = (ctypes.c_char * 4096)()                         # stands for every device buffer: a failed check returns before any HIP call
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)

    def stats(labels=p, H=24, W=70, n=3, out=p, invalid=p):
        return lib.kg_label_stats(labels, H, W, n, out, invalid, None)

    for kw in (dict(labels=None), dict(out=None), dict(invalid=None), dict(H=0), dict(W=0), dict(H=-1), dict(n=-1), dict(H=1 << 16, W=1 << 15),
               dict(n=1 << 30), dict(labels=ctypes.c_void_p(p.value + 2)), dict(out=ctypes.c_void_p(p.value + 1)), dict(invalid=ctypes.c_void_p(p.value + 2))):
        assert stats(**kw) != 0 and b"kg_label_stats" in lib.kg_last_error(), kw

    def inter(a=p, b=p, H=24, W=70, jobs=p, m=3, count=p):
        return lib.kg_label_inter_jobs(a, b, H, W, jobs, m, count, None)

    for kw in (dict(a=None), dict(b=None), dict(jobs=None), dict(count=None), dict(H=0), dict(W=0), dict(W=-5), dict(m=-1), dict(H=1 << 16, W=1 << 15),
               dict(a=ctypes.c_void_p(p.value + 2)), dict(b=ctypes.c_void_p(p.value + 1)), dict(jobs=ctypes.c_void_p(p.value + 2)),
               dict(count=ctypes.c_void_p(p.value + 4))):
        assert inter(**kw) != 0 and b"kg_label_inter_jobs" in lib.kg_last_error(), kw
    assert inter(m=0, jobs=None, count=None) == 0          # nothing to do: no launch, no device needed


def test_cpu_tensors_are_refused():
    lab = torch.zeros(6, 7, dtype=torch.int32)
    with pytest.raises(_lib.KGLibraryError, match="label_stats_host"):
        lm.label_stats(lab, 2)
    with pytest.raises(_lib.KGLibraryError, match="contingency_host"):
        lm.contingency(lab, lab, 1, 1)
    with pytest.raises(_lib.KGLibraryError):
        lm.inter_jobs(lab, lab, np.zeros((0, 6), np.int32))
    with pytest.raises(_lib.KGLibraryError):
        lm.contingency(lab.numpy(), lab.numpy(), 1, 1)
    c = lm.LabelEvaluator().add((lab, 0), (lab.numpy(), 0))                     # a host tensor takes the host route
    assert len(c.pairs) == 0


def test_product_module_stands_alone():
    src = open(os.path.join(ROOT, "kg_instance_segmentation_amd", "labelmetrics.py")).read()
    assert "oracle" not in src
