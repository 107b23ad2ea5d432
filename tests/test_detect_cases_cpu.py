"""The case tables of tests/detect_cases.py contain what the GPU tests of the detection stage rely on -- asserted from the oracle alone."""
import numpy as np
import pytest

import detect_cases as dc
from oracle import postproc as op


def present(skel):
    return (skel[:, :, 0] > 0.).sum(1) if len(skel) else np.zeros(0, int)


def n_boxes(skel):
    return len(op.boxes(op.refine(skel), 1)) if len(skel) else 0


# ---- part A -------------------------------------------------------------------------------------------------------------------------------

COUNTS = {(33, 70): (134, 25, 10, 12), (25, 17): (18, 5, 2, 2), (65, 87): (373, 56, 37, 39), (31, 97): (165, 34, 18, 19),
          (24, 256): (356, 71, 34, 40), (24, 257): (376, 70, 33, 36), (24, 512): (761, 139, 75, 86), (24, 513): (768, 126, 77, 80),
          (24, 1024): (1529, 300, 153, 174), (24, 1025): (1541, 286, 150, 166), (1025, 24): (1489, 280, 137, 155)}


@pytest.mark.parametrize("H,W", sorted(COUNTS))
def test_random_map_counts(H, W):
    """peaks, skeletons, skeletons of three or more keypoints and boxes of random_maps(H, W) with the default seed 1000 H + W"""
    r = dc.stage_reference(H, W)
    assert (r["npeaks"], len(r["skel"]), int((present(r["skel"]) >= 3).sum()), n_boxes(r["skel"])) == COUNTS[(H, W)]


def test_sizes_are_ragged_and_cross_the_seams():
    assert all(H % 32 or W % 32 for H, W in dc.RAGGED)
    for a, b in ((256, 257), (512, 513), (1024, 1025)):
        for s in (a, b):
            assert (24, s) in dc.SEAMS and ((s, 24) in dc.SEAMS or s in (256, 512))
    assert {(40, 256), (40, 257), (257, 40)} <= set(dc.SEAMS)
    assert set(dc.BATCH_SIZES) <= set(dc.RAGGED + dc.SEAMS) and {(33, 70), (24, 513), (24, 1025)} <= set(dc.BATCH_SIZES)


@pytest.mark.parametrize("H,W", dc.SEAMS)
def test_seam_sizes_group_many_skeletons(H, W):
    """at least 100 skeletons, 30 of them with three or more keypoints -- but for the 24-pixel strips of 256 / 257 columns, which hold 70 .. 76
    (their exact counts are asserted here and in COUNTS); the 40-pixel strips of the same widths meet the 100 on that seam"""
    r = dc.stage_reference(H, W)
    short_strips = {(24, 256): 71, (24, 257): 70, (257, 24): 76}
    if (H, W) in short_strips:
        assert len(r["skel"]) == short_strips[(H, W)]
        assert len(dc.stage_reference(*{(24, 256): (40, 256), (24, 257): (40, 257), (257, 24): (257, 40)}[(H, W)])["skel"]) >= 100
    else:
        assert len(r["skel"]) >= 100
    assert int((present(r["skel"]) >= 3).sum()) >= 30
    assert r["npeaks"] <= dc.GK_NL                       # the size alone decides the route


@pytest.mark.parametrize("H,W", [s for s in dc.RAGGED if s not in dc.THIN])
def test_ragged_sizes_give_boxes(H, W):
    assert n_boxes(dc.stage_reference(H, W)["skel"]) >= 2


@pytest.mark.parametrize("H,W", dc.THIN)
def test_thin_maps_carry_values_through_the_reflection(H, W):
    """kp = 0.9 everywhere: the blurred map is positive in every channel although the map is narrower than the Gaussian's reach"""
    assert not op.peaks(op.gauss(op.hough(*dc.random_maps(H, W)[:2])))[0].size          # (the random kp: no peak)
    r = dc.stage_reference(H, W)
    assert (r["heat"].reshape(5, -1).max(1) > 0).all()
    assert r["blur"].shape == (5, H, W) and (r["blur"].reshape(5, -1).max(1) > 0).all() and np.isfinite(r["blur"]).all()


def test_seam_routing():
    want = {(24, 256): 3, (24, 257): 4, (257, 24): 4, (24, 512): 4, (24, 513): 5, (513, 24): 5, (24, 1024): 5, (1024, 24): 5,
            (24, 1025): "general", (1025, 24): "general", (40, 256): 3, (40, 257): 4, (257, 40): 4}
    assert set(want) == set(dc.SEAMS)
    for (H, W), route in want.items():
        assert dc.group_route(dc.stage_reference(H, W)["npeaks"], H, W) == route, (H, W)
    assert {dc.group_route(dc.stage_reference(H, W)["npeaks"], H, W) for H, W in dc.RAGGED} == {3}
    assert dc.group_route(dc.GK_NL, 64, 64) == 3 and dc.group_route(dc.GK_NL + 1, 64, 64) == "general"


@pytest.mark.parametrize("case", dc.SYNTH)
def test_synth_cases_hold_objects(case):
    r = dc.synth_reference(*case)
    assert len(r["skel"]) >= 1 and int((present(r["skel"]) >= 3).sum()) >= 1
    if case == (24, 1025, 20, 5):
        assert len(r["skel"]) == 16 and dc.group_route(r["npeaks"], 24, 1025) == "general"


def test_end_to_end_images():
    decs, refs = dc.end_to_end()
    assert [tuple(d[0].shape[-2:]) for d in decs[0]] == [(200, 136), (100, 68), (50, 34), (25, 17)]
    assert refs[1] is None and len(refs[0]) >= 10 and len(refs[2]) >= 10


# ---- part B -------------------------------------------------------------------------------------------------------------------------------

def test_refine_leaves_no_row_for_the_rejecting_branches():
    """Over all 32 mask patterns: the rows refine_skeleton keeps are exactly the rows skeleton_box accepts.  With do_refine the two rejecting
    branches of skeleton_box are therefore unreachable -- their rows leave as 'refined out' -- and refine changes no result."""
    t = dc.skeleton_table(32, 0)
    assert len({tuple(r[:, 0] > 0) for r in t}) == 32
    for r in t:
        assert dc.refine_keeps(r) == (dc.box_branch(r) not in dc.REJECTING)


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049, 3000])
def test_skeleton_table_reaches_every_branch(n):
    t = dc.skeleton_table(n, n)
    off, on = dc.table_branches(t, 0), dc.table_branches(t, 1)
    assert set(off) == set(dc.BOX_BRANCHES)                                                        # both rejecting ones included
    assert set(on) == (set(dc.BOX_BRANCHES) - set(dc.REJECTING)) | {"refined out"}
    for br in (off, on):
        ok = np.array([b not in dc.REJECTING + ("refined out",) for b in br])
        assert len(dc.boxes_reference(t, 1, br is on)) == ok.sum() and 0 < ok.sum() < n
        for lo, hi in ((n - 64, n),) if n < 1088 else ((960, 1024), (1024, 1088)):             # both sides of the chunk seam
            assert ok[lo:hi].any() and not ok[lo:hi].all() and (ok[lo:hi][1:] != ok[lo:hi][:-1]).sum() >= 8
    x, y, c = t[:, :, 0], t[:, :, 1], t[:, :, 2]
    four = (x[:, :4] > 0).all(1)
    assert (y[four, 0] < y[four, 1]).any() and (y[four, 0] > y[four, 1]).any()                     # min(tl.y, tr.y) is either corner
    assert (x[four, 1] < x[four, 3]).any() and (x[four, 1] > x[four, 3]).any()                     # max(tr.x, br.x) too
    assert ((x == 0) & (y > 0) & (c > 0)).any()                                                    # a peak of column 0 counts as missing
    assert (c[6::7] == 0.5)[x[6::7] > 0].all()


def test_box_overflow_case_overflows():
    assert len(dc.boxes_reference(dc.skeleton_table(3000, 3000), 1, 0)) > 1000


# ---- part C -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2047, 2048, 2049, 5000])
def test_box_population_suppresses_and_ties(n):
    b = dc.nms_case(str(n))
    for th in (0.5, 0.1):
        k = len(dc.nms_reference(str(n), th))
        assert 100 <= k < n, (n, th, k)
    assert dc.tied(b) >= n / 2 and dc.tied(b) > 1900
    assert np.array_equal(b[dc.nms_reference(str(n), 0.5)], op.nms(b, 0.5))


def test_population_sizes_straddle_the_lds_limit():
    assert {dc.NMS_NL - 1, dc.NMS_NL, dc.NMS_NL + 1} <= set(dc.NMS_SIZES) and max(dc.NMS_SIZES) > 2 * dc.NMS_NL


@pytest.mark.parametrize("n", [300, 2049])
def test_spliced_rows_do_what_they_are_there_for(n):
    b, where = dc.spliced_population(n, 1)
    assert len(b) == n + 40 and np.array_equal(b[np.setdiff1d(np.arange(n + 40), where)], dc.box_population(n, 1))
    assert (len(b) <= dc.NMS_NL) == (n == 300)
    dup, zero, neg, inv = where[:20], where[20:30], where[30:35], where[35:]
    same = [i for i in zero if (b[i, :4] == b[zero[5], :4]).all()]
    assert len(same) == 5
    for th in (0.0, 0.1, 0.5, 1.0):
        kept = set(dc.nms_pick(b, th).tolist())
        # Equal confidences are ranked by index ascending and picked from the top: of equal rows (IoU 1) the LAST index is picked first and
        # suppresses the others -- unless thresh is 1, where 1 <= thresh keeps them all.
        for i in dup:
            twins = np.flatnonzero((b == b[i]).all(1))
            assert len(twins) >= 2
            if th < 1.0:
                assert not (kept & set(twins[:-1].tolist()))
            else:
                assert set(twins.tolist()) <= kept
        # two zero-area boxes: inter = 0 and union = (0 - 0) + 0, so 0 / 0 = NaN, and NaN is suppressed at EVERY thresh: the first one picked
        # (highest confidence, then highest index) is the only one of the ten that stays; against a box with an area the IoU is 0
        top = max(zero, key=lambda i: (b[i, 4], i))
        assert kept & set(zero.tolist()) == {top}
    assert ((b[zero, 2] - b[zero, 0]) * (b[zero, 3] - b[zero, 1]) == 0).all()
    assert (b[neg, :2] < 0).all() and (b[inv, 2] < b[inv, 0]).all()
    assert len(dc.nms_pick(b, 1.0)) == len(b) - 9             # thresh 1 keeps everything but nine of the ten zero-area boxes


def test_grid_population_chains():
    b = dc.grid_population()
    k = dc.nms_pick(b, 0.3)
    assert k[0] == 0 and 1 not in k and 9 not in k and 2 in k and 10 in k and 20 < len(k) < 81
    assert len(dc.nms_pick(b, 0.34)) == 81                    # the neighbours' IoU is 1/3


# ---- part D -------------------------------------------------------------------------------------------------------------------------------

def test_capacity_cases_rest_on_these_counts():
    full = dc.cap_reference(65, 87, 373)
    assert full["npeaks"] == 373 and len(full["skel"]) == 56
    wide = dc.cap_reference(24, 1025, 1541)
    assert wide["npeaks"] == 1541 and dc.group_route(1541, 24, 1025) == "general" and dc.group_route(500, 24, 1025) == "general"
    assert np.array_equal(full["skel"], dc.stage_reference(65, 87)["skel"])


@pytest.mark.parametrize("case", dc.CAP_CASES)
def test_truncated_grouping_yields_skeletons(case):
    H, W, pc, sc = case
    r = dc.cap_reference(H, W, pc)
    assert len(r["peaks"]) == min(pc, r["npeaks"]) and len(r["skel"]) >= 1
    full = dc.cap_reference(H, W, r["npeaks"])
    assert np.array_equal(r["peaks"], full["peaks"][:pc])                    # scan order: channel, row, column
    assert (np.diff(r["peaks"][:, 0] * H * W + r["peaks"][:, 2] * W + r["peaks"][:, 1]) > 0).all()
    if case in dc.SKEL_OVERFLOW:
        assert len(r["skel"]) > sc
    else:
        assert len(r["skel"]) <= sc
    if 1 < pc <= r["npeaks"] // 2:
        assert not np.array_equal(r["skel"], full["skel"][:len(r["skel"])])  # the truncation is visible in the result


def test_capacity_batch_is_below_at_and_above():
    maps, thresh, refs = dc.cap_batch()
    cap = dc.CAP_BATCH_PEAK_CAP
    assert thresh > 0.004
    assert refs[0]["npeaks"] < cap and refs[1]["npeaks"] == cap and refs[2]["npeaks"] > cap
    assert [len(r["peaks"]) for r in refs] == [refs[0]["npeaks"], cap, cap] and all(len(r["skel"]) >= 1 for r in refs)
