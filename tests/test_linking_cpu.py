"""CPU: the host statements of linking.py -- overlap lists against a per-pixel loop and against labelmetrics' contingency, the pager over
the row semantics, the linking rule on hand cases, tracks on a five-frame sequence with a death, a division, an exit and a birth.  Every
comparison is exact integer equality."""
import numpy as np
import pytest

import linking_cases as lc
from kg_instance_segmentation_amd import _lib, labelmetrics as lm
from kg_instance_segmentation_amd import linking as lk

I32 = lc.I32
E = _lib.KGLibraryError


@pytest.fixture(scope="module")
def pair():
    a, b = lc.blob_pair()
    return a, b, 30, 40


@pytest.mark.parametrize("shift", [(0, 0), (1, 0), (-1, 0), (3, -5), (70, 0)])
def test_overlaps_host_equals_a_pixel_loop(pair, shift):
    a, b, na, nb = pair
    ov = lk.overlaps_host(a, b, na, shift=shift)
    assert len(ov) == na and ov.values.dtype == np.int64
    assert lc.as_lists(ov) == lc.loop_overlaps(a, b, na, *shift)
    assert all(np.all(np.diff(ov.of(k)[0]) > 0) for k in range(na))                         # ascending, distinct
    assert np.array_equal(ov.area, lc.boxes_of(a, na)[:, 0])
    if shift == (70, 0):                                              # shifted by H: no partner lies in the map
        assert len(ov.values) == 0 and np.array_equal(ov.outside, ov.area) and not ov.zero.any()
    else:
        assert len(ov.values) > na and ov.zero.any() and (ov.outside.any() == (shift != (0, 0)))


def test_zero_shift_equals_contingency(pair):
    a, b, na, nb = pair
    ov = lk.overlaps_host(a, b, na)
    c = lm.contingency_host(a, b, na, nb)
    p = ov.pairs()
    assert np.array_equal(p[:, :2], c.pairs) and np.array_equal(p[:, 2], c.inter) and np.array_equal(ov.area, c.area_pred)
    assert np.array_equal(ov.iou(c.area_gt), c.iou())                                       # the same floats, not close ones
    assert np.array_equal(ov.fraction_of_b(c.area_gt), c.inter / c.area_gt[c.pairs[:, 1] - 1].astype(np.float64))


@pytest.mark.parametrize("shift", [(0, 0), (3, -5), (-1, 0)])
def test_swapped_maps_and_negated_shift_transpose(pair, shift):
    a, b, na, nb = pair
    fwd = lk.overlaps_host(a, b, na, shift=shift).pairs()
    back = lk.overlaps_host(b, a, nb, shift=(-shift[0], -shift[1])).pairs()
    back = back[:, [1, 0, 2]]
    assert np.array_equal(fwd, back[np.lexsort((back[:, 1], back[:, 0]))])


def test_every_job_adds_up(pair):
    a, b, na, nb = pair
    stack_a, stack_b = np.stack([a, b]), np.stack([b, a, a])
    jobs = np.concatenate([lc.jobs9(lc.boxes_of(a, na), 0, 1, 2, -3), lc.jobs9(lc.boxes_of(b, nb), 1, 0, -40, 60),
                           [[0, 7, -5, -5, 500, 500, 2, 0, 1], [1, 0, 0, 0, 70, 131, 2, 1, 1]]])
    ov = lk.overlaps_host(stack_a, stack_b, jobs)
    sums = np.zeros(len(ov), np.int64)
    np.add.at(sums, ov.rows(), ov.pixels)
    assert np.array_equal(ov.area, ov.zero + ov.outside + sums) and ov.area[-1] > 0 and ov.outside.any() and ov.zero.any()
    assert lc.as_lists(ov.slice(0, na)) == lc.loop_overlaps(a, a, na, 2, -3)                # id itself is an ordinary partner value
    assert (ov.slice(0, na).pairs()[:, 0] == ov.slice(0, na).pairs()[:, 1]).any()


def big_jobs(a, na):
    """the ids inside their boxes, shifted, and four whole-map boxes that a band rule of 4096 pixels cuts"""
    whole = [[0, i, -9, -9, 999, 999, 0, 2, 3] for i in (1, 2, 9, 77)]
    return np.concatenate([lc.jobs9(lc.boxes_of(a, na), dy=2, dx=3), whole])


@pytest.mark.parametrize("cap", [2 ** 30, 4096])
@pytest.mark.parametrize("slots", [1, 2, 3, 64])
def test_pager_over_the_row_semantics(pair, slots, cap):
    a, b, na, nb = pair
    jobs = big_jobs(a, na)
    want = lk.overlaps_host(a, b, jobs)
    assert np.diff(want.indptr).max() >= 4 and want.area[-1] == 0 and want.area[-2] > 0
    rounds = []

    def rows(table):
        rounds.append(len(table))
        return lk.overlaps_rows_host(a, b, table, slots)
    assert lk.paged(rows, jobs, 70, 131, slots, cap) == want
    assert (rounds[0] > len(jobs)) == (cap == 4096) and (len(rounds) > 1) == (slots < 64)


def test_row_semantics():
    a, b, vals = lc.checkerboard()
    job = [[0, 5, 0, 0, 24, 26, 0, 0, 0]]
    full = lk.overlaps_host(a, b, job)
    assert full.values.tolist() == sorted(vals.tolist()) and (full.pixels == 4).all() and full.area[0] == 400 and full.zero[0] == 0
    first = lk.overlaps_rows_host(a, b, lc.row_jobs(job), 64)
    assert first[0, :5].tolist() == [64, 1, 400, 0, 0] and first[0, 5] == I32.min
    rest = lk.overlaps_rows_host(a, b, lc.row_jobs(job, 1, int(first[0, 5 + 2 * 63])), 64)
    assert rest[0, :5].tolist() == [36, 0, 400, 0, 0] and rest[0, 5 + 2 * 35] == I32.max and not rest[0, 5 + 2 * 36:].any()
    for after, left in ((I32.min, 99), (I32.max, 0), (I32.max - 1, 1)):
        r = lk.overlaps_rows_host(a, b, lc.row_jobs(job, 1, after), 64)
        assert r[0, :5].tolist() == [min(left, 64), left > 64, 400, 0, 0]                   # the header is over all of P on a resumed row
    assert np.array_equal(lk.overlaps_rows_host(a, b, lc.row_jobs(job, 0, I32.max), 64), first)        # resume == 0 ignores after
    bad = [[1, 5, 0, 0, 24, 26, 0, 0, 0], [0, 5, 0, 0, 24, 26, -1, 0, 0], [0, 5, 9, 9, 3, 3, 0, 0, 0], [0, 6, 0, 0, 24, 26, 0, 0, 0]]
    assert not lk.overlaps_rows_host(a, b, lc.row_jobs(bad), 3).any()
    far = lk.overlaps_rows_host(a, b, lc.row_jobs([[0, 5, 0, 0, 24, 26, 0, I32.min, I32.max]]), 3)
    assert far[0].tolist() == [0, 0, 400, 0, 400] + [0] * 6


def test_arguments_are_checked(pair):
    a, b, na, nb = pair
    for bad in (lambda: lk.overlaps_host(a, b[:-1], na), lambda: lk.overlaps_host(a, np.stack([b, b]), na),
                lambda: lk.overlaps_host(a, b, na, pairs=[(0, 1)]), lambda: lk.overlaps_host(a, b, na, shift=(1, 2, 3)),
                lambda: lk.overlaps_host(a, b, na, shift=(0.5, 0)), lambda: lk.overlaps_host(a, b, na - 1),
                lambda: lk.overlaps_host(a, b, np.zeros((2, 9), np.int64), shift=(1, 1)),
                lambda: lk.overlaps_rows_host(a, b, np.zeros((1, 11), np.int64), 0), lambda: lk.overlaps_rows_host(a, b, np.zeros((1, 9), np.int64), 4),
                lambda: lk.overlaps_host(a, b, na).iou(np.ones(3, np.int64)), lambda: lk.link(None, [1])):
        with pytest.raises(E):
            bad()
    six = lk.overlaps_host(np.stack([a, a]), np.stack([b, b]), np.array([[1, 3, 0, 0, 70, 131], [2, 3, 0, 0, 70, 131], [0, 3, 0, 0, 70, 131]]),
                           pairs=[(0, 1), (1, 0)], shift=[(0, 0), (1, 1)])
    assert six.area.tolist() == [int((a == 3).sum()), 0, int((a == 3).sum())]               # column 0 names the pair; pair 2 does not exist
    assert lc.as_lists(six.slice(0, 1)) == [lc.loop_overlaps(a, b, 3, 1, 1)[2]]
    assert len(lk.overlaps_host(a, b, [])) == 0


# ---- links ------------------------------------------------------------------------------------------------------------------------------

def lists(*rows):
    """rows: (area, {b: pixels}) per a"""
    return lk.Overlaps.from_lists([(sorted(d), [d[k] for k in sorted(d)], area, 0, 0) for area, d in rows])


def test_link_tie_in_iou_goes_to_the_smaller_pair():
    ov = lists((10, {1: 5, 2: 5}), (10, {1: 5, 2: 5}))
    got = lk.link(ov, [10, 10], min_iou=0.3, min_child=None)
    assert got.parent.tolist() == [1, 2] and got.successor.tolist() == [1, 2] and got.linked.all() and not got.divided.any()
    one = lk.link(lists((10, {1: 5}), (10, {1: 5})), [10], min_child=None)
    assert one.parent.tolist() == [1] and one.successor.tolist() == [1, 0]


def test_link_threshold_exactly_met():
    ov = lists((2, {1: 1}))                                           # 1 / (2 + 1 - 1) = 0.5 exactly
    assert lk.link(ov, [1], min_iou=0.5, min_child=None).parent.tolist() == [1]
    assert lk.link(ov, [1], min_iou=float(np.nextafter(0.5, 1)), min_child=None).parent.tolist() == [0]
    child = lists((100, {1: 5}))                                      # 5 / 10 = 0.5 of the child exactly; iou 5 / 105
    assert lk.link(child, [10], min_iou=0.3, min_child=0.5).parent.tolist() == [1]
    assert lk.link(child, [10], min_iou=0.3, min_child=float(np.nextafter(0.5, 1))).parent.tolist() == [0]


def test_link_division_and_birth():
    ov = lists((100, {1: 60, 2: 40, 3: 10}), (50, {3: 12, 4: 12}), (50, {4: 12}))
    got = lk.link(ov, [60, 40, 40, 24])
    assert got.parent.tolist() == [1, 1, 0, 2]                        # 1 linked (iou 0.6); 2 a child (40 / 40); 3 a birth (12 / 40 < 0.5);
    assert got.linked.tolist() == [True, False, False, False]         # 4 a child of 2, not 3: equal pixels go to the smaller a
    assert got.divided.tolist() == [True, False, False] and got.successor.tolist() == [0, 4, 0]
    off = lk.link(ov, [60, 40, 40, 24], min_child=None)
    assert off.parent.tolist() == [1, 0, 0, 0] and off.successor.tolist() == [1, 0, 0] and not off.divided.any()
    parent, children = lc.link_rule(ov.pairs(), ov.area, [60, 40, 40, 24], 0.3, 0.5)
    assert parent.tolist() == got.parent.tolist() and (children >= 2).tolist() == got.divided.tolist()


def test_relate_on_nested_rectangles():
    parents = np.zeros((40, 60), np.int32)
    parents[2:30, 2:28], parents[2:30, 30:58] = 1, 2
    children = np.zeros((40, 60), np.int32)
    children[5:10, 5:10] = 1                                          # inside parent 1
    children[12:16, 26:32] = 2                                        # 8 pixels in each parent, 8 between them: the smaller parent
    children[20:24, 40:50] = 3                                        # inside parent 2
    children[32:38, 5:10] = 4                                         # in no parent
    children[26:34, 50:54] = 5                                        # half inside parent 2
    got = lk.relate_host(children, parents, 6, 2)
    assert got.parent.tolist() == [1, 1, 2, 0, 2, 0] and got.fraction.tolist() == [1.0, 8 / 24, 1.0, 0.0, 0.5, 0.0]
    assert got.children.tolist() == [2, 2]
    with pytest.raises(E):
        lk.relate_host(children, parents, 6, 1)


# ---- tracks -----------------------------------------------------------------------------------------------------------------------------

def test_track_host_on_the_sequence():
    stack, counts = lc.sequence()
    tr = lk.track_host(stack, counts)
    assert tr.table.tolist() == [[1, 0, 4, 0, 5],                     # the mover lives through all frames
                                 [2, 0, 1, 0, 2],                     # (70, 100) dies after frame 1
                                 [3, 0, 1, 0, 2],                     # (48, 40) ends at frame 1: it divides
                                 [4, 0, 2, 0, 3],                     # the corner disc dies after frame 2
                                 [5, 2, 4, 3, 3], [6, 2, 4, 3, 3],    # the two daughters, parent track 3
                                 [7, 3, 4, 0, 2]]                     # (80, 30) is born in frame 3
    assert len(tr) == 7 and tr.lineage() == [[1], [2], [3], [4], [3, 5], [3, 6], [7]]
    assert [t.tolist() for t in tr.track_of] == [[0, 1, 2, 3, 4], [0, 1, 2, 3, 4], [0, 1, 5, 6, 4], [0, 1, 5, 6, 7], [0, 1, 5, 6, 7]]
    assert tr.labels.dtype == np.int32 and all(np.array_equal(tr.labels[t], tr.track_of[t][stack[t]]) for t in range(5))
    # the rule restated in NumPy at the defaults, pair by pair
    ov = lk.overlaps_host(stack, stack, counts, pairs=[(t, t + 1) for t in range(4)])
    ious = []
    for t in range(4):
        o, area = ov.slice(4 * t, 4 * t + 4), lc.boxes_of(stack[t + 1], 4)[:, 0]
        got = lk.link(o, area)
        parent, children = lc.link_rule(o.pairs(), o.area, area, 0.3, 0.5)
        assert got.parent.tolist() == parent.tolist() and got.divided.tolist() == (children >= 2).tolist()
        iou = o.iou(area)
        ious += iou[got.linked[o.values - 1] & (got.parent[o.values - 1] == o.rows() + 1)].tolist()
        if t == 1:
            d = iou[(o.rows() == 2)]
            assert np.round(d, 3).tolist() == [0.241, 0.241] and (d < 0.3).all()            # both daughters miss min_iou ...
            assert got.parent.tolist() == [1, 3, 3, 4] and got.linked.tolist() == [True, False, False, True]       # ... the child rule takes them
            assert got.divided.tolist() == [False, False, True, False]
    assert len(ious) == 13 and round(min(ious), 2) == 0.60 and round(max(ious), 2) == 0.86           # 0.6 and 0.8603 to two places
    # a drift vector: every frame displaced by what the mover does keeps the mover's overlap whole
    moved = lk.overlaps_host(stack, stack, counts, pairs=[(0, 1)], shift=(1, 3))
    assert moved.of(0)[1].tolist() == [int(moved.area[0])]


def test_stitch_planes_and_single_frames():
    stack, counts = lc.sequence()
    vol = lk.stitch_planes(stack, counts, min_iou=0.25)
    assert len(vol) == 7 and not vol.table[:, 3].any()                # no child rule: the daughters and nothing else start without a parent
    assert vol.track_of[2].tolist() == [0, 1, 5, 6, 4]
    one = lk.track_host(stack[:1], counts[:1])
    assert one.table.tolist() == [[k, 0, 0, 0, 1] for k in (1, 2, 3, 4)] and np.array_equal(one.labels, stack[:1])
    gap = stack.copy()
    gap[1][gap[1] == 2] = 0                                           # an id without pixels has no track
    tr = lk.track_host(gap, counts)
    assert tr.track_of[1].tolist() == [0, 1, 0, 3, 4] and tr.table[1].tolist() == [2, 0, 0, 0, 1]
