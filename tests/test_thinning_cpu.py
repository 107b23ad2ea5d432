"""CPU: the host statement of the thinning semantics (thinning.thin_host / midlines_host: the rule by shifted comparisons with integer
sums) against a per-pixel Python loop of the rule as the header writes it, the observations that pin the order of the sub-iterations,
and the properties that make the result a midline: the 8-connected components and the 4-connected background components are kept, the
result is a subset and a fixed point.  Every comparison is exact integer equality, lengths() against closed forms at rtol 1e-12."""
import inspect

import numpy as np
import pytest

import thinning_cases as tc
from kg_instance_segmentation_amd import _lib, components, inference, instances, labelmetrics, tiling
from kg_instance_segmentation_amd import thinning as th

E = _lib.KGLibraryError
I32 = np.iinfo(np.int32)


def fg_bg(masks):
    """bool [n, h, w] -> (8-connected components, 4-connected background components) per mask, by components_host.  Everything outside
    the array is background, as the semantics say, so the mask is counted inside a one-pixel frame of background."""
    m = np.pad(np.asarray(masks, bool), ((0, 0), (1, 1), (1, 1))).astype(np.int32)
    fg = components.components_host(m, 8, 0)[1]
    both = components.components_host(m, 8, 4)[1]
    return np.asarray(fg, np.int64).reshape(-1), (np.asarray(both, np.int64) - fg).reshape(-1)


def fg_bg_scipy(mask):
    ndi = pytest.importorskip("scipy.ndimage")
    mask = np.pad(mask, 1)
    return ndi.label(mask, np.ones((3, 3), int))[1], ndi.label(~mask)[1]


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 1, 2])
def test_thin_host_equals_the_per_pixel_loop_on_ragged_blobs(seed):
    lab = tc.blobs(44, 57, 5, 20 + seed, 2, 8)
    for k in range(1, 6):
        P = lab == k
        want, passes = tc.thin_plain(P)
        got, gp = th.thin_host(P)
        assert got.dtype == bool and np.array_equal(got, want) and gp == passes
        for limit in (1, 2):
            want, passes = tc.thin_plain(P, limit)
            got, gp = th.thin_host(P, limit)
            assert np.array_equal(got, want) and gp == passes <= limit
    stack = np.stack([lab == k for k in range(1, 6)])
    S, passes = th.thin_host(stack)                                     # a stack: every array on its own
    assert passes.dtype == np.int64 and passes.shape == (5,)
    for k in range(5):
        one, p = th.thin_host(stack[k])
        assert np.array_equal(S[k], one) and passes[k] == p
    assert np.array_equal(th.thin_host(stack.astype(np.uint8))[0], S)


def test_deletable_equals_the_per_pixel_rule_on_every_neighbourhood():
    v = np.arange(512)
    m = ((v[:, None] >> np.arange(9)) & 1).astype(bool).reshape(-1, 3, 3)
    for second in (False, True):
        got = th.deletable(m, second)
        want = np.array([[[tc.deletable_plain(a, y, x, second) for x in range(3)] for y in range(3)] for a in m])
        assert np.array_equal(got, want)


def test_the_pinned_observations():
    S, p = th.thin_host(np.ones((2, 2), bool))
    assert S.tolist() == [[False, True], [False, False]] and p == 1
    S, p = th.thin_host(np.ones((7, 54), bool))
    want = np.zeros((7, 54), bool)
    want[3, 3:51] = True
    assert np.array_equal(S, want) and S.sum() == 48 and p == 3
    S, p = th.thin_host(tc.disc(18))
    assert S.sum() == 3 and p == 18
    S, p = th.thin_host(tc.checkerboard())
    assert np.array_equal(S, tc.checkerboard()) and p == 0
    S, p = th.thin_host(tc.annulus())
    c = th.count_host(S)
    assert p == 3 and fg_bg(S[None]) == (1, 2) and c[1] == c[2] == c[3] == 0 and c[4] + c[5] == c[0]      # one closed ring: as many edges as pixels


def test_the_pinned_example_row():
    lab, S, row = tc.pinned_example()
    skel, mid = th.midlines_host(lab, 1)
    assert skel.dtype == np.int32 and np.array_equal(skel, S.astype(np.int32)) and mid.rows.tolist() == [row] and mid.skel is skel
    assert mid.rows.dtype == np.int64 and th.ROW_COLUMNS == ("members", "pixels", "isolated", "ends", "junctions", "ortho", "diag", "passes", "status")
    assert mid.pixels().tolist() == [23] and mid.ends().tolist() == [3] and mid.junctions().tolist() == [1] and mid.isolated().tolist() == [0]
    assert mid.passes().tolist() == [2] and mid.members().tolist() == [78]
    np.testing.assert_allclose(mid.lengths(), [20 + 2 * np.sqrt(2.0)], rtol=1e-12)
    pr = mid.props()
    np.testing.assert_allclose(pr["thinness"], [23 / 78], rtol=1e-12)
    np.testing.assert_allclose(pr["length"], mid.lengths(), rtol=1e-12)
    assert pr["ends"].tolist() == [3.0] and pr["junctions"].tolist() == [1.0]
    # closed forms: a straight bar's midline is a row of 48 pixels, a diagonal line of n pixels has n - 1 diagonal edges
    _, bar = th.midlines_host(np.ones((7, 54), np.int32), 1)
    np.testing.assert_allclose(bar.lengths(), [47.0], rtol=1e-12)
    _, dia = th.midlines_host(np.eye(30, dtype=np.int32), 1)
    assert dia.rows[0].tolist() == [30, 30, 0, 2, 0, 0, 29, 0, 0]
    np.testing.assert_allclose(dia.lengths(), [29 * np.sqrt(2.0)], rtol=1e-12)
    empty = th.Midlines(np.zeros((2, 9), np.int64))
    assert np.isnan(empty.props()["thinness"]).all() and empty.lengths().tolist() == [0.0, 0.0] and len(empty) == 2


# ---- what makes it a midline ----------------------------------------------------------------------------------------------------------------

def check_topology(masks, limit=None):
    S, passes = th.thin_host(masks, limit)
    assert not (S & ~masks).any()                                       # a subset
    fg0, bg0 = fg_bg(masks)
    uniq, back = np.unique(S.reshape(len(S), -1), axis=0, return_inverse=True)      # many masks share a result: count each once
    fg1, bg1 = fg_bg(uniq.reshape((-1,) + S.shape[1:]))
    assert np.array_equal(fg0, fg1[back.reshape(-1)]) and np.array_equal(bg0, bg1[back.reshape(-1)])
    return S, passes


def test_all_masks_of_4_by_4():
    v = np.arange(65536)
    masks = ((v[:, None] >> np.arange(16)) & 1).astype(bool).reshape(-1, 4, 4)
    S, passes = check_topology(masks)
    again, p2 = th.thin_host(S)
    assert np.array_equal(again, S) and not p2.any()                    # a fixed point
    assert not th.deletable(S, False).any() and not th.deletable(S, True).any()
    assert (passes > 0).any() and passes.max() <= 2
    for k in range(0, 65536, 257):                                      # scipy on a stride of them, where it imports
        assert fg_bg_scipy(masks[k]) == fg_bg_scipy(S[k])


def test_bernoulli_masks_of_9_by_9():
    rng = np.random.default_rng(5)
    masks = rng.random((3000, 9, 9)) < 0.6
    S, passes = check_topology(masks)
    assert np.array_equal(th.thin_host(S)[0], S) and not th.deletable(S, False).any() and not th.deletable(S, True).any()
    for k in (1, 2):
        Sk, pk = check_topology(masks, k)                               # k passes keep the topology as well
        assert (pk <= k).all() and np.array_equal(pk, np.minimum(passes, k)) and not (S & ~Sk).any()
    for k in range(0, 3000, 100):
        assert fg_bg_scipy(masks[k]) == fg_bg_scipy(S[k])
        want, p = tc.thin_plain(masks[k], 1)
        assert np.array_equal(th.thin_host(masks[k], 1)[0], want)


def test_max_passes_is_k_passes_of_the_loop():
    P = tc.disc(9) | np.roll(tc.disc(9), 7, 1)
    full, total = th.thin_host(P)
    for k in range(1, total + 2):
        want, p = tc.thin_plain(P, k)
        got, gp = th.thin_host(P, k)
        assert np.array_equal(got, want) and gp == p == min(k, total)
        assert fg_bg(got[None]) == fg_bg(P[None])
    assert np.array_equal(th.thin_host(P, 0)[0], full) and np.array_equal(th.thin_host(P, None)[0], full)


# ---- the row ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["comb", "rings", "blobs", "noise", "serpentine"])
def test_row_counts_equal_per_pixel_loops(shape):
    rng = np.random.default_rng(3)
    P = {"comb": tc.comb(), "rings": tc.nested_rings(), "blobs": tc.blobs(50, 60, 6, 4) > 0, "noise": rng.random((40, 45)) < 0.6,
         "serpentine": tc.serpentine(23)}[shape]
    for m in (P, th.thin_host(P)[0], th.thin_host(P, 1)[0]):
        c = th.count_host(m)
        assert c.tolist() == tc.counts_plain(m)
        assert tc.degree_sum(m) == 2 * (c[4] + tc.all_diagonal_pairs(m))
    S = th.thin_host(P)[0]
    c = th.count_host(S)
    assert c[5] <= tc.all_diagonal_pairs(S)
    if shape == "comb":
        assert c[2] >= 9 and c[3] >= 7                                  # nine teeth end in a tip each, and branch off the back
    if shape == "serpentine":
        assert c[2] == 2 and c[3] == 0 and c[4] + c[5] == c[0] - 1      # a path stays a path: two tips, one edge fewer than pixels


# ---- jobs ---------------------------------------------------------------------------------------------------------------------------------

def test_midlines_host_over_jobs():
    n = 6
    lab = tc.blobs(70, 90, n, 11)
    stats = tc.stats_of(lab, n)
    assert np.array_equal(labelmetrics.label_stats_host(lab, n), stats)
    skel, mid = th.midlines_host(lab, n)
    assert len(mid) == n and skel.shape == lab.shape
    want = np.zeros_like(lab)
    for k in range(n):
        S, p = tc.thin_plain(lab == k + 1)
        want[S] = k + 1
        assert mid.rows[k].tolist() == [stats[k, 0], *tc.counts_plain(S), p, 0]
    assert np.array_equal(skel, want) and not (skel[skel > 0] != lab[skel > 0]).any()
    jobs = np.concatenate([np.zeros((n, 1), np.int64), np.arange(1, n + 1)[:, None], stats[:, 1:]], 1)
    s2, m2 = th.midlines_host(lab, jobs)
    assert np.array_equal(s2, skel) and m2 == mid
    s3, m3 = th.midlines_host(np.stack([lab, lab[::-1]]), [n, n], 2)    # a stack, two passes
    assert np.array_equal(s3[0], th.midlines_host(lab, n, 2)[0]) and np.array_equal(m3.rows[:n], th.midlines_host(lab, n, 2)[1].rows)
    assert len(m3) == 2 * n and (m3.rows[:, 7] <= 2).all()
    s4, m4 = th.midlines_host(lab, [])
    assert len(m4) == 0 and m4.rows.shape == (0, 9) and not s4.any() and s4.shape == lab.shape
    # it is a label map: the family works on it
    assert np.array_equal(labelmetrics.label_stats_host(skel, n)[:, 0], mid.pixels())


def test_boxes_that_cut_and_bad_jobs():
    lab = np.zeros((30, 40), np.int32)
    lab[5:25, 4:36] = 7
    jobs = np.array([[0, 7, 0, 0, 30, 40], [0, 7, 5, 4, 15, 20], [0, 7, -9, -9, 15, 20], [0, 7, 10, 10, I32.max, I32.max], [1, 7, 0, 0, 30, 40],
                     [-1, 7, 0, 0, 30, 40], [0, 7, 20, 20, 20, 30], [0, 7, 25, 30, 5, 4], [0, 8, 0, 0, 30, 40]], np.int64)
    skel, mid = th.midlines_host(lab, jobs)
    whole, p0 = th.thin_host(lab == 7)
    cut, p = th.thin_host(lab[5:15, 4:20] == 7)                         # outside the box is background: the cut part is thinned
    assert mid.rows[0].tolist() == [640, *th.count_host(whole), p0, 0] and p0 > 0
    assert mid.rows[1].tolist() == [160, *th.count_host(cut), p, 0] and np.array_equal(mid.rows[2], mid.rows[1])
    assert mid.rows[3, 0] == 15 * 26 and not mid.rows[4:].any()
    one = th.midlines_host(lab, jobs[1:2])[0]
    assert np.array_equal(one[5:15, 4:20], cut * 7) and one.sum() == 7 * cut.sum()
    union = whole.copy()                                                # jobs of one id store the union of their results
    union[5:15, 4:20] |= cut
    union[10:25, 10:36] |= th.thin_host(lab[10:, 10:] == 7)[0][:15, :26]
    assert np.array_equal(skel, union * 7)
    for v in (0, -1, I32.min, I32.max):                                 # any int32 is an id
        l2 = np.where(lab == 7, v, 3).astype(np.int32)
        s2, m2 = th.midlines_host(l2, [[0, v, 0, 0, 30, 40]])
        assert np.array_equal(m2.rows, mid.rows[:1]) and np.array_equal(s2 == v, whole if v else np.ones_like(whole))


def test_fits_on_both_sides_of_its_rule():
    for h, w, ok in ((126, 126, True), (254, 510, True), (255, 510, False), (254, 511, False), (4094, 30, True), (4095, 30, False),
                     (4094, 31, False), (1, 1, True), (1, 32768, True), (2, 32768, False), (2046, 62, True), (2046, 63, False)):
        assert th.fits(h, w) is ok and ((h + 2) * -(-(w + 2) // 32) <= 4096) is ok
    assert th.MAX_WORDS == 4096


def test_refusals():
    lab = np.ones((4, 5), np.int32)
    for bad in (-1, 1.5, True, "2", 2 ** 31):
        with pytest.raises(E):
            th.thin_host(lab > 0, bad)
        with pytest.raises(E):
            th.midlines_host(lab, 1, bad)
    for bad in (np.ones(4, bool), np.ones((2, 2, 2, 2), bool), np.ones((3, 3), np.float32)):
        with pytest.raises(E):
            th.thin_host(bad)
    with pytest.raises(E):
        th.midlines_host(lab.astype(np.float32), 1)
    with pytest.raises(E):
        th.midlines_host(lab, np.zeros((1, 5), np.int64))
    with pytest.raises(E):
        th.midlines_host(lab, [[0, 2 ** 31, 0, 0, 1, 1]])
    with pytest.raises(E):
        th.midlines_host(lab, [1, 1])
    with pytest.raises(E):                                              # the device functions refuse a host map and name the host route
        th.thin(lab, 1)
    with pytest.raises(E):
        th.thin_rows(lab, np.zeros((0, 6), np.int64))
    with pytest.raises(E):
        th.thin_instances("no instances")


def test_instances_and_options():
    n = 4
    lab = tc.blobs(50, 60, n, 2)
    stats = tc.stats_of(lab, n)
    dets = np.concatenate([stats[:, 1:].astype(np.float32), np.ones((n, 1), np.float32)], 1)
    table = tiling.table_from_labels_host(lab, np.concatenate([np.arange(1, n + 1)[:, None], stats[:, 1:]], 1), stats[:, 0])
    inst = instances.Instances(lab, dets, table, None)
    assert inst.midlines is None and "midlines" in instances.Instances.__slots__
    mid = th.thin_instances(inst)                                       # a host label map goes through midlines_host
    skel, want = th.midlines_host(lab, n)
    assert mid == want and np.array_equal(mid.skel, skel)
    out = th.thin_instances_batch([inst, None], max_passes=1)
    assert out[0] is inst and inst.midlines == th.midlines_host(lab, n, 1)[1] and out[1] is None
    for fn in (inference.predict_instances, tiling.predict_tiled):
        assert inspect.signature(fn).parameters["thin"].default is None
