"""CPU: the host statement of the nearest-other-label transform (distance.py) against a per-pixel loop written here, scipy where it is
installed, and closed forms; the tie rule spelled out; the registration of csrc/distance.hip; the refusals with their messages."""
import math
import os
import re

import numpy as np
import pytest

from kg_instance_segmentation_amd import _lib, build, instances, tiling
from kg_instance_segmentation_amd import distance as dt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32 = np.iinfo(np.int32)


def loop_transform(lab, max_d2, frame):
    """The definition, pixel by pixel, pair by pair."""
    H, W = lab.shape
    d2 = np.zeros((H, W), np.int64)
    near = np.zeros((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            v = int(lab[y, x])
            best = None
            for qy in range(H):
                for qx in range(W):
                    u, d = int(lab[qy, qx]), (qy - y) ** 2 + (qx - x) ** 2
                    if u != v and d <= max_d2 and (best is None or (d, u) < best):
                        best = (d, u)
            d2[y, x], near[y, x] = best if best is not None else (max_d2 + 1, v)
            f = min(y + 1, x + 1, H - y, W - x)
            if frame and f * f <= max_d2:
                d2[y, x] = min(d2[y, x], f * f)
    return d2, near


@pytest.mark.parametrize("frame", [False, True])
@pytest.mark.parametrize("max_d2", [1, 2, 4, 5, 9, 49])
def test_host_statement_equals_the_pixel_loop(max_d2, frame):
    rng = np.random.default_rng(100 + max_d2)
    for H, W in ((1, 1), (1, 9), (8, 1), (5, 13), (13, 13), (9, 4)):
        lab = rng.integers(-1, 5, (H, W))
        if H * W > 20:
            lab[rng.random((H, W)) < 0.6] = 0                          # long runs, so that large radii matter
        d2, near = dt.distance_host(lab, max_d2, frame)
        wd, wn = loop_transform(lab, max_d2, frame)
        assert d2.dtype == near.dtype == np.int32 and d2.shape == (H, W)
        assert np.array_equal(d2, wd) and np.array_equal(near, wn), (H, W)
    stack = rng.integers(-1, 5, (3, 6, 7))                             # a stacked image never sees its neighbours
    d2, near = dt.distance_host(stack, max_d2, frame)
    for i in range(3):
        one = dt.distance_host(stack[i], max_d2, frame)
        assert np.array_equal(d2[i], one[0]) and np.array_equal(near[i], one[1])


def sparse_sources(H, W, share, nid, seed):
    rng = np.random.default_rng(seed)
    lab = np.zeros((H, W), np.int32)
    sel = rng.random((H, W)) < share
    lab[sel] = rng.integers(1, nid + 1, int(sel.sum()))
    return lab


def test_d2_of_the_background_equals_scipy_edt():
    ndi = pytest.importorskip("scipy.ndimage")
    lab = sparse_sources(60, 75, 0.004, 8, 3)
    for max_d2 in (9, 49, 100):
        d2, _ = dt.distance_host(lab, max_d2)
        edt = ndi.distance_transform_edt(lab == 0)
        want = np.minimum(np.rint(edt ** 2).astype(np.int64), max_d2 + 1)
        assert np.array_equal(d2[lab == 0], want[lab == 0])
        assert (want[lab == 0] == max_d2 + 1).any() and (want[lab == 0] <= max_d2).any()


def test_expand_labels_equals_scipy_where_the_nearest_value_is_unique():
    ndi = pytest.importorskip("scipy.ndimage")
    lab, dist = sparse_sources(40, 50, 0.05, 8, 1), 6
    got = dt.expand_labels_host(lab, dist)
    edt, idx = ndi.distance_transform_edt(lab == 0, return_indices=True)
    theirs = np.where(edt <= dist, lab[idx[0], idx[1]], 0)
    # the pixels whose nearest source value is unique, computed here from all pixel-source pairs
    sy, sx = np.nonzero(lab)
    yy, xx = np.mgrid[0:40, 0:50]
    pair = (yy[..., None] - sy) ** 2 + (xx[..., None] - sx) ** 2       # [H, W, sources]
    at_min = pair == pair.min(2, keepdims=True)
    vals = np.where(at_min, lab[sy, sx], 0)
    unique = np.where(at_min, lab[sy, sx], 99).min(2) == vals.max(2)
    expanded = (lab == 0) & (pair.min(2) <= dist * dist)
    assert np.array_equal(expanded, (got != 0) & (lab == 0))
    share = np.count_nonzero(unique & expanded) / np.count_nonzero(expanded)
    print("share of expanded pixels with a unique nearest value", share)
    assert share >= 0.8
    assert np.array_equal(got[unique], theirs[unique])
    assert np.array_equal(got[lab != 0], lab[lab != 0])
    # and on the rest the tie rule holds: the smallest of the equally near values
    assert np.array_equal(got[expanded], np.where(at_min, lab[sy, sx], 99).min(2)[expanded])


def test_tie_rule():
    def centre(lab, max_d2=2):
        d2, near = dt.distance_host(np.array(lab, np.int64), max_d2)
        return int(d2[len(lab) // 2, len(lab[0]) // 2]), int(near[len(lab) // 2, len(lab[0]) // 2])
    assert centre([[5, 0, 3]]) == (1, 3) and centre([[3, 0, 5]]) == (1, 3)                      # horizontally
    assert centre([[5, 0, -2]]) == (1, -2) and centre([[I32.max, 0, I32.min]]) == (1, I32.min)
    assert centre([[5], [0], [3]]) == (1, 3) and centre([[3], [0], [5]]) == (1, 3)              # above and below in one column
    assert centre([[-7], [0], [I32.max]]) == (1, -7) and centre([[I32.min], [0], [-1]]) == (1, I32.min)
    assert centre([[7, 0, 0], [0, 0, 0], [0, 0, 4]]) == (2, 4)                                     # diagonally
    assert centre([[0, 0, I32.max], [0, 0, 0], [-3, 0, 0]]) == (2, -3)
    assert centre([[0, 0, I32.min], [0, 0, 0], [-3, 0, I32.max]]) == (2, I32.min)
    assert centre([[7, 0, 0], [0, 0, 0], [0, 0, 4]], 1) == (2, 0)                                  # out of reach: saturated, its own value
    assert centre([[9, 0, 0], [0, 0, 3], [0, 0, 0]]) == (1, 3)                                     # the nearer one wins whatever its value
    # a non-zero pixel sees the background as a value like any other, and the smaller of two neighbours
    d2, near = dt.distance_host(np.array([[5, 0, 3], [-1, 5, 5]]), 1)
    assert near.tolist() == [[-1, 3, 0], [5, -1, 3]] and d2.tolist() == [[1, 1, 1], [1, 1, 1]]


def test_ring_is_the_difference_of_two_expansions():
    lab = sparse_sources(30, 41, 0.02, 6, 5)
    lab[10:14, 20:27] = 9
    for a, b in ((0, 3), (2, 5), (1.5, 4.2), (3, 3.1)):
        ring = dt.ring_labels_host(lab, a, b)
        outer = dt.expand_labels_host(lab, b)
        inner = dt.expand_labels_host(lab, a) if a * a >= 1 else lab
        want = np.where((lab == 0) & (inner == 0), outer, 0)
        assert np.array_equal(ring, want) and not ring[lab != 0].any()
        assert ring.any() == (math.floor(b * b) > math.floor(a * a))   # 3 .. 3.1: an empty ring


def test_shrink_rectangles_closed_form():
    H, W = 24, 31
    lab = np.zeros((H, W), np.int32)
    lab[3:15, 4:20] = 3                                                # away from the frame
    lab[16:24, 22:31] = 5                                              # in the bottom right corner
    for dist, cut in ((1, 1), (1.5, 1), (2, 2), (3.99, 3), (5, 5)):
        want = np.zeros_like(lab)
        want[3 + cut:15 - cut, 4 + cut:20 - cut] = 3
        plain, framed = want.copy(), want.copy()
        plain[16 + cut:24, 22 + cut:31] = 5                            # without frame the image's sides do not shrink it
        framed[16 + cut:24 - cut, 22 + cut:31 - cut] = 5
        assert np.array_equal(dt.shrink_labels_host(lab, dist), plain)
        assert np.array_equal(dt.shrink_labels_host(lab, dist, frame=True), framed)


def test_inscribed_closed_forms():
    H, W = 30, 40
    lab = np.zeros((H, W), np.int32)
    lab[2:8, 3:14] = 1                                                 # 6 x 11: radius 3, first attained at (2 + 2, 3 + 2)
    lab[10:19, 5:14] = 2                                               # a 9 x 9 ring of thickness 3: the centroid lies in the hole
    lab[13:16, 8:11] = 0
    lab[25, 30] = 3                                                    # a single pixel
    lab[20:30, 0:7] = 4                                                # 10 x 7 in the corner
    r = dt.inscribed_host(lab, 5, max_d2=49, frame=False)
    assert r.dtype == dt.INSCRIBED_DTYPE and len(r) == 5
    assert r[["d2max", "y", "x", "count"]].tolist() == [(9, 4, 5, 66), (4, 11, 6, 72), (1, 25, 30, 1), (49, 26, 0, 70), (0, -1, -1, 0)]
    assert r["radius"].tolist() == [3.0, 2.0, 1.0, 7.0, 0.0] and not r["saturated"].any()
    assert lab[r["y"][1], r["x"][1]] == 2 and lab[14, 9] == 0        # inside the ring, which its centroid (14, 9) is not
    f = dt.inscribed_host(lab, 5, max_d2=49, frame=True)
    assert f[["d2max", "y", "x", "count"]].tolist()[3] == (16, 23, 3, 70) and np.array_equal(f[:3], r[:3])
    s = dt.inscribed_host(lab, jobs=[[0, 1, 0, 0, H, W], [0, 1, 0, 0, 4, W], [0, 0, 0, 0, H, W], [1, 1, 0, 0, H, W]], max_d2=4, frame=False)
    assert s[["d2max", "y", "x", "count", "saturated"]].tolist()[:2] == [(5, 4, 5, 66, True), (4, 3, 4, 22, False)]
    assert s["saturated"][2] and s["count"][2] == np.count_nonzero(lab == 0) and s[3]["count"] == 0 and s[3]["y"] == -1
    # the rows are not additive over bands: largest d2max, then the smallest index, counts added
    rows = np.array([[4, 3, 9, 10], [9, 5, 1, 7], [9, 4, 30, 2], [0, -1, -1, 0], [0, -1, -1, 0], [2, 0, 0, 1]])
    got = dt.combine_bands(rows, [0, 0, 0, 1, 1, 2], 4, W)
    assert got.tolist() == [[9, 4, 30, 19], [0, -1, -1, 0], [2, 0, 0, 1], [0, -1, -1, 0]]


def test_expand_instances_on_a_host_map():
    lab = np.zeros((20, 30), np.int32)
    lab[5:8, 5:9], lab[5:8, 12:15] = 1, 3                              # id 2 has no visible pixel
    table = np.concatenate([tiling.table_from_labels_host(lab, [[1, 5, 5, 8, 9]]), np.zeros((1, 8), np.int64),
                            tiling.table_from_labels_host(lab, [[3, 5, 12, 8, 15]])])
    table[:, 0] = [12, 40, 9]
    inst = instances.Instances(lab, np.zeros((3, 5), np.float32), table, None)
    got = dt.expand_instances(inst, 2.5)
    want = dt.expand_labels_host(lab, 2.5)
    assert type(got) is instances.Instances and np.array_equal(got.labels, want) and got.dets is inst.dets and got.measurements is None
    assert np.array_equal(got.table[[0, 2]], tiling.table_from_labels_host(want, [[1, 0, 0, 20, 30], [3, 0, 0, 20, 30]], [12, 9]))
    assert got.table[1].tolist() == [40, 0, 0, 0, 0, 0, 0, 0] and got.table[0, 1] > 12
    assert want[6, 10] == 1 and want[6, 11] == 3 and np.array_equal(inst.labels, lab)             # they met and did not merge
    assert dt.expand_instances_batch([None, inst], 1)[0] is None


def test_registration():
    assert "distance.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "distance.hip"))
    header = open(os.path.join(ROOT, "include", "kgnet_hip.h")).read()
    for name in ("kg_label_distance", "kg_label_regrow", "kg_label_inscribed"):
        assert name in _lib._SIGS and re.search(r"\bint " + name + r"\(", header), name
    src = open(os.path.join(build.CSRC, "distance.hip")).read()
    assert int(re.search(r"#define KG_DT_TH (\d+)", src).group(1)) == dt.TILE_H
    assert int(re.search(r"#define KG_DT_TW (\d+)", src).group(1)) == dt.TILE_W


def test_refusals():
    lab = np.zeros((4, 5), np.int32)
    for bad in (0, 4097, -1, 2.0, True):
        with pytest.raises(_lib.KGLibraryError, match=r"distance_host: max_d2 .* must be an integer in 1 \.\. 4096"):
            dt.distance_host(lab, bad)
    with pytest.raises(_lib.KGLibraryError, match=r"inscribed_host: max_d2 4097 must be an integer in 1 \.\. 4096"):
        dt.inscribed_host(lab, 1, max_d2=4097)
    for fn in (dt.expand_labels_host, dt.shrink_labels_host, dt.expand_labels, dt.shrink_labels):
        with pytest.raises(_lib.KGLibraryError, match=r"distance 64\.01 exceeds 64"):
            fn(lab, 64.01)
        with pytest.raises(_lib.KGLibraryError, match=r"distance 0\.5 must be at least 1"):
            fn(lab, 0.5)
    assert dt.expand_labels_host(lab, 64).shape == (4, 5) and dt.expand_labels_host(lab, 64.0).shape == (4, 5)
    for fn in (dt.ring_labels_host, dt.ring_labels):
        for inner, outer in ((3, 3), (4, 2), (-1, 2)):
            with pytest.raises(_lib.KGLibraryError, match=r"need 0 <= inner < outer"):
                fn(lab, inner, outer)
        with pytest.raises(_lib.KGLibraryError, match=r"distance 65 exceeds 64"):
            fn(lab, 2, 65)
    with pytest.raises(_lib.KGLibraryError, match=r"want \('d2', 'both'\) must name"):
        dt.distance(lab, 4, want=("d2", "both"))
    with pytest.raises(_lib.KGLibraryError, match=r"distance \(MI355X build\) needs the label maps on a GPU device; the host route is distance_host"):
        dt.distance(lab, 4)
    for fn, args in ((dt.expand_labels, (2,)), (dt.ring_labels, (1, 2)), (dt.shrink_labels, (2,)), (dt.inscribed, (1,))):
        with pytest.raises(_lib.KGLibraryError, match=fn.__name__ + r" \(MI355X build\) needs the label maps on a GPU device"):
            fn(lab, *args)
    with pytest.raises(_lib.KGLibraryError, match=r"jobs cannot be given together with n"):
        dt.inscribed_host(lab, 1, jobs=[[0, 1, 0, 0, 4, 5]])
    with pytest.raises(_lib.KGLibraryError, match=r"expand_instances: an Instances or a TiledInstances"):
        dt.expand_instances(lab, 2)
