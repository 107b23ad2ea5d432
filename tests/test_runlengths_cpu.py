"""CPU: the host statements of the run-length semantics (runlengths.py) against instances.rle_encode / rle_decode / rle_string, which stay
the yardstick.  Every comparison is exact integer equality."""
import numpy as np
import pytest

from kg_instance_segmentation_amd import _lib, instances
from kg_instance_segmentation_amd import measure as ms
from kg_instance_segmentation_amd import runlengths as rl

E = _lib.KGLibraryError


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


def wrap_map():
    """The 4 x 3 map with id 5 at p = 2, 3, 4, 5, 7, 8: its first run continues from the bottom of column 0 into the top of column 1"""
    flat = np.zeros(12, np.int32)
    flat[[2, 3, 4, 5, 7, 8]] = 5
    return np.ascontiguousarray(flat.reshape(3, 4).T)


def full_jobs(lab, ids):
    H, W = lab.shape
    return np.array([[0, int(i), 0, 0, H, W] for i in ids], np.int64).reshape(-1, 6)


def same_as_rle_encode(lab, got, ids):
    want = instances.rle_encode(lab, ids=ids)
    assert len(got) == len(ids)
    for k, i in enumerate(ids):
        assert got.of(k).dtype == np.int64 and np.array_equal(got.of(k), want[int(i)]), (k, i)
        assert got.string(k) == instances.rle_string(want[int(i)])
    assert np.array_equal(got.areas(), [int((lab == i).sum()) for i in ids])


MAPS = [blob_map(23, 37, 9, 1), blob_map(70, 131, 40, 170), blob_map(1, 40, 5, 2), blob_map(40, 1, 5, 3), np.full((1, 1), 3, np.int32),
        np.zeros((1, 1), np.int32), np.full((6, 5), 2, np.int32), wrap_map()]


@pytest.mark.parametrize("k", range(len(MAPS)))
def test_runs_host_equals_rle_encode(k):
    lab = MAPS[k]
    ids = sorted(set(np.unique(lab).tolist()) - {0}) + [99]           # an absent id gets an empty list
    same_as_rle_encode(lab, rl.runs_host(lab, full_jobs(lab, ids)), ids)
    n = int(lab.max())
    got = rl.runs_host(lab, n)                                        # ids 1 .. n inside their own boxes
    same_as_rle_encode(lab, got, list(range(1, n + 1)))
    assert got.to_dict().keys() == instances.rle_encode(lab, ids=range(1, n + 1)).keys()
    assert got == rl.runs_host(lab[None], [n]) and got.slice(0, len(got)) == got
    assert len(rl.runs_host(lab, [])) == 0 and len(rl.runs_host(lab, np.zeros((0, 6), np.int64))) == 0      # no jobs, as a list or an array


def test_wrap_example_literals():
    lab = wrap_map()
    got = rl.runs_host(lab, full_jobs(lab, [5, 0]))
    assert got.string(0) == "3 4 8 2" == instances.rle_string(instances.rle_encode(lab)[5])
    assert got.first.tolist() == [2, 7, 0, 6, 9] and got.last.tolist() == [5, 8, 1, 6, 11] and got.counts().tolist() == [2, 3]
    assert got.coco(0) == {"size": [4, 3], "counts": [2, 4, 1, 2, 3]}
    assert got.coco(1) == {"size": [4, 3], "counts": [0, 2, 4, 1, 2, 3]}
    one = np.full((70, 131), 4, np.int32)                             # a map of one value is ONE run, whatever the columns
    got = rl.runs_host(one, 4)
    assert got.counts().tolist() == [0, 0, 0, 1] and got.of(3).tolist() == [[1, 70 * 131]] and got.coco(3)["counts"] == [0, 70 * 131]
    assert got.coco(0)["counts"] == [70 * 131]
    # a box sees the map around it: the band of columns 1 .. 2 holds no head and no tail of the single run
    assert rl.run_counts_host(one, [[0, 4, 0, 1, 70, 3], [0, 4, 0, 0, 70, 1], [0, 4, 0, 130, 70, 131], [0, 4, 5, 0, 9, 131]]).tolist() \
        == [[0, 0], [1, 0], [0, 1], [0, 0]]


def test_bands_concatenate_to_the_unsplit_result():
    rng = np.random.default_rng(7)
    maps = [blob_map(23, 37, 9, 1), np.where(rng.random((11, 11)) < 0.8, 1, rng.integers(0, 4, (11, 11))).astype(np.int32),
            np.ones((9, 14), np.int32)]
    for lab in maps:
        H, W = lab.shape
        n = int(lab.max())
        whole = np.concatenate([ms.jobs_from_stats(ms.labelmetrics.label_stats_host(lab, n)), [[0, 0, 0, 0, H, W], [0, 1, 0, 0, H, W]]]).astype(np.int64)
        want = rl.runs_host(lab, whole)
        assert want.slice(0, n) == rl.runs_host(lab, n)
        jobs = np.concatenate([whole, [[0, 1, 2, 3, H - 1, W - 2]]])                               # and a box that cuts runs: raw entries only
        flat = rl.run_counts_host(lab, jobs).astype(np.int64)
        assert np.array_equal(flat[:-1, 0], want.counts()) and np.array_equal(flat[:-1, 1], want.counts())
        unsplit = rl.run_rows_host(lab, np.concatenate([jobs, np.cumsum(flat, 0) - flat], 1), int(flat.sum(0).max()), fill=-9)
        assert np.array_equal(unsplit[:len(want.first), 0], want.first) and np.array_equal(unsplit[:len(want.last), 1], want.last)
        for cap in (1, H, 3 * H, 65536):                              # the whole-map jobs have h = H
            pieces, owner = rl.split_columns(jobs, cap)
            assert pieces.dtype == np.int32 and (np.diff(owner) >= 0).all() and set(owner.tolist()) == set(range(len(jobs)))
            ph, pw = pieces[:, 4] - pieces[:, 2], pieces[:, 5] - pieces[:, 3]
            cut = np.bincount(owner)[owner] > 1
            assert np.array_equal(pieces[:, [2, 4]], jobs[owner][:, [2, 4]])                     # every band has the box's full height
            assert (pw[cut] <= np.maximum(cap // ph[cut], 1)).all() and cut.any() == (cap < 65536)
            assert ((ph * pw <= cap) | (pw <= 1)).all()
            cnt = rl.run_counts_host(lab, pieces).astype(np.int64)
            per = np.zeros((len(jobs), 2), np.int64)
            np.add.at(per, owner, cnt)
            assert np.array_equal(per, flat)
            table = np.concatenate([pieces.astype(np.int64), np.cumsum(cnt, 0) - cnt], 1)
            assert np.array_equal(rl.run_rows_host(lab, table, len(unsplit), fill=-9), unsplit)
    lab = wrap_map()
    assert rl.run_counts_host(lab, [[0, 5, 0, 0, 3, 3]]).tolist() == [[1, 2]]                      # the box cuts both runs: heads at 2, tails at 5 and 8
    with pytest.raises(E):
        rl.runs_host(lab, [[0, 5, 0, 0, 3, 3]])
    # a head whose tail lies in a later band: heads and tails are offset separately
    one = np.ones((5, 6), np.int32)
    pieces, owner = rl.split_columns([[0, 1, 0, 0, 5, 6]], 10)
    assert pieces[:, 2:].tolist() == [[0, 0, 5, 2], [0, 2, 5, 4], [0, 4, 5, 6]] and owner.tolist() == [0, 0, 0]
    assert rl.run_counts_host(one, pieces).tolist() == [[1, 0], [0, 0], [0, 1]]


def test_run_rows_host_store_predicate():
    lab = wrap_map()
    job = [0, 5, 0, 0, 4, 3]
    assert rl.run_rows_host(lab, [job + [0, 0]], 2).tolist() == [[2, 5], [7, 8]]
    assert rl.run_rows_host(lab, [job + [1, -1]], 2, fill=-7).tolist() == [[-7, 8], [2, -7]]           # slots outside [0, R) are dropped
    assert rl.run_rows_host(lab, [job + [3, -5], [3, 5, 0, 0, 4, 3, 0, 0], [0, 5, 3, 0, 1, 3, 0, 0]], 3, fill=-7).tolist() == [[-7, -7]] * 3
    assert rl.run_rows_host(lab, np.zeros((0, 8), np.int64), 0).shape == (0, 2)
    with pytest.raises(E):
        rl.run_rows_host(lab, [job], 2)


def coco_loop(lab, v):
    counts, cur, c = [], 0, 0
    for p in (lab.T.reshape(-1) == v).astype(int).tolist():
        if p != cur:
            counts.append(c)
            c, cur = 0, p
        c += 1
    return counts + [c]


def test_coco_equals_a_per_pixel_loop():
    for lab in (blob_map(23, 37, 9, 1), wrap_map(), np.full((3, 2), 1, np.int32), np.eye(5, dtype=np.int32)):
        ids = list(range(0, int(lab.max()) + 2))
        got = rl.runs_host(lab, full_jobs(lab, ids))
        for k, v in enumerate(ids):
            c = got.coco(k)
            assert c["size"] == list(lab.shape) and c["counts"] == coco_loop(lab, v) and sum(c["counts"]) == lab.size
            assert all(isinstance(x, int) for x in c["counts"])


def test_paint_host_equals_rle_decode():
    for lab in (blob_map(23, 37, 9, 1), wrap_map(), np.zeros((4, 4), np.int32), np.full((1, 1), 6, np.int32)):
        H, W = lab.shape
        enc = instances.rle_encode(lab)
        want = instances.rle_decode(enc, H, W)
        assert np.array_equal(want, lab)
        got = rl.paint_host(enc, H, W)
        assert got.dtype == np.int32 and got.flags.c_contiguous and np.array_equal(got, want)
        n = int(lab.max())
        r = rl.runs_host(lab, n)
        assert np.array_equal(rl.paint_host(r, H, W), lab)
        assert np.array_equal(rl.paint_host(r, H, W, background=-3, ids=np.arange(n) + 50), np.where(lab > 0, lab + 49, -3))
        assert np.array_equal(rl.paint_host(r.to_dict(), H, W), lab)
    assert np.array_equal(rl.paint_host({}, 2, 3, background=8), np.full((2, 3), 8))
    assert np.array_equal(rl.paint_host({7: [[1, 6]]}, 2, 3), np.full((2, 3), 7))


def test_paint_host_refuses_overlap_and_range():
    for bad in ({1: [[1, 3]], 2: [[3, 2]]}, {1: [[1, 3], [2, 1]]}, {1: [[0, 2]]}, {1: [[5, 3]]}, {1: [[2, 0]]}, {1: [[7, 1]]}, {2 ** 31: [[1, 1]]}):
        with pytest.raises(E):
            rl.paint_host(bad, 2, 3)
    r = rl.runs_host(wrap_map(), 5)
    with pytest.raises(E):
        rl.paint_host(r, 3, 4)                                        # the RunLengths of another image size
    with pytest.raises(E):
        rl.paint_host(r, 4, 3, ids=[1, 2])
    with pytest.raises(E):
        rl.paint_host([[1, 2]], 4, 3)
    assert np.array_equal(rl.paint_host({1: [[1, 3]], 2: [[4, 3]]}, 2, 3), [[1, 1, 2], [1, 2, 2]])    # touching runs do not overlap


def test_strings_round_trip_and_submission_rows():
    lab = blob_map(23, 37, 9, 1)
    lab[lab == 4] = 0                                                 # an empty instance in the middle
    r = rl.runs_host(lab, 9)
    assert r.counts()[3] == 0 and r.string(3) == "" and rl.parse_string("").shape == (0, 2)
    for k in range(len(r)):
        back = rl.parse_string(r.string(k))
        assert back.dtype == np.int64 and np.array_equal(back, r.of(k))
    rows = rl.submission_rows("img7", r)
    full = [k for k in range(9) if r.counts()[k]]
    assert len(rows) == len(full) < 9 and rows == [("img7", r.string(k)) for k in full] and all(s for _, s in rows)
    for bad in ("1 2 3", "1 x"):
        with pytest.raises(E):
            rl.parse_string(bad)
    with pytest.raises(E):
        rl.submission_rows("a", {1: [[1, 1]]})


def test_runlengths_object():
    a = rl.RunLengths([0, 2, 2, 3], [2, 7, 0], [5, 8, 0], 4, 3)
    assert len(a) == 3 and a.counts().tolist() == [2, 0, 1] and a.areas().tolist() == [6, 0, 1] and a.rows().tolist() == [0, 0, 2]
    assert a.slice(1, 3).indptr.tolist() == [0, 0, 1] and a.slice(1, 3).first.tolist() == [0]
    assert a != rl.RunLengths([0, 2, 2, 3], [2, 7, 0], [5, 8, 0], 3, 4) and a == rl.RunLengths(np.array([0, 2, 2, 3]), np.array([2, 7, 0]), np.array([5, 8, 0]), 4, 3)
    assert a.to_dict(ids=[5, 6, 9])[9].tolist() == [[1, 1]]
    for bad in (([0, 2], [1], [1]), ([1, 2], [1], [1]), ([0, 1], [1], [1, 2])):
        with pytest.raises(E):
            rl.RunLengths(*bad, 4, 3)


def test_binding_and_defaults_are_in_place():
    import inspect
    from kg_instance_segmentation_amd import inference, tiling
    assert {"kg_label_run_counts", "kg_label_runs", "kg_runs_paint"} <= set(_lib._SIGS)
    for fn in (inference.predict_instances, tiling.predict_tiled):
        assert inspect.signature(fn).parameters["runs"].default is None
    assert instances.Instances(None, [], None, None).runs is None
