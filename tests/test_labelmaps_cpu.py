"""The argument and batch layer the label-map modules share (_labelmaps.py), pinned directly at the smallest shapes where it can go wrong:
the n / jobs / stats rule and its clamp (job_table), the jobs_or_n rule of every *_host entry (host_job_table), the side bound and its two
reasons (side), and the walk over predict_instances' list (size_batches, deal) on host label maps.  The device branch of the walk is what
the batch tests of the test_gpu_* files run."""
import numpy as np
import pytest

from kg_instance_segmentation_amd import _labelmaps as lm
from kg_instance_segmentation_amd import _lib, contours, hulls, instances, intensity, labelmetrics, measure, neighbours, runlengths, texture

E = _lib.KGLibraryError
H, W = 7, 9


def two_maps():
    """[2, 7, 9]: ids 1 and 2 in map 0, nothing in map 1"""
    lab = np.zeros((2, H, W), np.int32)
    lab[0, 1:3, 2:5] = 1
    lab[0, 4:7, 6:9] = 2
    return lab


STATS0 = np.array([[6, 1, 2, 3, 5], [9, 4, 6, 7, 9]], np.int64)            # (area, y1, x1, y2, x2) of map 0
JOBS0 = np.array([[0, 1, 1, 2, 3, 5], [0, 2, 4, 6, 7, 9]], np.int64)


def no_stats(lab, n):
    raise AssertionError("stats_of must not be called when stats or jobs are given")


# ---- job_table --------------------------------------------------------------------------------------------------------------------------

def test_job_table_counts_and_stats_forms():
    lab = two_maps()
    one = lm.job_table("f", lab[:1], 2, None, STATS0, no_stats)              # a scalar count and ONE [n, 5] array for one map
    assert one.dtype == np.int64 and np.array_equal(one, JOBS0)
    assert np.array_equal(lm.job_table("f", lab[:1], [2], None, [STATS0], no_stats), JOBS0)          # the list forms of both
    both = lm.job_table("f", lab, [2, 0], None, [STATS0, np.zeros((0, 5), np.int64)], no_stats)      # one count and one array per map
    assert np.array_equal(both, JOBS0)
    seen = []

    def stats_of(m, n):
        seen.append((m.shape, n))
        return labelmetrics.label_stats_host(m, n)
    assert np.array_equal(lm.job_table("f", lab, [2, 0], None, None, stats_of), JOBS0)               # without stats: stats_of per map
    assert seen == [((H, W), 2), ((H, W), 0)]
    hidden = lm.job_table("f", lab[:1], 2, None, np.array([[0, 1, 2, 3, 5], [9, 4, 6, 7, 9]]), no_stats)
    assert np.array_equal(hidden, [[0, 1, 0, 0, 0, 0], [0, 2, 4, 6, 7, 9]])                          # area 0: an empty box


def test_job_table_clamps_and_keeps_a_bad_image_index():
    lab = two_maps()
    jobs = [[0, 1, -3, -2, H + 13, W + 21],                                  # reaches outside on all four sides
            [1, 2, H + 1, W + 1, H + 5, W + 5],                              # wholly outside: clamped to an empty box at the far corner
            [5, 1, 1, 1, 3, 3], [-1, 2, -1, 1, 3, 30]]                       # bad image indices: kept, the box still clamped
    given = np.array(jobs, np.int32)
    got = lm.job_table("f", lab, None, given, None, no_stats)
    assert got.dtype == np.int64
    assert np.array_equal(got, [[0, 1, 0, 0, H, W], [1, 2, H, W, H, W], [5, 1, 1, 1, 3, 3], [-1, 2, 0, 1, 3, W]])
    assert np.array_equal(given, jobs)                                       # the caller's table is not written
    assert lm.job_table("f", lab, None, np.zeros((0, 6), np.int64), None, no_stats).shape == (0, 6)


def test_job_table_refusals_name_the_function():
    lab = two_maps()
    with pytest.raises(E, match=r"^inscribed: jobs cannot be given together with n / stats"):
        lm.job_table("inscribed", lab, [2, 0], JOBS0, None, no_stats)
    with pytest.raises(E, match=r"^runs: jobs cannot be given together with n / stats"):
        lm.job_table("runs", lab, None, JOBS0, [STATS0, STATS0[:0]], no_stats)
    with pytest.raises(E, match=r"^hulls: the instance count n or a job table is needed"):
        lm.job_table("hulls", lab, None, None, None, no_stats)
    with pytest.raises(E, match=r"^glcm: stats must be \[n, 5\] per label map \(2 map\(s\), counts \[2, 0\]\)"):
        lm.job_table("glcm", lab, [2, 0], None, [STATS0, STATS0], no_stats)     # the second map has 0 instances, not 2
    with pytest.raises(E, match=r"^glcm: stats must be \[n, 5\] per label map"):
        lm.job_table("glcm", lab, [2, 0], None, [STATS0], no_stats)             # one array for two maps
    with pytest.raises(E, match=r"^measure: 1 instance count\(s\) for 2 label map\(s\)"):
        lm.job_table("measure", lab, 2, None, None, no_stats)
    with pytest.raises(E, match=r"^measure: jobs must be integers \[m, 6\]"):
        lm.job_table("measure", lab, None, JOBS0[:, :5], None, no_stats)


# ---- host_job_table, through every *_host entry -----------------------------------------------------------------------------------------

IMG = (np.arange(2 * H * W * 2, dtype=np.int64) * 37 % 251).astype(np.uint8).reshape(2, H, W, 2)


def _rows(r):
    """a *_host result as comparable arrays"""
    if isinstance(r, np.ndarray):
        return [r]
    if isinstance(r, texture.CoMatrices):
        return [r.counts]
    return [np.asarray(getattr(r, k)) for k in r.__slots__ if k not in ("H", "W")]


HOST_ENTRIES = {
    "measure_host": (lambda lab, j: measure.measure_host(lab, j, IMG), np.ndarray, (0, 18)),
    "neighbours_host": (lambda lab, j: neighbours.neighbours_host(lab, j), neighbours.Neighbours, None),
    "runs_host": (lambda lab, j: runlengths.runs_host(lab, j), runlengths.RunLengths, None),
    "contours_host": (lambda lab, j: contours.contours_host(lab, j), contours.Contours, None),
    "hulls_host": (lambda lab, j: hulls.hulls_host(lab, j), hulls.Hulls, None),
    "quantiles_host": (lambda lab, j: intensity.quantiles_host(lab, j, IMG, [0.5]), np.ndarray, (0, 2, 3)),
    "glcm_host": (lambda lab, j: texture.glcm_host(lab, j, IMG, levels=4), texture.CoMatrices, (0, 2, 1, 4, 4, 4)),
}


@pytest.mark.parametrize("name", sorted(HOST_ENTRIES))
def test_host_entries_take_counts_jobs_and_an_empty_list(name):
    call, kind, empty_shape = HOST_ENTRIES[name]
    lab = two_maps()
    by_n = call(lab, [2, 0])
    by_jobs = call(lab, JOBS0)
    assert isinstance(by_n, kind) and len(by_n) == 2
    assert all(np.array_equal(a, b) for a, b in zip(_rows(by_n), _rows(by_jobs)))
    outside = JOBS0 + [0, 0, -2, -3, 1, 0]                                   # grown past the map on the top and the left: clamped
    assert all(np.array_equal(a, b) for a, b in zip(_rows(call(lab, outside)), _rows(by_jobs)))
    for none in ([], np.zeros((0, 6), np.int64)):
        got = call(lab, none)
        assert isinstance(got, kind) and len(got) == 0
        if empty_shape is not None:
            assert _rows(got)[0].shape == empty_shape and _rows(got)[0].dtype == np.int64
    with pytest.raises(E, match=f"^{name}: 1 instance count"):
        call(lab, 2)                                                         # a stack of two maps needs two counts


def test_host_job_table_itself():
    lab = two_maps()
    assert np.array_equal(lm.host_job_table("f", lab, [2, 0], labelmetrics.label_stats_host), JOBS0)
    assert np.array_equal(lm.host_job_table("f", lab, JOBS0.tolist(), no_stats), JOBS0)
    assert lm.host_job_table("f", lab, [], no_stats).shape == (0, 6)
    assert lm.host_job_table("f", lab, (), no_stats).dtype == np.int64


# ---- side ---------------------------------------------------------------------------------------------------------------------------------

def _thin(h, w):
    """a map of h x w over ONE stored element"""
    return np.broadcast_to(np.zeros((), np.int32), (h, w))


def test_side_bound_and_its_reasons():
    assert lm.MAX_SIDE == 32768 and measure.MAX_SIDE == 32768
    for shape in ((32768, 1), (1, 32768), (3, 32768, 1)):
        a = _thin(*shape[-2:]) if len(shape) == 2 else np.broadcast_to(np.zeros((), np.int32), shape)
        assert lm.side("f", a) is a
    with pytest.raises(E, match=r"^f: a map of 32769 x 1 exceeds 32768$"):
        lm.side("f", _thin(32769, 1))
    with pytest.raises(E, match=r"^f: a map of 1 x 32769 exceeds 32768 \(because\)$"):
        lm.side("f", _thin(1, 32769), "because")
    assert lm.host_stack("f", _thin(32768, 1)).shape == (1, 32768, 1)
    none = np.zeros((0, 6), np.int64)
    with pytest.raises(E, match=r"^measure_host: a map of 32769 x 1 exceeds 32768 \(the bound that keeps every sum inside int64\)$"):
        measure.measure_host(_thin(32769, 1), none)
    with pytest.raises(E, match=r"^quantiles_host: a map of 1 x 32769 exceeds 32768 \(the bound that keeps every sum inside int64\)$"):
        intensity.quantiles_host(_thin(1, 32769), none, np.zeros((1, 32769, 1), np.uint8))
    with pytest.raises(E, match=r"^neighbours_host: a map of 1 x 32769 exceeds 32768 \(the bound that keeps every count inside int64\)$"):
        neighbours.neighbours_host(_thin(1, 32769), none)
    with pytest.raises(E, match=r"^contours_host: a map of 32769 x 1 exceeds 32768$"):
        contours.contours_host(_thin(32769, 1), none)
    assert len(runlengths.runs_host(_thin(32768, 1), none)) == 0             # the bound itself passes


# ---- size_batches and deal ----------------------------------------------------------------------------------------------------------------

def _instances(lab):
    n = int(lab.max())
    t = np.zeros((n, 8), np.int64)
    for k in range(n):
        ys, xs = np.nonzero(lab == k + 1)
        if len(ys):
            t[k] = len(ys), len(ys), ys.min(), xs.min(), ys.max() + 1, xs.max() + 1, ys.sum(), xs.sum()
    return instances.Instances(lab, np.zeros((n, 5), np.float32), t, None)


def _batch():
    """two sizes (5 x 6 twice, 4 x 4 once), a None entry and an entry without instances"""
    a = np.zeros((5, 6), np.int32); a[0:2, 0:3] = 1; a[3:5, 2:6] = 2
    b = np.zeros((4, 4), np.int32); b[1:3, 1:4] = 1
    c = np.zeros((5, 6), np.int32); c[2, 1:5] = 1; c[4, 0] = 2; c[0, 5] = 3
    return [_instances(a), None, _instances(b), _instances(np.zeros((4, 4), np.int32)), _instances(c)]


def test_size_batches_hands_host_entries_over_in_order():
    insts = _batch()
    seen = []
    assert list(lm.size_batches("f", insts, lambda i, inst, lab: seen.append((i, inst, lab)))) == []   # no device entry: no stack
    assert [s[0] for s in seen] == [0, 2, 3, 4]
    assert all(inst is insts[i] and isinstance(lab, np.ndarray) and lab is inst.labels for i, inst, lab in seen)
    assert list(lm.size_batches("f", [None, None], None)) == []
    with pytest.raises(E, match="^f .*needs the label maps on a GPU device"):
        list(lm.size_batches("f", insts))                                    # a family without a host route
    with pytest.raises(E, match="^f: an Instances or a TiledInstances"):
        list(lm.size_batches("f", [insts[0], "x"], lambda *a: None))
    bad = _instances(insts[0].labels)
    bad.table = bad.table[:1]
    seen.clear()
    with pytest.raises(E, match=r"^f: a table of \(1, 8\) for 2 instances"):
        list(lm.size_batches("f", [insts[0], bad], lambda i, inst, lab: seen.append(i)))
    assert seen == []                                                        # every entry is checked before any work


def test_size_groups_and_deal():
    insts = _batch()
    sizes = [v.labels.shape for v in insts if v is not None]
    assert lm.size_groups(sizes) == [((5, 6), [0, 3]), ((4, 4), [1, 2])]
    assert list(lm.deal(insts, [0, 4])) == [(0, 0, 2), (4, 2, 5)]
    assert list(lm.deal(insts, [2, 3])) == [(2, 0, 1), (3, 1, 1)]            # an entry without instances owns no row
    assert list(lm.deal(insts, [4, 0], [1, 0])) == [(4, 0, 1), (0, 1, 1)]    # row counts of the caller's own
    assert list(lm.deal(insts, [])) == []


@pytest.mark.parametrize("batch, one, attr", [(runlengths.runs_instances_batch, runlengths.runs_instances, "runs"),
                                              (contours.contours_instances_batch, contours.contours_instances, "contours"),
                                              (hulls.hulls_instances_batch, hulls.hulls_instances, "hulls"),
                                              (neighbours.neighbours_instances_batch, neighbours.neighbours_instances, "neighbours")])
def test_batches_land_on_their_entries(batch, one, attr):
    insts = _batch()
    assert batch(insts) is insts and insts[1] is None
    for v in insts:
        if v is not None:
            got = getattr(v, attr)
            assert len(got) == len(v) and got == one(v)
    assert len(getattr(insts[3], attr)) == 0
