"""CPU: the touching-neighbour graph in NumPy (neighbours.neighbours_host, neighbours_rows_host) against a per-pixel Python loop, and the
pager and merger (neighbours.paged) driven by the host rows.  Every comparison is exact integer equality."""
import numpy as np
import pytest

from kg_instance_segmentation_amd import _lib
from kg_instance_segmentation_amd import measure as ms
from kg_instance_segmentation_amd import neighbours as nb

I32 = np.iinfo(np.int32)
H0, W0, N0 = 70, 131, 40


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


def loop_graph(lab, n, connectivity):
    """Per id 1 .. n: {value: [sides, corners]} by a loop over every pixel of the map and every direction"""
    H, W = lab.shape
    out = [dict() for _ in range(n)]
    dirs = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0)]
    if connectivity == 8:
        dirs += [(-1, -1, 1), (-1, 1, 1), (1, -1, 1), (1, 1, 1)]
    for y in range(H):
        for x in range(W):
            a = int(lab[y, x])
            if not 1 <= a <= n:
                continue
            for dy, dx, c in dirs:
                if 0 <= y + dy < H and 0 <= x + dx < W:
                    b = int(lab[y + dy, x + dx])
                    if b != a and b != 0:
                        out[a - 1].setdefault(b, [0, 0])[c] += 1
    return out


@pytest.fixture(scope="module")
def blobs():
    lab = blob_map(H0, W0, N0, 170)
    return lab, {c: nb.neighbours_host(lab, N0, c) for c in (4, 8)}


@pytest.mark.parametrize("connectivity", [4, 8])
def test_host_equals_the_pixel_loop(blobs, connectivity):
    lab, graphs = blobs
    g = graphs[connectivity]
    want = loop_graph(lab, N0, connectivity)
    assert len(g) == N0 and g.indptr.dtype == g.values.dtype == g.sides.dtype == g.corners.dtype == np.int64
    for k in range(N0):
        v, s, c = g.of(k)
        assert v.tolist() == sorted(want[k]) and s.tolist() == [want[k][b][0] for b in sorted(want[k])]
        assert c.tolist() == [want[k][b][1] for b in sorted(want[k])]
    assert np.array_equal(g.degree(), [len(w) for w in want])


def test_the_input_exercises_paging_and_corners(blobs):
    lab, graphs = blobs
    g4, g8 = graphs[4], graphs[8]
    assert (len(g4.pairs()), len(g8.pairs())) == (76, 79)
    assert (g4.degree().max(), g8.degree().max()) == (9, 10)
    assert (int((g4.degree() > 2).sum()), int((g8.degree() > 2).sum())) == (27, 28)
    seen = np.bincount(lab.reshape(-1), minlength=N0 + 1)[1:] > 0       # one id is painted over entirely: an empty row, not an isolated instance
    assert int((~seen).sum()) == 1 and not g8.degree()[~seen].any()
    assert int((g4.degree()[seen] == 0).sum()) == 1 and int((g8.degree()[seen] == 0).sum()) == 1
    assert int(((g8.sides == 0) & (g8.corners > 0)).sum()) == 6 and not g4.corners.any() and (g4.sides > 0).all()


@pytest.mark.parametrize("connectivity", [4, 8])
def test_symmetry_and_contact_sums(blobs, connectivity):
    lab, graphs = blobs
    g = graphs[connectivity]
    ent = {(a + 1, int(b)): (int(s), int(c)) for a in range(N0) for b, s, c in zip(*g.of(a))}
    assert ent and all(ent.get((b, a)) == sc for (a, b), sc in ent.items())
    assert np.array_equal(g.contact_length(), ms.measure_host(lab, N0)[:, 8])
    p = g.pairs()
    assert p.dtype == np.int64 and p.shape[1] == 4 and (p[:, 0] < p[:, 1]).all() and len(p) * 2 == len(g.values)
    assert all(ent[(a, b)] == (s, c) for a, b, s, c in p.tolist())


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("cap", [65536, 50])
def test_pager_over_host_rows(blobs, connectivity, cap):
    lab, graphs = blobs
    jobs = ms.jobs_from_stats(ms.labelmetrics.label_stats_host(lab, N0))
    for slots in (1, 2, 3, 64):
        calls = []

        def rows(table):
            calls.append(len(table))
            return nb.neighbours_rows_host(lab, table, slots, connectivity)
        assert nb.paged(rows, jobs, H0, W0, slots, cap) == graphs[connectivity]
        if cap == 65536:                                              # one piece per job: a round per `slots` neighbours of the busiest one
            assert calls[0] == N0 and len(calls) == -(-graphs[connectivity].degree().max() // slots)
        else:                                                         # bands: a band edge inside the map is not an object edge
            assert calls[0] > N0


def test_resume_semantics():
    lab = np.zeros((5, 9), np.int32)
    lab[2, 1:8] = 5
    lab[1, 1], lab[1, 3], lab[3, 2], lab[3, 5], lab[1, 6] = I32.max, -1, I32.min, 7, 3
    full = nb.neighbours_host(lab, np.array([[0, 5, 0, 0, 5, 9]]))
    assert full.of(0)[0].tolist() == [I32.min, -1, 3, 7, I32.max] and full.of(0)[1].tolist() == [1] * 5

    def row(resume, after, slots=8):
        return nb.neighbours_rows_host(lab, np.array([[0, 5, 0, 0, 5, 9, resume, after]]), slots)[0]
    r = row(0, 0)
    assert r[:2].tolist() == [5, 0] and r[2:17:3].tolist() == [I32.min, -1, 3, 7, I32.max] and not r[17:].any()
    assert np.array_equal(row(0, I32.max), r) and np.array_equal(row(0, I32.min), r)      # resume == 0 ignores after
    r = row(1, I32.min)
    assert r[:2].tolist() == [4, 0] and r[2:14:3].tolist() == [-1, 3, 7, I32.max]       # only INT_MIN is skipped
    assert not row(1, I32.max).any()                                                     # count = more = 0
    r = row(1, -1, 2)
    assert r.tolist() == [2, 1, 3, 1, 0, 7, 1, 0]
    r = row(1, 3, 2)
    assert r.tolist() == [2, 0, 7, 1, 0, I32.max, 1, 0]                                 # the last value written is the last: more == 0
    assert row(0, 0, 1).tolist() == [1, 1, I32.min, 1, 0]
    # the background is a value like any other as an id, never as a neighbour
    zero = nb.neighbours_host(lab, np.array([[0, 0, 0, 0, 5, 9]]))
    assert zero.of(0)[0].tolist() == [I32.min, -1, 3, 5, 7, I32.max]


def test_three_by_three_and_one_pixel():
    lab = np.arange(1, 10, dtype=np.int32).reshape(3, 3)
    centre = np.array([[0, 5, 1, 1, 2, 2]])
    g8, g4 = nb.neighbours_host(lab, centre, 8), nb.neighbours_host(lab, centre, 4)
    assert g8.of(0)[0].tolist() == [1, 2, 3, 4, 6, 7, 8, 9]
    assert g8.of(0)[1].tolist() == [0, 1, 0, 1, 1, 0, 1, 0] and g8.of(0)[2].tolist() == [1, 0, 1, 0, 0, 1, 0, 1]
    assert g4.of(0)[0].tolist() == [2, 4, 6, 8] and g4.of(0)[1].tolist() == [1, 1, 1, 1] and not g4.of(0)[2].any()
    one = np.full((1, 1), 3, np.int32)
    for c in (4, 8):
        g = nb.neighbours_host(one, np.array([[0, 3, 0, 0, 1, 1], [0, 0, 0, 0, 1, 1]]), c)
        assert len(g) == 2 and g.indptr.tolist() == [0, 0, 0] and len(g.values) == 0
        assert not nb.neighbours_rows_host(one, np.array([[0, 3, 0, 0, 1, 1, 0, 0]]), 4, c).any()
    assert nb.neighbours_host(one, 3).degree().tolist() == [0, 0, 0] and len(nb.neighbours_host(one, 3).pairs()) == 0


def test_bad_jobs_and_stacks():
    lab = np.stack([blob_map(20, 30, 6, 1), blob_map(20, 30, 6, 2)])
    jobs = np.array([[0, 2, 0, 0, 20, 30], [1, 2, 0, 0, 20, 30], [2, 2, 0, 0, 20, 30], [-1, 2, 0, 0, 20, 30], [0, 2, 9, 9, 3, 3],
                     [0, 2, 5, 5, 5, 9], [0, 77, 0, 0, 20, 30], [1, 2, -99, -99, 99, 99]])
    g = nb.neighbours_host(lab, jobs, 8)
    assert g.degree()[0] > 0 and g.degree()[1] > 0 and not g.degree()[2:7].any()
    assert all(np.array_equal(a, b) for a, b in zip(g.of(7), g.of(1)))
    assert g.of(0)[0].tolist() != g.of(1)[0].tolist() or g.of(0)[1].tolist() != g.of(1)[1].tolist()      # content per image
    both = nb.neighbours_host(lab, [6, 6])
    assert len(both) == 12 and both.slice(6, 12) == nb.neighbours_host(lab[1], 6)
    rows = nb.neighbours_rows_host(lab, np.concatenate([jobs, np.zeros((len(jobs), 2), np.int64)], 1), 64, 8)
    assert rows[:, 0].tolist() == g.degree().tolist() and not rows[2:7].any()


def test_neighbours_structure_and_argument_errors():
    g = nb.Neighbours([0, 2, 2, 3], [2, 9, 1], [4, 1, 4], [0, 1, 0])
    assert len(g) == 3 and g.degree().tolist() == [2, 0, 1] and g.contact_length().tolist() == [5, 0, 4]
    assert g.pairs().tolist() == [[1, 2, 4, 0], [1, 9, 1, 1]]
    assert g.pairs([5, 6, 7]).tolist() == [[5, 9, 1, 1]]
    assert g == nb.Neighbours.from_lists([g.of(k) for k in range(3)]) and g != g.slice(0, 2) and g.slice(2, 3).of(0)[0].tolist() == [1]
    lab = np.ones((4, 4), np.int32)
    E = _lib.KGLibraryError
    for bad in (6, 0, True, "8"):
        with pytest.raises(E):
            nb.neighbours_host(lab, 1, bad)
    for bad in (0, 65, -1, 2.0):
        with pytest.raises(E):
            nb.neighbours_rows_host(lab, np.zeros((1, 8), np.int64), bad)
        with pytest.raises(E):
            nb.paged(lambda t: None, np.zeros((1, 6), np.int64), 4, 4, bad)
    with pytest.raises(E):
        nb.neighbours_host(lab.astype(np.float32), 1)
    with pytest.raises(E):
        nb.neighbours_rows_host(lab, np.zeros((1, 6), np.int64), 4)    # the row entry takes 8 columns
    with pytest.raises(E):
        nb.neighbours_host(lab, np.zeros((1, 8), np.int64))            # the graph takes 6
    with pytest.raises(E):
        g.pairs([1, 2])
    with pytest.raises(E):
        nb.Neighbours([0, 2], [1], [1], [1])
    with pytest.raises(E):                                             # a row function that never advances is refused, not looped on
        nb.paged(lambda t: np.tile(np.array([1, 1, 5, 1, 0]), (len(t), 1)), np.array([[0, 1, 0, 0, 4, 4]]), 4, 4, 1)
