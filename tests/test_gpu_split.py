"""GPU: the seeded geodesic regrow on the device (csrc/split.hip, split.py) against the host statement of the same semantics
(split.regrow_host / split_host: per-seed breadth-first distance maps and a lexicographic minimum; the device runs a level-synchronous
flood).  Every comparison is exact integer equality.  Shapes are the smallest at which the kernel can go wrong: one-pixel, one-row and
one-column maps with the tie pixel in the middle, box widths around the 256-thread walk, both sides of the size rule, a serpentine of
1023 levels, a checkerboard, more seeds than threads, ranks and ids of any int32, boxes that cut or overhang, several images in one
launch, hostile job tables between guards, more jobs than the grid cap, and the predict routes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import split_cases as sc  # noqa: E402
from kg_instance_segmentation_amd import KGnet, _lib, inference, instances, labelmetrics, tiling  # noqa: E402
from kg_instance_segmentation_amd import components as cc  # noqa: E402
from kg_instance_segmentation_amd import contours as ct  # noqa: E402
from kg_instance_segmentation_amd import distance as dt  # noqa: E402
from kg_instance_segmentation_amd import hulls as hl  # noqa: E402
from kg_instance_segmentation_amd import measure as ms  # noqa: E402
from kg_instance_segmentation_amd import runlengths as rl  # noqa: E402
from kg_instance_segmentation_amd import split as sp  # noqa: E402

DEV = "cuda"
I32 = np.iinfo(np.int32)
E = _lib.KGLibraryError


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def job_fits(jobs, H, W):
    j = np.asarray(jobs, np.int64).reshape(-1, 8)
    h = np.maximum(np.minimum(j[:, 4], H) - np.maximum(j[:, 2], 0), 0)
    w = np.maximum(np.minimum(j[:, 5], W) - np.maximum(j[:, 3], 0), 0)
    return np.array([sp.fits(a, b) for a, b in zip(h, w)], bool)


def same_as_host(lab, seeds, jobs, conn=4):
    """the raw entry and regrow (with the host route of the boxes that do not fit) against regrow_host -> (out, rows) of the host"""
    lab, seeds = np.asarray(lab, np.int32), np.asarray(seeds, np.int32)
    jobs = np.asarray(jobs, np.int64).reshape(-1, 8)
    want, wrows = sp.regrow_host(lab, seeds, jobs, conn)
    fit = job_fits(jobs, *lab.shape[-2:])
    d, s = up(lab), up(seeds)
    out, rows = sp.regrow_rows(d, s, jobs, conn)
    assert out.is_cuda and out.dtype == torch.int32 and out.shape == d.shape and rows.dtype == torch.int32 and rows.shape == (len(jobs), 4)
    rows = rows.cpu().numpy()
    assert np.array_equal(rows[fit], wrows[fit]) and np.array_equal(rows[~fit], np.tile([0, 0, 0, 1], ((~fit).sum(), 1)))
    if fit.all():
        assert np.array_equal(out.cpu().numpy(), want)
    assert torch.equal(d, up(lab)) and torch.equal(s, up(seeds))       # the inputs are left alone
    out2, rows2 = sp.regrow(d, s, jobs, conn)
    assert np.array_equal(out2.cpu().numpy(), want)
    assert np.array_equal(rows2[:, :3], wrows[:, :3]) and np.array_equal(rows2[:, 3], (~fit).astype(np.int64))
    return want, wrows


# ---- smallest maps, ties, widths, the size rule ---------------------------------------------------------------------------------------------

def test_one_pixel():
    lab = np.ones((1, 1), np.int32)
    for s, want in ((1, 1), (2, 9), (3, 1), (0, 1)):
        out, rows = same_as_host(lab, [[s]], [[0, 1, 0, 0, 1, 1, 2, 9]])
        assert out.tolist() == [[want]] and rows[0].tolist() == [1, int(s not in (1, 2)), 0, 0]


@pytest.mark.parametrize("n", [2, 7, 8, 255, 256, 257, 1001])
@pytest.mark.parametrize("col", [False, True])
def test_lines_with_a_seed_at_each_end(n, col):
    lab = np.ones((n, 1) if col else (1, n), np.int32)
    s = np.zeros(n, np.int32)
    s[0], s[-1] = 2, 1                                                # the far end holds rank 1: the tie pixel of an odd line goes there
    out, rows = same_as_host(lab, s.reshape(lab.shape), [[0, 1, 0, 0, *lab.shape, 2, 5]], 8 if n % 2 else 4)
    flat = out.reshape(-1)
    assert (flat[:(n - 1) // 2] == 5).all() and (flat[n // 2:] == 1).all() and flat[(n - 1) // 2] == (1 if n % 2 else 5)
    assert rows[0].tolist() == [n, 0, (n - 1) // 2, 0]


@pytest.mark.parametrize("w", [1, 255, 256, 257])
def test_box_widths(w):
    rng = np.random.default_rng(w)
    lab = (rng.random((7, w + 4)) < 0.8).astype(np.int32)
    s = sc.random_seed_map(lab, 6, w, 3)
    jobs = [[0, 1, 0, 2, 7, 2 + w, 3, 10], [0, 1, 2, 2, 5, 2 + w, 3, 20]] if w > 1 else [[0, 1, 0, 2, 7, 3, 3, 10]]
    for conn in (4, 8):
        same_as_host(lab, s, jobs[:1], conn)
        same_as_host(lab, s, jobs[1:], conn)


@pytest.mark.parametrize("h,w", [(126, 126), (126, 127), (127, 126), (1, 5459), (1, 5460), (5459, 1), (5460, 1)])
def test_both_sides_of_the_size_rule(h, w):
    rng = np.random.default_rng(h + w)
    lab = (rng.random((h, w)) < (0.75 if min(h, w) > 1 else 0.999)).astype(np.int32)
    s = sc.random_seed_map(lab, 12, h, 4)
    out, rows = same_as_host(lab, s, [[0, 1, 0, 0, h, w, 4, 2]], 8 if h % 2 else 4)
    assert sp.fits(h, w) == ((h + 2) * (w + 2) <= 16384) and rows[0, 0] > 0 and rows[0, 2] > 0 and len(np.unique(out)) > 2


def test_serpentine():
    lab, a, b = sc.serpentine(63)
    s = np.zeros_like(lab)
    s[a], s[b] = 1, 2
    assert lab.sum() == 2047
    out, rows = same_as_host(lab, s, [[0, 1, 0, 0, 63, 63, 2, 2]])
    assert rows[0].tolist() == [2047, 0, 1023, 0] and (out == 2).sum() == 1023
    s[a] = 0                                                           # one seed: the whole path, 2046 levels
    out, rows = same_as_host(lab, s, [[0, 1, 0, 0, 63, 63, 2, 2]])
    assert rows[0].tolist() == [2047, 0, 2046, 0] and (out == 2).sum() == 2047
    out, rows = same_as_host(lab, s, [[0, 1, 0, 0, 63, 63, 2, 2]], 8)   # diagonal steps cut the corner of every turn
    assert rows[0, 2] < 2046


def test_checkerboard():
    yy, xx = np.mgrid[0:41, 0:53]
    lab = ((yy + xx) % 2 == 0).astype(np.int32)
    s = np.zeros_like(lab)
    s[0, 0], s[40, 52], s[20, 26] = 1, 2, 3
    out, rows = same_as_host(lab, s, [[0, 1, 0, 0, 41, 53, 3, 2]], 4)
    assert rows[0].tolist() == [int(lab.sum()), int(lab.sum()) - 3, 0, 0]
    out, rows = same_as_host(lab, s, [[0, 1, 0, 0, 41, 53, 3, 2]], 8)
    assert rows[0, 1] == 0 and rows[0, 2] > 10 and set(np.unique(out)) == {0, 1, 2, 3}


@pytest.mark.parametrize("S", [255, 256, 257, 1000])
def test_many_one_pixel_seeds(S):
    rng = np.random.default_rng(S)
    lab = np.zeros((44, 50), np.int32)
    lab[2:42, 3:48] = 1
    lab[10:30, 20] = 0
    s = np.zeros_like(lab)
    pos = rng.permutation(np.flatnonzero(lab.reshape(-1)))[:S]
    s.reshape(-1)[pos] = rng.permutation(S) + 1
    out, rows = same_as_host(lab, s, [[0, 1, 0, 0, 44, 50, S, 2]], 4 if S % 2 else 8)
    assert rows[0, 1] == 0 and len(np.unique(out)) == S + 1


def test_ranks_above_nseeds_and_foreign_seeds():
    lab = sc.blobs(60, 70, 5, 4)
    s = sc.random_seed_map(lab, 200, 5, 9)
    stats = labelmetrics.label_stats_host(lab, 5)
    jobs = [[0, k + 1, *stats[k, 1:].tolist(), ns, 100 * (k + 1)] for k, ns in enumerate((9, 4, 1, 0, -3))]
    out, rows = same_as_host(lab, s, jobs)
    assert rows[3, 1] == rows[3, 0] > 0 and rows[4, 1] == rows[4, 0] and np.array_equal(out[lab >= 3], lab[lab >= 3])
    big = s.copy()
    big[s == 5] = 16382
    big[s == 6] = 16383                                               # above the rank field: no seed
    big[s == 7] = I32.max
    big[s == 8] = I32.min
    same_as_host(lab, big, [[0, 1, *stats[0, 1:].tolist(), I32.max, 7], [0, 2, *stats[1, 1:].tolist(), 16382, I32.max - 2]], 8)


def test_any_int32_is_an_id():
    rng = np.random.default_rng(12)
    vals = np.array([0, -1, I32.min, I32.max, 5], np.int32)
    lab = vals[rng.integers(0, 5, (9, 11))].repeat(4, 0).repeat(4, 1)
    s = sc.random_seed_map(lab, 80, 13, 3)
    jobs = [[0, int(v), 0, 0, 36, 44, 3, f] for v, f in zip(vals, (100, I32.max, I32.min, -7, I32.max - 1))]
    for conn in (4, 8):
        out, rows = same_as_host(lab, s, jobs[:1], conn)
        assert rows[0, 0] == (lab == 0).sum() and (out != lab).any()
        for k in range(1, 5):
            same_as_host(lab, s, jobs[k:k + 1], conn)
    out, rows = sp.regrow_host(lab, s, jobs)                           # different ids never store the same pixel: all in one launch
    got, grows = sp.regrow(up(lab), up(s), np.asarray(jobs))
    assert np.array_equal(got.cpu().numpy(), out) and np.array_equal(grows, rows)


def test_boxes_that_cut_or_overhang():
    lab = sc.blobs(50, 64, 4, 7, 5, 12)
    s = sc.random_seed_map(lab, 120, 8, 3)
    jobs = [[0, 1, -5, -9, 30, 40, 3, 10], [0, 2, 10, 12, 80, 90, 3, 20], [0, 3, 20, 0, 21, 64, 3, 30], [0, 4, 0, 30, 50, 31, 3, 40],
            [0, 1, I32.min, I32.min, I32.max, I32.max, 3, 50]]
    for k in range(len(jobs)):
        same_as_host(lab, s, jobs[k:k + 1], 4 + 4 * (k % 2))
    same_as_host(lab, s, jobs[:4])


def test_three_images_with_interleaved_jobs():
    labs = np.stack([sc.blobs(40, 48, 4, 30 + i) for i in range(3)])
    s = np.stack([sc.random_seed_map(labs[i], 60, 40 + i, 3) for i in range(3)])
    jobs = []
    for k in range(4):
        for i in (2, 0, 1):
            st = labelmetrics.label_stats_host(labs[i], 4)
            jobs.append([i, k + 1, *st[k, 1:].tolist(), 3, 10 * (i + 1) + 2 * k])
    for conn in (4, 8):
        out, rows = same_as_host(labs, s, jobs, conn)
        assert (out != labs).reshape(3, -1).any(1).all()


def test_hostile_tables_between_guards():
    H, W, nimg = 24, 40, 2
    labs = np.stack([sc.blobs(H, W, 3, 50 + i, 3, 6) for i in range(nimg)])
    s = np.stack([sc.random_seed_map(labs[i], 50, 60 + i, 3) for i in range(nimg)])
    jobs = np.array([[-1, 1, 0, 0, H, W, 3, 9], [nimg, 1, 0, 0, H, W, 3, 9], [I32.max, 1, 0, 0, H, W, 3, 9], [I32.min, 1, 0, 0, H, W, 3, 9],
                     [0, 1, H, W, 0, 0, 3, 9], [1, 1, 5, 5, 5, 30, 3, 9], [0, 1, I32.max, I32.max, I32.min, I32.min, 3, 9],
                     [1, 2, -I32.max, -I32.max, I32.max, I32.max, I32.max, I32.min], [0, 2, 0, 0, H, W, I32.min, I32.max],
                     [1, 3, H - 1, W - 1, I32.max, I32.max, 2, -1], [0, 77, 0, 0, H, W, 3, 9]], np.int64)
    want, wrows = sp.regrow_host(labs, s, jobs)
    assert not wrows[:7].any() and wrows[7, 0] > 0 and not wrows[10].any()
    m = len(jobs)
    d, sd, jd = up(labs), up(s), up(jobs.astype(np.int32))
    obuf = torch.full((nimg * H * W + 2 * W,), -5, dtype=torch.int32, device=DEV)
    rbuf = torch.full((m + 2, 4), 77, dtype=torch.int32, device=DEV)
    out, rows = obuf[W:-W], rbuf[1:-1]
    _lib.call("kg_label_split", _lib.ptr(d), _lib.ptr(sd), nimg, H, W, 4, _lib.ptr(jd), m, _lib.ptr(out), _lib.ptr(rows), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(labs.shape), want) and np.array_equal(rows.cpu().numpy(), wrows)
    assert (obuf[:W] == -5).all() and (obuf[-W:] == -5).all() and (rbuf[0] == 77).all() and (rbuf[-1] == 77).all()
    same_as_host(labs, s, jobs, 8)


def test_more_jobs_than_the_grid_cap():
    """1 049 600 one-pixel jobs, more than the 2^20 workgroups of a launch: the first blocks take a second job and write their LDS state
    again.  The expected map is a closed form: a pixel whose seed has rank 2 takes its job's first_new, every third one (rank 1) stays."""
    H, W = 1025, 1024
    m = H * W
    lab = np.ones((H, W), np.int32)
    s = np.where(np.arange(m) % 3 == 0, 1, 2).astype(np.int32).reshape(H, W)
    yy, xx = np.divmod(np.arange(m, dtype=np.int64), W)
    jobs = np.stack([np.zeros(m, np.int64), np.ones(m, np.int64), yy, xx, yy + 1, xx + 1, np.full(m, 2), 1000 + np.arange(m)], 1)
    out, rows = sp.regrow_rows(up(lab), up(s), jobs)
    assert np.array_equal(out.cpu().numpy().reshape(-1), np.where(np.arange(m) % 3 == 0, 1, 1000 + np.arange(m)))
    assert np.array_equal(rows.cpu().numpy(), np.tile(np.array([1, 0, 0, 0], np.int32), (m, 1)))
    few = np.concatenate([jobs[:3], jobs[-3:]])
    assert np.array_equal(sp.regrow_host(lab, s, few)[0].reshape(-1)[[0, 1, 2, m - 3, m - 2, m - 1]], out.cpu().numpy().reshape(-1)[[0, 1, 2, m - 3, m - 2, m - 1]])


def test_no_jobs_and_refusals():
    lab = sc.dumbbell(4, 7)
    d = up(lab)
    out, rows = sp.regrow_rows(d, d, np.zeros((0, 8), np.int64))
    assert torch.equal(out, d) and out.data_ptr() != d.data_ptr() and rows.shape == (0, 4)
    out, rows = sp.regrow(d, d, np.zeros((0, 8), np.int64))
    assert torch.equal(out, d) and rows.shape == (0, 4)
    for args in ((lab, d, []), (d, up(lab[:, 1:]), []), (d, d.long(), [])):
        with pytest.raises(E):
            sp.regrow_rows(args[0], args[1], np.zeros((0, 8), np.int64))
    with pytest.raises(E):
        sp.regrow_rows(d, d, np.zeros((1, 6), np.int64))
    with pytest.raises(E):
        sp.regrow_rows(d, d, np.zeros((0, 8), np.int64), 6)
    j = up(np.array([[0, 1, 0, 0, 5, 5, 2, 2]], np.int32))
    r = torch.zeros(1, 4, dtype=torch.int32, device=DEV)
    for o, rr in ((d, r), (torch.empty_like(d), d.view(-1)[:4])):   # out aliases labels; rows alias a map
        with pytest.raises(E):
            _lib.call("kg_label_split", _lib.ptr(d), _lib.ptr(d), 1, *lab.shape, 4, _lib.ptr(j), 1, _lib.ptr(o), _lib.ptr(rr), _lib.stream_ptr())
    with pytest.raises(E):
        sp.split(d, 1, 0)
    with pytest.raises(E):
        sp.split(d[None], 1, 3)


# ---- split against split_host ---------------------------------------------------------------------------------------------------------------

def split_same(lab, n, d, **kw):
    want = sp.split_host(lab, n, d, **kw)
    out, table, parent = sp.split(up(lab), n, d, **kw)
    assert out.is_cuda and out.dtype == torch.int32 and table.dtype == np.int64 and parent.dtype == np.int32
    assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(table, want[1]) and np.array_equal(parent, want[2])
    rank, S = sp.seeds(up(lab), n, d, kw.get("connectivity", 4), kw.get("min_seed_area", 1), kw.get("frame", False))
    hrank, hS = sp.seeds_host(lab, n, d, kw.get("connectivity", 4), kw.get("min_seed_area", 1), kw.get("frame", False))
    assert np.array_equal(rank.cpu().numpy(), hrank) and np.array_equal(S, hS)
    return want


@pytest.mark.parametrize("conn", [4, 8])
def test_split_on_the_cpu_fixtures(conn):
    for (r, gap, d), parts in sc.DUMBBELLS.items():
        for tr in (False, True):
            m = sc.dumbbell(r, gap)
            out, table, parent = split_same(np.ascontiguousarray(m.T) if tr else m, 1, d, connectivity=conn)
            assert parent.tolist() == [0, 0] and (parts[conn == 8] is None or tuple(table[:, 1].tolist()) == parts[conn == 8])
    for r, gap, d in sc.ONE_SEED:
        assert split_same(sc.dumbbell(r, gap), 1, d, connectivity=conn)[2].tolist() == [0]
    for r in (3, 5, 8, 12):
        lab = sc.disc(2 * r + 5, 2 * r + 5, r + 2, r + 2, r).astype(np.int32)
        for d in (1, 2, 3, 5):
            assert split_same(lab, 1, d, connectivity=conn)[2].tolist() == [0]
    assert split_same(sc.three_discs(), 1, 4, connectivity=conn)[1][:, 1].tolist() == ([111, 105, 105] if conn == 4 else split_same(
        sc.three_discs(), 1, 4, connectivity=8)[1][:, 1].tolist())


def test_split_of_a_box_that_does_not_fit():
    out, table, parent = split_same(sc.large_pair(), 1, 8)
    assert parent.tolist() == [0, 0] and (table[:, 1] > 2000).all()


@pytest.mark.parametrize("seed", [0, 1])
def test_split_on_ragged_maps(seed):
    n = 12
    lab = sc.blobs(141, 203, n, 70 + seed, 4, 11)
    out, table, parent = split_same(lab, n, 3)
    assert len(parent) > n + 1
    split_same(lab, n, 3, connectivity=8, only=np.arange(1, n + 1, 2), min_seed_area=3)
    split_same(lab, n, 2.5, frame=True)
    old = np.concatenate([np.arange(n)[:, None] + 500, tiling.table_from_labels_host(
        lab, np.concatenate([np.arange(1, n + 1)[:, None], labelmetrics.label_stats_host(lab, n)[:, 1:]], 1))[:, 1:]], 1)
    out, table, parent = split_same(lab, n, 3, table=old)
    assert np.array_equal(table[:, 0], 500 + parent)


def test_split_batch():
    ns = [6, 9, 4]
    labs = np.stack([sc.blobs(90, 120, k, 80 + i, 4, 10) for i, k in enumerate(ns)])
    only = [None, [1, 2, 3, 4], None]
    out, tabs, parents = sp.split_batch(up(labs), ns, 3, only=only)
    assert sum(len(p) for p in parents) > sum(ns)
    for i in range(3):
        want = sp.split_host(labs[i], ns[i], 3, only=only[i])
        assert np.array_equal(out[i].cpu().numpy(), want[0]) and np.array_equal(tabs[i], want[1]) and np.array_equal(parents[i], want[2])


# ---- Instances, end to end ------------------------------------------------------------------------------------------------------------------

def sheet_instances(device=True):
    lab, n, meta = sc.dumbbell_sheet(2)
    lab = lab.copy()
    lab[1, 0] = 3                                                      # a speck of id 3 for the clean-up to drop
    stats = labelmetrics.label_stats_host(lab, n)
    dets = np.concatenate([stats[:, 1:].astype(np.float32), np.linspace(0.9, 0.5, n, dtype=np.float32)[:, None]], 1)
    table = tiling.table_from_labels_host(lab, np.concatenate([np.arange(1, n + 1)[:, None], stats[:, 1:]], 1), stats[:, 0])
    return instances.Instances(up(lab) if device else lab, dets, table, "the masks"), lab, n


def host_copy(inst):
    new = instances.Instances(inst.labels.cpu().numpy(), inst.dets, inst.table, inst.masks)
    new.parent = inst.parent
    return new


def same_result(a, b):
    return (np.array_equal(a.labels.cpu().numpy() if torch.is_tensor(a.labels) else a.labels, b.labels) and np.array_equal(a.table, b.table)
            and np.array_equal(a.dets, b.dets) and np.array_equal(a.parent, b.parent) and type(a) is type(b) and len(a) == len(b))


@pytest.mark.parametrize("clean", [None, dict(min_area=4, connectivity=4)])
@pytest.mark.parametrize("d,conn", [(4, 4), (7, 8)])
def test_split_instances_end_to_end(d, conn, clean):
    inst, lab, n = sheet_instances()
    hinst = sheet_instances(False)[0]
    if clean is not None:
        inst, hinst = cc.clean_instances(inst, **clean), cc.clean_instances(hinst, **clean)
        assert inst.labels[1, 0] == 0
    got = sp.split_instances(inst, d, connectivity=conn)
    want = sp.split_instances(hinst, d, connectivity=conn)
    assert same_result(got, want) and len(got) == n + 12 and got.masks == "the masks"       # twelve real splits
    assert got.parent[n:].tolist() == sorted(got.parent[n:].tolist()) and np.array_equal(got.dets[n:], inst.dets[got.parent[n:]])
    assert (got.table[:, 1] > 0).all() and got.table[:, 1].sum() == inst.table[:, 1].sum()
    assert np.array_equal(got.table[:, 0], inst.table[got.parent, 0])
    grown = dt.expand_instances(got, 2)                                # every later step works from labels and table alone
    assert same_result(grown, dt.expand_instances(want, 2))
    img = np.random.default_rng(d).integers(0, 256, lab.shape + (3,), dtype=np.uint8)
    for final, hfinal in ((got, want), (grown, host_copy(grown))):
        assert np.array_equal(ms.measure_instances(final, img).raw, ms.measure_instances(hfinal, img).raw)
        assert rl.runs_instances(final) == rl.runs_instances(hfinal)
        assert ct.contours_instances(final) == ct.contours_instances(hfinal)
        hulls = hl.hulls_instances(final)
        assert hulls == hl.hulls_instances(hfinal) and np.array_equal(hulls.areas(), final.table[:, 1])
    # splitting only the suspicious ones: every dumbbell is concave, and each new half is more solid than the pair it came from
    solid = hl.hulls_instances(inst).solidity()
    only = np.flatnonzero(solid < 0.9) + 1
    picked = sp.split_instances(inst, d, connectivity=conn, only=only)
    assert len(only) == n and same_result(picked, want)
    assert (hl.hulls_instances(picked).solidity()[n:] > solid[picked.parent[n:]]).all()
    assert same_result(sp.split_instances(inst, d, connectivity=conn, only=only[:3]), sp.split_instances(hinst, d, connectivity=conn, only=only[:3]))


@pytest.fixture(scope="module")
def cal_model():
    from oracle import weightgen
    m = KGnet.resnet50(pretrained=False)
    m.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    return m.to(DEV).eval()


def same_instances(a, b):
    return (torch.equal(a.labels, b.labels) and np.array_equal(a.dets, b.dets) and np.array_equal(a.table, b.table) and type(a) is type(b))


def test_predict_tiled_with_split(cal_model):
    H, W, S = 400, 600, 256
    img = np.random.default_rng(8).integers(0, 256, (H, W, 3), dtype=np.uint8)
    plain = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4)
    none = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4, split=None)
    assert len(plain) > 0 and plain.parent is None and none.parent is None and same_instances(plain, none)     # the default path is untouched
    host = tiling.TiledInstances(plain.labels.cpu().numpy(), plain.dets, plain.table, plain.tile, plain.origin, plain.tile_masks)
    for kw in (2, dict(distance=2, connectivity=8, min_seed_area=2)):
        got = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4, split=kw)
        want = sp.split_instances(host, **(kw if isinstance(kw, dict) else {"distance": kw}))
        print("instances", len(plain), "after the split", len(got))
        assert same_result(got, want) and got.tile_masks is not None and len(got.tile) == len(got.origin) == len(got)
    policy = dict(min_area=4)
    both = tiling.predict_tiled(cal_model, up(img), tile=S, overlap=64, batch=4, clean=policy, split=2, expand=3, hulls=True, measure=True)
    final = dt.expand_instances(sp.split_instances(cc.clean_instances(plain, **policy), 2), 3)
    assert same_instances(both, final) and np.array_equal(both.parent, final.parent) and len(both.hulls) == len(both) == len(both.measurements.raw)


def test_predict_instances_with_split(cal_model):
    S = 256
    src = np.random.default_rng(9).integers(0, 256, (2, S, S, 3), dtype=np.uint8)
    x = torch.cat([tiling.cut_tiles(src[i], tiling.plan(S, S, S, 64)) for i in range(2)])
    plain = inference.predict_instances(cal_model, x)
    none = inference.predict_instances(cal_model, x, split=None)
    assert all(p is not None and len(p) > 0 and q.parent is None and same_instances(p, q) for p, q in zip(plain, none))
    got = inference.predict_instances(cal_model, x, split=2)
    full = inference.predict_instances(cal_model, x, clean=dict(min_area=4), split=dict(distance=2, connectivity=8), expand=2, runs=True, contours=True)
    for p, g, f in zip(plain, got, full):
        want = sp.split_instances(host_copy(p), 2)
        assert same_result(g, want) and len(g.masks) == len(p.masks) == len(p) <= len(g)      # the masks stay the parents' rows
        ref = dt.expand_instances(sp.split_instances(cc.clean_instances(p, min_area=4), 2, connectivity=8), 2)
        assert same_instances(f, ref) and np.array_equal(f.parent, ref.parent) and len(f.runs) == len(f) == len(f.contours)
