"""GPU: boundary distances on the device (csrc/boundaries.hip, boundaries.py) against the host statements of the same semantics
(boundaries.border_d2_host, border_d2_store_host, pair_distances_host) and LabelEvaluator(boundary=) end to end.  Every comparison is exact
integer equality (and equality of the float64 metrics the same host code derives from the integers).  Shapes are the smallest at which
the kernel can go wrong: one-pixel, one-row and one-column maps, source boxes and source counts on both sides of the 256-position chunk
and of the queue flush, target lists on both sides of the 16-byte read and of the 8192-pixel rule, the frame as border, any int32 as an
id, d2 near 2^30, several images and both directions in one launch, wrong tables between guard words, more jobs than the grid cap."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from kg_instance_segmentation_amd import KGnet, _lib, tiling  # noqa: E402
from kg_instance_segmentation_amd import boundaries as bd  # noqa: E402
from kg_instance_segmentation_amd import labelmetrics as lm  # noqa: E402

from boundaries_cases import (I32, MODES, all_pair_jobs, blob_maps, boxes_of, disc_in_ring, ellipse_pair, job, stripes, thick_row, unsplit_d2,  # noqa: E402
                              whole)

DEV = "cuda"
E = _lib.KGLibraryError


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def raw_equals_host(a, b, jobs, modes=MODES, da=None, db=None):
    """Both raw entries on jobs [m, 13] against their NumPy statements in every mode; -> the counts of the last mode"""
    da, db = up(a) if da is None else da, up(b) if db is None else db
    jobs = np.asarray(jobs, np.int64).reshape(-1, 13)
    for mode in modes:
        want, vals = bd.border_d2_host(a, b, jobs, mode)
        got = bd.border_counts(da, db, jobs, mode)
        assert got.is_cuda and got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), mode
        table = jobs.copy()
        table[:, 12] = np.cumsum(want[:, 0]) - want[:, 0]
        D = int(want[:, 0].sum())
        out = torch.full((D,), -7, dtype=torch.int32, device=DEV)
        assert bd.border_d2(da, db, table, mode, D, out) is out
        flat = np.concatenate(vals) if vals else np.zeros(0, np.int32)
        assert np.array_equal(out.cpu().numpy(), flat), mode
        assert np.array_equal(bd.border_d2_store_host(a, b, table, mode, D, fill=-7), flat)
    return want


@pytest.mark.parametrize("H,W", [(1, 1), (1, 130), (130, 1)])
def test_smallest_maps(H, W):
    n = 5
    a, b = (np.ones((1, 1), np.int32),) * 2 if H * W == 1 else blob_maps(H, W, n, 20 + H)
    jobs = np.concatenate([all_pair_jobs(a, b, n), [job(1, whole(a), 1, whole(a)), job(1, (0, 0, 1, 1), 2, (H - 1, W - 1, H, W), 1)]])
    assert raw_equals_host(a, b, jobs)[:, 0].sum() > 0
    sa, sb = boxes_of(a, n), boxes_of(b, n)
    pairs = [(i, i) for i in range(1, n + 1)]
    want = bd.pair_distances_host(a, b, pairs, sa, sb)
    assert bd.pair_distances(up(a), up(b), pairs, sa, sb) == want and bd.pair_distances(up(a), up(b), pairs, n_a=n, n_b=n, max_job_pixels=1) == want


@pytest.mark.parametrize("w", [1, 255, 256, 257])
def test_source_widths_and_counts_around_the_chunk_and_the_flush(w):
    """Dense sources fill the queue on a chunk edge; sparse ones (every third position, all of them border pixels) flush inside a chunk"""
    for k in (255, 256, 257, 513):
        for every in (1, 3):
            h = -(-k * every // w)
            a = np.zeros((h + 2, max(w, 8) + 3), np.int32)
            flat = np.zeros(h * w, np.int32)
            flat[:k * every:every] = 1
            a[1:h + 1, 2:w + 2] = flat.reshape(h, w)
            b = np.zeros_like(a)
            b[h // 2, 1:6] = 1
            b[0, 0] = 1
            jobs = [job(1, (1, 2, h + 1, w + 2), 1, (max(h // 2 - 2, 0), 0, h // 2 + 3, 8)), job(1, whole(a), 1, (0, 0, 1, 4)), job(1, whole(b), 1, (1, 2, 2, w + 2), 1)]
            counts = raw_equals_host(a, b, jobs, (1,) if every == 1 else (0, 3))
            assert counts[0, 0] == k and counts[1, 0] == k, (k, every, counts)


def test_target_lists_at_the_size_rule():
    """Boxes of exactly 8192 pixels in which every pixel is a target; one pixel more breaks the rule in the entry and splits in pair_jobs"""
    for H, W, t in ((5, 8192, 1), (6, 4096, 2)):
        b = thick_row(H, W, 2, t)
        a = np.zeros_like(b)
        a[0, 5:9] = 1; a[H - 1, W - 300:W - 1] = 1; a[2, W // 2] = 1
        jobs = [job(1, whole(a), 1, (2, 0, 2 + t, W)), job(1, (2, 0, 2 + t, W), 1, whole(a), 1)[:8] + [0, 0, 1, W, 0]]
        counts = raw_equals_host(a, b, jobs, (0, 3))
        assert counts[0].tolist() == [304, 8192, 0] and counts[1, 0] == 8192
    b = thick_row(5, 8193, 2, 1)
    a = np.zeros_like(b)
    a[0, 5:9] = 1; a[4, 8000:8193] = 1
    counts = raw_equals_host(a, b, [job(1, whole(a), 1, (2, 0, 3, 8193)), job(1, whole(a), 1, (2, 1, 3, 8193))], (0,))
    assert counts.tolist() == [[0, 0, 1], [197, 8192, 0]]
    sa, sb = boxes_of(a, 1), boxes_of(b, 1)
    pj = bd.pair_jobs([(1, 1)], sa, sb, 5, 8193)
    assert pj.jobs[pj.direction == 0][:, 8:12].tolist() == [[2, 0, 3, 8192], [2, 8192, 3, 8193]]
    got = bd.pair_distances(up(a), up(b), [(1, 1)], sa, sb)
    assert got == bd.pair_distances_host(a, b, [(1, 1)], sa, sb) and np.array_equal(got.of(0, 0), unsplit_d2(a, b, 0, 0))
    # the worst case the documents name: one-pixel stripes over 90 x 90, every pixel a border pixel, 4050 targets and as many sources
    s = np.zeros((92, 92), np.int32)
    s[1:91, 1:91] = stripes(90, 90)
    assert raw_equals_host(s, np.roll(s, 1, 1), [job(1, whole(s), 1, (1, 1, 91, 91))], (0, 1))[0].tolist() == [4050, 4050, 0]


@pytest.mark.parametrize("k", [1, 3, 4, 5, 1023])
def test_target_counts_around_the_sixteen_byte_read(k):
    b = np.zeros((9, 1030), np.int32)
    b[4, 3:3 + k] = 1
    a = np.zeros_like(b)
    a[0:2, 0:5] = 1; a[8, 1000:1030] = 1; a[4, 3 + k - 1] = 1
    counts = raw_equals_host(a, b, [job(1, whole(a), 1, whole(b))[:8] + [2, 0, 7, 1030, 0], job(1, whole(b), 1, (0, 0, 2, 1030), 1)])
    assert counts[0, 1] == k and counts[1].tolist() == [k, 10, 0]


def test_frame_as_border_modes_cut_boxes_and_any_id():
    full = np.ones((20, 30), np.int32)                                 # touches all four edges: the frame is its border
    small = np.zeros_like(full)
    small[8:11, 12:20] = 1
    counts = raw_equals_host(full, small, [job(1, whole(full), 1, whole(small)), job(1, whole(small), 1, whole(full), 1)])
    assert counts[0, 0] == 600 and counts[1, 1] == 2 * 30 + 2 * 18
    assert bd.border_counts(up(full), up(small), [job(1, whole(full), 1, whole(small))], 0).cpu().numpy()[0, 0] == 96
    disc, ring = disc_in_ring()
    raw_equals_host(disc, ring, [job(1, whole(disc), 1, whole(ring)), job(1, whole(ring), 1, whole(disc), 1)])
    a, b = blob_maps(70, 131, 12, 7)
    jobs = np.concatenate([all_pair_jobs(a, b, 12), all_pair_jobs(a, b, 12, grow=3),          # both directions in one launch; overhang
                           [job(2, (10, 10, 50, 90), 2, (0, 40, 60, 131)), job(3, (-5, -5, 200, 200), 4, (30, 30, 60, 131), 1),    # cut
                            job(5, whole(a), 6, (0, 0, 60, 131)), job(0, whole(a), 0, (5, 5, 65, 125))]])        # sources of other ids
    counts = raw_equals_host(a, b, jobs)
    assert (counts[:, 0] > 0).sum() > 20
    ids = np.array([0, -1, I32.min, I32.max], np.int64)
    rng = np.random.default_rng(4)
    c = ids[rng.integers(0, 4, (33, 47))].astype(np.int32)
    d = np.roll(c, (2, -1), (0, 1))
    jobs = [job(int(u), whole(c), int(v), (3, 3, 30, 40), k % 2) for k, (u, v) in enumerate((u, v) for u in ids for v in ids)]
    assert (raw_equals_host(c, d, jobs)[:, :2] > 0).all()


def test_far_corners_of_a_two_row_map():
    a = np.zeros((2, 32768), np.int32)
    b = np.zeros_like(a)
    a[0, 0] = 1; b[1, 32767] = 1; a[1, 20000:20003] = 1
    da, db = up(a), up(b)
    jobs = [job(1, whole(a), 1, (0, 32768 - 4096, 2, 32768)), job(1, whole(b), 1, (0, 0, 2, 4096), 1)]
    raw_equals_host(a, b, jobs, (0, 1), da, db)
    got = bd.pair_distances(da, db, [(1, 1)], n_a=1, n_b=1)
    assert got.of(0, 0).tolist() == [1 + 32767 ** 2, 12767 ** 2, 12766 ** 2, 12765 ** 2] and got.of(0, 1).tolist() == [12765 ** 2]
    assert got == bd.pair_distances_host(a, b, [(1, 1)], n_a=1, n_b=1)


def test_three_images_in_one_launch():
    maps = [blob_maps(40, 57, 6, s) for s in (1, 2, 3)]
    a, b = np.stack([m[0] for m in maps]), np.stack([m[1] for m in maps])
    per = [all_pair_jobs(a[i], b[i], 6, grow=1) for i in range(3)]
    for i in range(3):
        per[i][:, 0] = i
    jobs = np.stack(per, 1).reshape(-1, 13)                            # interleaved: image 0, 1, 2, 0, 1, 2, ...
    counts = raw_equals_host(a, b, jobs, (0, 3))
    assert all(counts[i::3, 0].sum() > 0 for i in range(3))


def test_hostile_tables_between_guards():
    a, b = blob_maps(40, 57, 6, 9)
    da, db = up(a), up(b)
    good = all_pair_jobs(a, b, 6)
    bad = [job(1, whole(a), 1, whole(b), img=1), job(1, whole(a), 1, whole(b), img=-1), job(1, whole(a), 1, whole(b), img=I32.max),
           job(1, (30, 5, 10, 50), 1, whole(b)), job(1, whole(a), 1, (5, 50, 30, 10)), job(1, (I32.max, I32.max, I32.min, I32.min), 1, whole(b))]
    for mode in (0, 3):
        n0, n2 = (int(v) for v in bd.border_d2_host(a, b, good[[0, 2]], mode)[0][:, 0])
        D = n0 + n2 + 60                                               # laid out so that no two jobs store into one slot
        assert n0 > 3 and n2 > 0
        g0, g2 = good[0].tolist()[:12], good[2].tolist()[:12]
        table = np.array(bad + [g0 + [-2], g0 + [D - 1], g0 + [D], g0 + [I32.max], g0 + [I32.min], g2 + [n0 + 10]], np.int64)
        want = bd.border_d2_store_host(a, b, table, mode, D, fill=-9)
        assert (want != -9).sum() == n0 - 2 + 1 + n2 and want[D - 1] != -9 and want[n0 - 2] == -9
        jd = up(table.astype(np.int32))
        guard = torch.full((D + 2,), -9, dtype=torch.int32, device=DEV)
        with torch.cuda.device(DEV):
            _lib.call("kg_label_border_d2", _lib.ptr(da), _lib.ptr(db), 1, *a.shape, _lib.ptr(jd), len(table), mode, _lib.ptr(guard[1:]), D, _lib.stream_ptr())
        got = guard.cpu().numpy()
        assert got[0] == -9 and got[-1] == -9 and np.array_equal(got[1:-1], want)
        cnt = torch.full((len(table) + 2, 3), -9, dtype=torch.int32, device=DEV)
        with torch.cuda.device(DEV):
            _lib.call("kg_label_border_counts", _lib.ptr(da), _lib.ptr(db), 1, *a.shape, _lib.ptr(jd), len(table), mode, _lib.ptr(cnt[1:]), _lib.stream_ptr())
        got = cnt.cpu().numpy()
        assert (got[[0, -1]] == -9).all() and np.array_equal(got[1:-1], bd.border_d2_host(a, b, table, mode)[0]) and not got[1:7].any()
    with pytest.raises(E):
        bd.border_d2(da, db, table, 0, D, da.view(-1)[:D])                                                  # out aliases a map
    with pytest.raises(E):
        bd.border_counts(da, db[:, :-1], table)
    with pytest.raises(E):
        bd.border_counts(da, db, table, 4)
    with pytest.raises(E):
        bd.pair_distances(a, b, [(1, 1)], n_a=6, n_b=6)                                                     # host maps: the host route is named
    assert bd.border_counts(da, db, np.zeros((0, 13), np.int64)).shape == (0, 3) and len(bd.pair_distances(da, db, [], n_a=6, n_b=6)) == 0


def test_more_jobs_than_the_grid_cap():
    """1 048 584 one-pixel jobs: the grid strides.  The table repeats 72 distinct jobs, so the host states 72 and the rest follows."""
    a = np.zeros((8, 9), np.int32)
    b = np.zeros_like(a)
    a[::2, ::2] = 1; b[1::3, 1::2] = 1
    ys, xs = np.nonzero(a == 1)
    yt, xt = np.nonzero(b == 1)
    base = np.array([job(1, (ys[k % len(ys)], xs[k % len(ys)], ys[k % len(ys)] + 1, xs[k % len(ys)] + 1), 1,
                         (yt[k % len(yt)], xt[k % len(yt)], yt[k % len(yt)] + 1, xt[k % len(yt)] + 1)) for k in range(72)], np.int64)
    base[5, 8:12] = [0, 0, 1, 1]                                       # a target box without a target: -1
    want_c, want_v = bd.border_d2_host(a, b, base)
    assert want_c[:, 0].tolist() == [1] * 72 and want_c[5].tolist() == [1, 0, 0]
    m = (1 << 20) + 8
    table = np.tile(base, (m // 72 + 1, 1))[:m].astype(np.int32)
    table[:, 12] = np.arange(m)
    da, db, jd = up(a), up(b), up(table)
    cnt = bd.border_counts(da, db, jd).cpu().numpy()
    assert np.array_equal(cnt, np.tile(want_c, (m // 72 + 1, 1))[:m])
    out = torch.full((m,), -7, dtype=torch.int32, device=DEV)
    bd.border_d2(da, db, jd, 0, m, out)
    assert np.array_equal(out.cpu().numpy(), np.tile(np.concatenate(want_v), m // 72 + 1)[:m])


def test_a_300_by_300_pair_through_the_bands():
    a, b = ellipse_pair(300)
    sa, sb = boxes_of(a, 1), boxes_of(b, 1)
    da, db = up(a), up(b)
    want = bd.pair_distances_host(a, b, [(1, 1)], sa, sb, max_job_pixels=4096)
    for cap in (4096, 65536):
        got = bd.pair_distances(da, db, [(1, 1)], sa, sb, max_job_pixels=cap)
        assert got == want and all(np.array_equal(got.of(0, d), unsplit_d2(a, b, 0, d)) for d in (0, 1))
    small_a, small_b = ellipse_pair(110)
    for sources, targets in (("all", "border"), ("all", "region"), ("border", "region")):
        got = bd.pair_distances(up(small_a), up(small_b), [(1, 1)], n_a=1, n_b=1, sources=sources, targets=targets, max_job_pixels=4096)
        assert got == bd.pair_distances_host(small_a, small_b, [(1, 1)], n_a=1, n_b=1, sources=sources, targets=targets)
        mode = bd.mode_of("t", sources, targets)
        assert all(np.array_equal(got.of(0, d), unsplit_d2(small_a, small_b, mode, d)) for d in (0, 1))


# ---- end to end -------------------------------------------------------------------------------------------------------------------------

def same(a, b):
    if a is None or b is None:
        return a is b
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


@pytest.fixture(scope="module")
def cal_model():
    from oracle import weightgen
    m = KGnet.resnet50(pretrained=False)
    m.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    return m.to(DEV).eval()


@pytest.mark.parametrize("clean", [None, dict(min_area=4)])
def test_evaluator_with_boundary_on_the_device_equals_the_host_route(cal_model, clean):
    H, W, S = 400, 600, 256
    img = np.random.default_rng(8).integers(0, 256, (H, W, 3), dtype=np.uint8)
    r = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4, clean=clean)
    n = len(r)
    lab = r.labels.cpu().numpy()
    gt = np.roll(lab, (2, 1), (0, 1))                                  # the prediction shifted: most ids stay true positives
    for option in (True, dict(tolerance=1, sources="all", targets="region")):
        ev, host = lm.LabelEvaluator(boundary=option), lm.LabelEvaluator(boundary=option)
        c = ev.add(r, (up(gt), n))
        ch = host.add((lab, n), (gt, n), r.dets[:, 4])
        got, want = ev.summary(), host.summary()
        assert c == ch and list(got) == list(want) and all(same(got[k], want[k]) for k in got), (got, want)
        assert got["boundary_pairs"] == lm.panoptic(c)["tp"] > 10 and 0 < got["nsd"] <= 1 and 0 < got["assd"] <= got["hd"] < np.inf
    print({k: got[k] for k in ("hd", "hd95", "assd", "nsd", "boundary_pairs")}, "instances", n)
    plain = lm.LabelEvaluator()
    plain.add(r, (up(gt), n))
    assert all(same(plain.summary()[k], got[k]) for k in plain.summary())
    s = lm.evaluate_tiled(cal_model, [(img, (gt, n))], tile=S, overlap=64, batch=4, clean=clean, boundary=option)
    assert all(same(s[k], got[k]) for k in got)
