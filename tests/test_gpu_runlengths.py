"""GPU: run-length lists on the device (csrc/runlengths.hip, runlengths.py) against the host statements of the same semantics
(runlengths.runs_host, run_counts_host, run_rows_host, paint_host) and against instances.rle_encode.  Every comparison is exact integer
equality.  Shapes are the smallest at which the kernel can go wrong: one-pixel, one-row and one-column maps, runs that wrap from one
column into the next, box heights and widths on both sides of the wave and of the 256-position chunk, maps where every pixel is a run,
unsplit boxes of more than one tile of columns on both branches of the tile choice (a pitch of at most one dword, an odd number of dwords),
column bands whose heads and tails fall into different bands, any int32 as an id, tables with wrong offsets, more than one image in a
launch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from kg_instance_segmentation_amd import KGnet, _lib, inference, instances, tiling  # noqa: E402
from kg_instance_segmentation_amd import components as cc  # noqa: E402
from kg_instance_segmentation_amd import distance as dt  # noqa: E402
from kg_instance_segmentation_amd import measure as ms  # noqa: E402
from kg_instance_segmentation_amd import runlengths as rl  # noqa: E402

DEV = "cuda"
I32 = np.iinfo(np.int32)
E = _lib.KGLibraryError


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


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
    flat = np.zeros(12, np.int32)
    flat[[2, 3, 4, 5, 7, 8]] = 5
    return np.ascontiguousarray(flat.reshape(3, 4).T)


def table_of(jobs, counts):
    """jobs [m, 6] and their {heads, tails} -> the [m, 8] table of kg_label_runs and R"""
    c = np.asarray(counts, np.int64).reshape(-1, 2)
    return np.concatenate([np.asarray(jobs, np.int64).reshape(-1, 6), np.cumsum(c, 0) - c], 1), int(c.sum(0).max()) if len(c) else 0


def raw_equals_host(lab, d, jobs):
    """Both raw entries on jobs [m, 6] (boxes may cut runs) against their NumPy statements; -> the counts"""
    want = rl.run_counts_host(lab, jobs)
    got = rl.run_counts(d, jobs)
    assert got.is_cuda and got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    table, R = table_of(jobs, want)
    out = torch.full((R, 2), -7, dtype=torch.int32, device=DEV)
    assert rl.run_rows(d, table, R, out) is out
    assert np.array_equal(out.cpu().numpy(), rl.run_rows_host(lab, table, R, fill=-7))
    return want


def same_as_rle_encode(lab, got, ids):
    want = instances.rle_encode(lab, ids=ids)
    assert isinstance(got, rl.RunLengths) and len(got) == len(ids) and got.first.dtype == np.int64
    for k, i in enumerate(ids):
        assert np.array_equal(got.of(k), want[int(i)]), (k, i)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 130), (130, 1)])
def test_smallest_maps(H, W):
    n = 6
    lab = np.ones((1, 1), np.int32) if H * W == 1 else blob_map(H, W, n, 10 + H)
    want = rl.runs_host(lab, n)
    d = up(lab)
    got = rl.runs(d, n)
    assert got == want and (got.H, got.W) == (H, W) and want.counts().any()
    same_as_rle_encode(lab, got, range(1, n + 1))
    assert rl.runs(d, n, max_job_pixels=1) == want
    raw_equals_host(lab, d, [[0, 1, 0, 0, H, W], [0, 0, 0, 0, H, W], [0, 1, 0, 0, 1, 1], [0, 1, H - 1, W - 1, H, W]])
    assert torch.equal(rl.paint(want, H, W, DEV), d)


def test_wrap_example_and_one_id_map():
    lab = wrap_map()
    d = up(lab)
    got = rl.runs(d, jobs=[[0, 5, 0, 0, 4, 3], [0, 0, 0, 0, 4, 3]])
    assert got.string(0) == "3 4 8 2" and got.coco(0)["counts"] == [2, 4, 1, 2, 3] and got == rl.runs_host(lab, [[0, 5, 0, 0, 4, 3], [0, 0, 0, 0, 4, 3]])
    assert raw_equals_host(lab, d, [[0, 5, 0, 0, 3, 3], [0, 5, 1, 1, 4, 2]]).tolist() == [[1, 2], [1, 1]]      # boxes that cut runs
    for cut in ([[0, 5, 0, 0, 3, 3]], [[0, 5, 1, 1, 4, 2]]):         # unequal counts; a tail in front of its head
        with pytest.raises(E):
            rl.runs(d, jobs=cut)
        with pytest.raises(E):
            rl.runs_host(lab, cut)
    H, W = 70, 131
    one = np.full((H, W), 3, np.int32)
    d = up(one)
    job = [[0, 3, 0, 0, H, W]]
    assert rl.runs(d, jobs=job).of(0).tolist() == [[1, H * W]]                               # unsplit: a single run of H * W
    pieces, owner = rl.split_columns(job, 210)                        # bands of 3 columns
    assert len(pieces) == 44 and (pieces[:-1, 5] - pieces[:-1, 3] == 3).all() and pieces[-1, 3:].tolist() == [129, H, W]
    cnt = rl.run_counts(d, pieces).cpu().numpy()
    assert cnt.tolist() == [[1, 0]] + [[0, 0]] * 42 + [[0, 1]]        # the head and the tail lie in different bands
    assert rl.runs(d, jobs=job, max_job_pixels=210).of(0).tolist() == [[1, H * W]]
    assert rl.runs(d, 3, max_job_pixels=H).counts().tolist() == [0, 0, 1]


@pytest.fixture(scope="module")
def blobs():
    H, W, n = 70, 131, 40
    lab = blob_map(H, W, n, 170)
    return lab, up(lab), n, rl.runs_host(lab, n)


def test_blobs_every_job_source(blobs):
    lab, d, n, want = blobs
    H, W = lab.shape
    cols = want.first // H
    per_col = np.zeros((n, W), np.int64)
    np.add.at(per_col, (want.rows(), cols), 1)
    assert per_col.max() > 1 and (want.counts() == 0).any()           # some id has more than one run in a column, some id is empty
    same_as_rle_encode(lab, want, range(1, n + 1))
    assert rl.runs(d, n) == want                                      # boxes from label_stats
    stats = ms.labelmetrics.label_stats_host(lab, n)
    assert rl.runs(d, n, stats=stats) == want                         # boxes given
    jobs = ms.jobs_from_stats(stats)
    for cap in (2 ** 30, 65536, 500, 70, 1):
        assert rl.runs(d, jobs=jobs, max_job_pixels=cap) == want      # host jobs, unsplit and in bands down to one column
    table, R = table_of(jobs, rl.run_counts_host(lab, jobs))
    assert R == len(want.first)
    cnt = rl.run_counts(d, up(jobs.astype(np.int32)))                 # the raw entries: device jobs, rows stay on the device
    rows = rl.run_rows(d, up(table.astype(np.int32)), R)
    assert cnt.is_cuda and rows.is_cuda and rows.dtype == torch.int32 and rows.shape == (R, 2)
    assert np.array_equal(cnt.cpu().numpy()[:, 0], want.counts()) and np.array_equal(cnt.cpu().numpy()[:, 1], want.counts())
    assert np.array_equal(rows.cpu().numpy()[:, 0], want.first) and np.array_equal(rows.cpu().numpy()[:, 1], want.last)
    whole = np.array([[0, i, 0, 0, H, W] for i in range(0, n + 2)])   # the whole map as every id's box, the background and an absent id too
    got = rl.runs(d, jobs=whole)
    assert got == rl.runs_host(lab, whole) and got.slice(1, n + 1) == want and got.counts()[n + 1] == 0
    assert torch.equal(rl.paint(want, H, W, DEV), d)                  # and back


STRIPES = np.ones((300, 300), np.int32)
STRIPES[1::2] = 2                                                     # one-pixel horizontal stripes: every pixel is a run


@pytest.mark.parametrize("w", [1, 255, 256, 257])
def test_box_heights_and_widths_on_stripes(w):
    lab, d = STRIPES, up(STRIPES)
    jobs = np.array([[0, v, 3, 6, 3 + h, 6 + w] for h in (1, 63, 64, 65, 255, 256, 257) for v in (1, 2)])
    cnt = raw_equals_host(lab, d, jobs)
    assert np.array_equal(cnt[:, 0], cnt[:, 1]) and cnt[0].tolist() == [0, 0] and cnt[1].tolist() == [w, w]
    assert cnt[-2].tolist() == [128 * w, 128 * w] and cnt[-1].tolist() == [129 * w, 129 * w]
    got = rl.runs(d, jobs=jobs, max_job_pixels=2 ** 30)               # nothing split: the kernel's own tiles and chunks
    assert got == rl.runs_host(lab, jobs) and np.array_equal(got.first, got.last)
    assert rl.runs(d, jobs=jobs, max_job_pixels=4096) == got


def test_stripes_as_one_box():
    lab, d = STRIPES, up(STRIPES)
    jobs = [[0, 1, 0, 0, 300, 300], [0, 2, 0, 0, 300, 300]]
    want = rl.runs_host(lab, jobs)
    assert want.counts().tolist() == [45000, 45000] and np.array_equal(want.first, want.last)
    assert rl.runs(d, jobs=jobs, max_job_pixels=2 ** 30) == want
    assert rl.runs(d, jobs=jobs, max_job_pixels=4096) == want
    assert rl.runs(d, 2) == want
    assert torch.equal(rl.paint(want, 300, 300, DEV), d)


@pytest.mark.parametrize("H,W", [(1400, 100), (500, 700)])
def test_unsplit_boxes_of_more_than_one_tile(H, W):
    """A box the kernel walks in several tiles of columns: the bitmap is refilled behind a barrier, the carry of heads and tails and the
    parity of the wave totals run on across the tiles, the last tile is narrower, and the wrap neighbours of a tile's first and last
    column lie outside it.  1400 x 100: 1402 rows leave 93 bits per row, so tiles of 32 columns at a pitch of 32 bits (32, 32, 32, 4;
    the 1395 x 88 box 32, 32, 24).  500 x 700: tiles of 224 columns at a pitch of 7 dwords (224, 224, 224, 28)."""
    lab = np.random.default_rng(H).integers(0, 3, (H // 4 + 1, W)).repeat(4, 0)[:H].astype(np.int32)      # vertical pieces of about 4 pixels
    d = up(lab)
    cnt = raw_equals_host(lab, d, [[0, 1, 0, 0, H, W], [0, 2, 0, 0, H, W], [0, 1, 3, 5, H - 2, W - 7], [0, 2, 1, 0, H, W], [0, 0, 7, 1, H, W - 1]])
    assert cnt.min() > H * W // 40 and (cnt[2, 0] != cnt[2, 1] or cnt[3, 0] != cnt[3, 1] or cnt[4, 0] != cnt[4, 1])       # boxes from y1 > 0 cut runs
    whole = np.array([[0, v, 0, 0, H, W] for v in (1, 2, 0)])
    want = rl.runs_host(lab, whole)
    same_as_rle_encode(lab, want.slice(0, 2), [1, 2])
    assert rl.runs(d, jobs=whole, max_job_pixels=2 ** 30) == want     # nothing split: the kernel's own tiles
    assert rl.runs(d, jobs=whole) == want                             # and in bands of 65536 pixels
    assert torch.equal(rl.paint(want.slice(0, 2), H, W, DEV), d)


@pytest.mark.parametrize("H", [67, 66])
def test_checkerboard(H):
    W = 69
    lab = ((np.add.outer(np.arange(H), np.arange(W)) % 2) + 1).astype(np.int32)
    d = up(lab)
    want = rl.runs_host(lab, 2)
    # down a column every pixel is its own run; an even H joins the bottom of a column to the top of the next, an odd H does not
    assert want.counts().sum() == H * W - (W - 1) * (H % 2 == 0) and (want.last - want.first).max() == (H % 2 == 0)
    same_as_rle_encode(lab, want, [1, 2])
    for cap in (2 ** 30, 65536, 1000, H, 1):
        assert rl.runs(d, 2, max_job_pixels=cap) == want
    raw_equals_host(lab, d, [[0, 1, 0, 0, H, W], [0, 2, 1, 1, H - 1, W - 1], [0, 1, 0, 5, H, 6], [0, 2, H - 1, 0, H, W]])
    assert torch.equal(rl.paint(want, H, W, DEV), d)


def test_ids_are_compared_only():
    ids = [0, -1, I32.min, I32.max]
    rng = np.random.default_rng(4)
    lab = np.array(ids + [7], np.int32)[rng.integers(0, 5, (37, 45))]
    d = up(lab)
    jobs = np.array([[0, v, 0, 0, 37, 45] for v in ids + [8]], np.int64)
    want = rl.runs_host(lab, jobs)
    assert (want.counts()[:4] > 0).all() and want.counts()[4] == 0
    assert rl.runs(d, jobs=jobs) == want and rl.runs(d, jobs=jobs, max_job_pixels=37) == want
    for k, v in enumerate(ids):
        assert np.array_equal(rl.paint_host(want.slice(k, k + 1), 37, 45, ids=[1]) != 0, lab == v)
    back = rl.paint(want.slice(0, 4), 37, 45, DEV, background=7, ids=ids)
    assert torch.equal(back, d)


def test_three_images_in_one_launch():
    H, W = 40, 67
    ns = [7, 0, 12]
    lab = np.stack([blob_map(H, W, 7, 1), np.zeros((H, W), np.int32), blob_map(H, W, 12, 2)])
    want = rl.runs_host(lab, ns)
    assert len(want) == 19 and want.counts()[:7].any() and want.counts()[7:].any()
    d = up(lab)
    assert rl.runs(d, ns) == want and rl.runs(d, ns, max_job_pixels=100) == want
    stats = [ms.labelmetrics.label_stats_host(lab[i], ns[i]) for i in range(3)]
    jobs = np.concatenate([ms.jobs_from_stats(s, i) for i, s in enumerate(stats)])
    order = np.random.default_rng(3).permutation(len(jobs))          # jobs interleaved across the images
    got = rl.runs(d, jobs=jobs[order], max_job_pixels=300)
    assert got == rl.runs_host(lab, jobs[order])
    assert all(np.array_equal(got.of(k), want.of(o)) for k, o in enumerate(order))
    for i in (0, 2):
        same_as_rle_encode(lab[i], rl.runs(d[i], ns[i]), range(1, ns[i] + 1))


def test_wrong_tables_between_guard_rows():
    """These tables check the clamps and the store predicate; the result is run_rows_host's, sentinel included."""
    H, W, nimg = 33, 47, 2
    lab = np.stack([blob_map(H, W, 9, 5), blob_map(H, W, 9, 6)])
    d = up(lab)
    full = [0, 5, 0, 0, H, W]
    heads5 = int(rl.run_counts_host(lab, [full])[0, 0])
    assert heads5 >= 3
    R = 40
    # no two jobs name the same slot of a column: heads 1 .. 19, 20 .. 25, 0, 39, 35; tails 1 .. 19, 20 .. 25, 30 .. 32, 35
    table = np.array([[0, 5, -50, -50, H + 50, W + 50, 1, 1],                                  # an oversized box is clamped
                      [-1, 5, 0, 0, H, W, 0, 0], [nimg, 5, 0, 0, H, W, 0, 0], [I32.max, 5, 0, 0, H, W, 1, 1], [I32.min, 5, 0, 0, H, W, 2, 2],
                      [0, 5, 20, 30, 10, 40, 0, 0], [0, 5, 10, 40, 20, 30, 0, 0], [0, 5, 5, 5, 5, 9, 0, 0],   # inverted, inverted, empty
                      [0, 4, I32.min, I32.min, I32.max, I32.max, 20, 20],
                      [1, 3, 0, 0, H, W, -2, 30],                                               # head_at negative: the first two heads are dropped
                      [1, 4, 0, 0, H, W, I32.min, I32.min],
                      [0, 5, 0, 0, H, W, R - 1, R + 5],                                         # head_at at R - 1 with >= 3 heads: one is stored
                      [0, 5, 0, 0, H, W, R, I32.max],                                           # beyond R
                      [1, 6, H - 1, W - 1, H + 9, W + 9, 35, 35], [1, 6, H, W, H + 9, W + 9, 0, 0],
                      [0, 77, 0, 0, H, W, 0, 0]], np.int64)
    want = rl.run_rows_host(lab, table, R, fill=-7)
    assert (want == -7).any() and (want[:, 0] != -7).any() and want[R - 1, 0] != -7
    guard = torch.full((R + 2, 2), -7, dtype=torch.int32, device=DEV)                          # rows in front of and behind the output
    from kg_instance_segmentation_amd._lib import ptr, stream_ptr
    dj = up(table.astype(np.int32))
    _lib.call("kg_label_runs", ptr(d), nimg, H, W, ptr(dj), len(table), ptr(guard[1:]), R, stream_ptr())
    g = guard.cpu().numpy()
    assert np.array_equal(g[1:-1], want) and (g[0] == -7).all() and (g[-1] == -7).all()
    cnt = torch.full((len(table) + 2, 2), -7, dtype=torch.int32, device=DEV)
    _lib.call("kg_label_run_counts", ptr(d), nimg, H, W, ptr(up(table[:, :6].astype(np.int32))), len(table), ptr(cnt[1:]), stream_ptr())
    c = cnt.cpu().numpy()
    assert np.array_equal(c[1:-1], rl.run_counts_host(lab, table[:, :6])) and (c[0] == -7).all() and (c[-1] == -7).all()
    assert not c[2:5].any() and not c[6:9].any() and c[1, 0] == heads5 and not c[-3:-1].any()
    # m == 0 and R == 0 launch nothing
    assert rl.run_counts(d, np.zeros((0, 6), np.int64)).shape == (0, 2) and rl.run_rows(d, np.zeros((0, 8), np.int64), 0).shape == (0, 2)
    assert rl.run_rows(d, table, 0).shape == (0, 2) and len(rl.runs(d, jobs=np.zeros((0, 6), np.int64))) == 0
    with pytest.raises(E):
        rl.runs(d.to(torch.int64), [3, 3])
    with pytest.raises(E):
        rl.run_rows(d, table, -1)
    with pytest.raises(E):
        _lib.call("kg_label_runs", ptr(d), nimg, H, W, ptr(dj), 1, ptr(d), 4, stream_ptr())  # out aliases labels
    with pytest.raises(E):
        _lib.call("kg_label_run_counts", ptr(d), 0, H, W, ptr(dj), 1, ptr(cnt), stream_ptr())
    with pytest.raises(E):
        _lib.call("kg_runs_paint", None, 1, H, W, 0, ptr(cnt), stream_ptr())


@pytest.mark.parametrize("H,W", [(1, 1), (37, 70), (300, 257)])
def test_paint(H, W):
    n = 1 if H * W == 1 else 25
    lab = np.ones((1, 1), np.int32) if H * W == 1 else blob_map(H, W, n, 20 + H)
    d = up(lab)
    r = rl.runs(d, n)
    assert torch.equal(rl.paint(r, H, W, DEV), d)                                              # paint(runs(lab)) == lab on the device
    enc = instances.rle_encode(lab)
    got = rl.paint(enc, H, W, DEV)
    assert got.is_cuda and got.dtype == torch.int32 and got.shape == (H, W) and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy(), instances.rle_decode(enc, H, W))
    shuffled = {k: enc[k] for k in np.random.default_rng(1).permutation(list(enc)).tolist()}   # the host sorts
    ids = np.random.default_rng(2).permutation(n) + 100
    assert np.array_equal(rl.paint(shuffled, H, W, DEV, background=-5).cpu().numpy(), np.where(lab > 0, lab, -5))
    assert np.array_equal(rl.paint(r, H, W, DEV, background=I32.min, ids=ids).cpu().numpy(), rl.paint_host(r, H, W, background=I32.min, ids=ids))
    assert np.array_equal(rl.paint({}, H, W, DEV, background=9).cpu().numpy(), np.full((H, W), 9))        # R == 0
    assert np.array_equal(rl.paint({I32.max: [[1, H * W]]}, H, W, DEV).cpu().numpy(), np.full((H, W), I32.max))    # one run covers the image
    with pytest.raises(E):
        rl.paint({1: [[1, 1]], 2: [[1, 1]]}, H, W, DEV)
    with pytest.raises(E):
        rl.paint({1: [[H * W, 2]]}, H, W, DEV)
    with pytest.raises(E):
        rl.paint(enc, H, W, "cpu")


# ---- end to end -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cal_model():
    from oracle import weightgen
    m = KGnet.resnet50(pretrained=False)
    m.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    return m.to(DEV).eval()


def same_instances(a, b):
    return (torch.equal(a.labels, b.labels) and np.array_equal(a.dets, b.dets) and np.array_equal(a.table, b.table) and type(a) is type(b)
            and a.table.dtype == b.table.dtype)


def runs_match_rle_encode(inst):
    n = len(inst)
    lab = inst.labels.cpu().numpy()
    want = instances.rle_encode(lab, ids=range(1, n + 1))
    assert isinstance(inst.runs, rl.RunLengths) and len(inst.runs) == n and (inst.runs.H, inst.runs.W) == lab.shape
    assert all(np.array_equal(inst.runs.of(k), want[k + 1]) for k in range(n))
    assert np.array_equal(inst.runs.areas(), np.asarray(inst.table)[:, 1])


def test_predict_tiled_with_runs(cal_model):
    H, W, S = 400, 600, 256
    img = np.random.default_rng(8).integers(0, 256, (H, W, 3), dtype=np.uint8)
    plain = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4)
    got = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4, runs=True)
    n = len(plain)
    print("instances", n, "runs", len(got.runs.first))
    assert n > 0 and plain.runs is None and plain.neighbours is None and same_instances(got, plain)      # the default path is untouched
    runs_match_rle_encode(got)
    assert torch.equal(rl.paint(got.runs, H, W, got.labels.device), got.labels)
    assert len(rl.submission_rows("img", got.runs)) == int((np.asarray(got.table)[:, 1] > 0).sum())
    host = tiling.TiledInstances(got.labels.cpu().numpy(), got.dets, got.table, got.tile, got.origin, None)      # a host map goes through runs_host
    assert rl.runs_instances(host) == got.runs and rl.runs_instances(got, max_job_pixels=64) == got.runs
    policy = dict(min_area=4)
    final = dt.expand_instances(cc.clean_instances(plain, **policy), 3)
    both = tiling.predict_tiled(cal_model, up(img), tile=S, overlap=64, batch=4, clean=policy, expand=3, runs=dict(max_job_pixels=200))
    assert same_instances(both, final) and both.neighbours is None
    runs_match_rle_encode(both)                                       # taken last, on the cleaned and expanded map


def test_predict_instances_with_runs(cal_model):
    S = 256
    src = np.random.default_rng(9).integers(0, 256, (2, S, S, 3), dtype=np.uint8)
    x = torch.cat([tiling.cut_tiles(src[i], tiling.plan(S, S, S, 64)) for i in range(2)])
    plain = inference.predict_instances(cal_model, x)
    assert all(p is not None and len(p) > 0 and p.runs is None for p in plain)
    assert all(p.runs is None for p in inference.predict_instances(cal_model, x, runs=None, measure=True))
    got = inference.predict_instances(cal_model, x, runs=True)
    full = inference.predict_instances(cal_model, x, clean=dict(min_area=4), expand=2, runs=True)
    assert len(got) == len(full) == 2
    for p, g, f in zip(plain, got, full):
        assert same_instances(p, g) and len(f) == len(p)
        runs_match_rle_encode(g)
        runs_match_rle_encode(f)
