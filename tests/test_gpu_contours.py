"""GPU: instance outlines on the device (csrc/contours.hip, contours.py) against the host statement of the same semantics
(contours.contours_host).  Every comparison is exact integer equality.  Shapes are the smallest at which the kernel can go wrong: one-pixel,
one-row and one-column maps, box widths on both sides of the 32 / 64 / 96-bit pitch, box heights around the 256-row fill chunk, vertex
counts around the 256-position scan chunk, walks where most candidates abort (diamond), one long ring (comb), many rings with pinch
vertices (checkerboard), any int32 as an id, boxes that cut their id or reach beyond the map, tables with wrong offsets, more than one
image in a launch, and both sides of the size rule."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from kg_instance_segmentation_amd import KGnet, _lib, inference, tiling  # noqa: E402
from kg_instance_segmentation_amd import components as cc  # noqa: E402
from kg_instance_segmentation_amd import contours as ct  # noqa: E402
from kg_instance_segmentation_amd import distance as dt  # noqa: E402
from kg_instance_segmentation_amd import measure as ms  # noqa: E402

DEV = "cuda"
I32 = np.iinfo(np.int32)
E = _lib.KGLibraryError


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def random_mask(H, W, seed, density=0.6):
    return (np.random.default_rng(seed).random((H, W)) < density).astype(np.int32)


def whole(lab, ids=(1,), img=0):
    H, W = lab.shape[-2:]
    return np.array([[img, int(i), 0, 0, H, W] for i in ids], np.int64).reshape(-1, 6)


def clamped_hw(jobs, H, W):
    j = np.asarray(jobs, np.int64).reshape(-1, 6)
    return np.maximum(np.minimum(j[:, 4], H) - np.maximum(j[:, 2], 0), 0), np.maximum(np.minimum(j[:, 5], W) - np.maximum(j[:, 3], 0), 0)


def same_as_host(lab, jobs, d=None):
    """contours and the raw count entry on host jobs [m, 6] against contours_host; -> the host result"""
    d = up(lab) if d is None else d
    want = ct.contours_host(lab, jobs)
    got = ct.contours(d, jobs=jobs)
    assert isinstance(got, ct.Contours) and got == want and got.verts.dtype == np.int32
    cnt = ct.contour_counts(d, jobs)
    assert cnt.is_cuda and cnt.dtype == torch.int64 and cnt.shape == (len(want), 4)
    cnt = cnt.cpu().numpy()
    nimg, H, W = (1,) + lab.shape if lab.ndim == 2 else lab.shape
    j = np.asarray(jobs, np.int64).reshape(-1, 6)
    h, w = clamped_hw(j, H, W)
    live = (j[:, 0] >= 0) & (j[:, 0] < nimg) & (h > 0) & (w > 0)
    status = np.array([lv and not ct.fits(a, b) for lv, a, b in zip(live.tolist(), h.tolist(), w.tolist())], np.int64)
    assert np.array_equal(cnt[:, 3], status)
    on_device = status == 0
    verts = np.zeros(len(want), np.int64)
    np.add.at(verts, want.rows(), want.count)
    for col, ref in enumerate((want.counts(), verts, want.perimeters())):
        assert np.array_equal(cnt[:, col], np.where(on_device, ref, 0)), col
    return want


# ---- smallest maps and pitch boundaries -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", [(1, 1), (1, 130), (130, 1)])
def test_smallest_maps(H, W):
    lab = np.ones((1, 1), np.int32) if H * W == 1 else random_mask(H, W, 10 + H)
    want = same_as_host(lab, [[0, 1, 0, 0, H, W], [0, 0, 0, 0, H, W], [0, 1, 0, 0, 1, 1], [0, 1, H - 1, W - 1, H, W], [0, 2, 0, 0, H, W]])
    assert want.counts()[0] > 0 and want.counts()[4] == 0
    if H * W == 1:
        assert want.of(0)[0].tolist() == [[0, 0], [0, 1], [1, 1], [1, 0]] and want.perimeter[0] == 4 and want.area2[0] == 2


@pytest.mark.parametrize("w", [29, 30, 31, 61, 62, 63, 94])
def test_box_widths_across_the_pitch(w):
    """w + 2 crosses 32, 64 and 96 bits: the pitch goes from 1 to 3 dwords (never 2) and, at 94 + 2 = 96, stays at 3"""
    H, W = 11, w + 5
    lab = random_mask(H, W, w)
    lab[:, 2] = lab[:, w + 1] = 1                                     # the box's first and last column hold the id
    same_as_host(lab, [[0, 1, 0, 2, H, 2 + w], [0, 1, 1, 2, H - 1, 2 + w], [0, 0, 0, 2, H, 2 + w], [0, 1, 0, 0, H, W]])


@pytest.mark.parametrize("h", [1, 254, 255, 256])
def test_box_heights_at_width_three(h):
    H, W = h + 3, 6
    lab = random_mask(H, W, h, 0.7)
    same_as_host(lab, [[0, 1, 2, 1, 2 + h, 4], [0, 0, 2, 1, 2 + h, 4], [0, 1, 0, 0, H, W]])


@pytest.mark.parametrize("h,w", [(14, 16), (15, 15), (5, 42), (1, 128), (26, 18)])
def test_vertex_counts_across_the_scan_chunk(h, w):
    """(h + 1)(w + 1) = 255, 256, 258, 258 and 513 vertex positions (257 is prime, so no box has it; 258 stands in, as a flat and as a
    one-row box): a last chunk that is full, one short and two long.  Single pixels in the corners of the last row give ring starts at the
    positions (h - 1)(w + 1) and (h - 1)(w + 1) + w - 1; with 513 positions they lie in the second chunk, behind the rings that start in
    the first, so their ring slot and vertex offset hold the carry across the chunks."""
    nv = (h + 1) * (w + 1)
    assert nv in (255, 256, 258, 513)
    lab = random_mask(h, w, h * w, 0.5)
    lab[-1, :] = 0
    lab[-1, -1] = lab[-1, 0] = 1
    if h > 1:
        lab[-2, -1] = lab[-2, 0] = 0
    want = same_as_host(lab, whole(lab, [1, 0]))
    at = [int(r[0][0]) * (w + 1) + int(r[0][1]) for r in want.of(0)]
    assert (h - 1) * (w + 1) in at and (h - 1) * (w + 1) + w - 1 in at and at == sorted(at)
    if nv > 512:
        assert min(at) < 256 <= (h - 1) * (w + 1) and sum(a < 256 for a in at) > 3


# ---- ownership walks --------------------------------------------------------------------------------------------------------------------

def diamond(r):
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    return (np.abs(yy) + np.abs(xx) <= r).astype(np.int32)


def comb(n):
    lab = np.zeros((n, n), np.int32)
    lab[:, ::2] = 1
    lab[0, :] = 1
    return lab


def spiral(n):
    lab = np.zeros((n, n), np.int32)
    y, x, dy, dx = 0, 0, 0, 1
    lab[0, 0] = 1
    for _ in range(n * n):
        ny, nx = y + dy, x + dx
        ahead = (ny + dy, nx + dx)
        if not (0 <= ny < n and 0 <= nx < n) or (0 <= ahead[0] < n and 0 <= ahead[1] < n and lab[ahead] == 1):
            dy, dx = dx, -dy
            ny, nx = y + dy, x + dx
            ahead = (ny + dy, nx + dx)
            if not (0 <= ny < n and 0 <= nx < n) or lab[ny, nx] == 1 or (0 <= ahead[0] < n and 0 <= ahead[1] < n and lab[ahead] == 1):
                break
        y, x = ny, nx
        lab[y, x] = 1
    return lab


NESTED = np.array([[1, 1, 1, 1, 1], [1, 0, 0, 0, 1], [1, 0, 1, 0, 1], [1, 0, 0, 0, 1], [1, 1, 1, 1, 1]], np.int32)


def test_diamond_where_most_candidates_abort():
    lab = np.pad(diamond(4), 2)
    assert lab.sum() == 41
    want = same_as_host(lab, whole(lab, [1, 0]))
    assert want.counts().tolist() == [1, 2] and want.count[0] == 36 and want.perimeter[0] == 36 and want.area2[0] == 82


def test_comb_is_one_long_ring():
    lab = comb(40)
    want = same_as_host(lab, whole(lab, [1, 0]))
    assert want.counts()[0] == 1 and want.areas()[0] == lab.sum() and want.perimeter[0] == 1642 == ms.measure_host(lab, whole(lab))[0, ms.GEOMETRY_COLUMNS.index("edges")]
    same_as_host(lab.T.copy(), whole(lab, [1, 0]))                    # teeth to the right: one candidate per tooth
    same_as_host(lab[::-1].copy(), whole(lab, [1, 0]))                # teeth upwards: the start is the first tooth's tip


def test_checkerboard_of_one_id():
    """128 rings in one job, and every inner vertex is a pinch that two rings pass: right first keeps the pixels apart"""
    lab = ((np.add.outer(np.arange(16), np.arange(16)) % 2) == 0).astype(np.int32)
    want = same_as_host(lab, whole(lab, [1, 0]))
    assert want.counts().tolist() == [128, 128] and (want.count == 4).all() and (want.area2 == 2).all()
    holes = 1 - np.pad(lab, 1)                                         # the complement in a frame: the board's 128 pixels are ONE 8-connected hole
    want = same_as_host(holes, whole(holes))
    assert want.counts()[0] == 100 and want.is_hole().sum() == 1 and want.areas()[0] == 18 * 18 - 128
    hole = want.ring(int(np.flatnonzero(want.is_hole())[0]))
    assert len(hole) == 120 and len(np.unique(hole, axis=0)) < 120    # one ring through its pinch vertices twice


def test_spiral_and_nested_island():
    lab = spiral(21)
    want = same_as_host(lab, whole(lab, [1, 0]))
    assert want.counts().tolist() == [1, 1] and want.count.tolist() == [44, 40]
    want = same_as_host(NESTED, whole(NESTED, [1, 0, 5]))
    assert want.area2.tolist() == [50, 2, -18, 18, -2] and want.counts().tolist() == [3, 2, 0]
    big = np.kron(NESTED, np.ones((7, 9), np.int32))
    assert same_as_host(big, whole(big, [1, 0])).counts().tolist() == [3, 2]


# ---- jobs and ids ------------------------------------------------------------------------------------------------------------------------

def test_ids_are_compared_only():
    ids = [0, -1, I32.min, I32.max]
    rng = np.random.default_rng(4)
    lab = np.array(ids + [7], np.int32)[rng.integers(0, 5, (37, 45))]
    want = same_as_host(lab, whole(lab, ids + [8]))
    assert (want.counts()[:4] > 0).all() and want.counts()[4] == 0
    assert np.array_equal(want.areas()[:4], [(lab == v).sum() for v in ids])


def test_boxes_that_cut_reach_beyond_and_bad_jobs_between_good_ones():
    H, W = 33, 47
    lab = random_mask(H, W, 5, 0.75) * 5
    jobs = [[0, 5, 0, 0, H, W], [0, 5, 3, 4, 20, 30],                 # whole, a box that cuts its id
            [-1, 5, 0, 0, H, W], [1, 5, 0, 0, H, W], [I32.max, 5, 0, 0, H, W], [I32.min, 5, 0, 0, H, W],
            [0, 5, -50, -50, H + 50, W + 50], [0, 5, I32.min, I32.min, I32.max, I32.max], [0, 5, -3, 40, 9, 99],
            [0, 5, 20, 30, 10, 40], [0, 5, 10, 40, 20, 30], [0, 5, 5, 5, 5, 9], [0, 5, H, W, H + 9, W + 9],      # inverted, inverted, empty, outside
            [0, 77, 0, 0, H, W], [0, 5, H - 1, W - 1, H + 9, W + 9], [0, 0, 3, 4, 20, 30]]
    want = same_as_host(lab, jobs)
    c = want.counts()
    assert c[0] > 1 and c[1] > 0 and not c[2:6].any() and want.slice(6, 7) == want.slice(0, 1) == want.slice(7, 8) and not c[9:14].any()
    me = np.zeros((H, W), bool)
    me[3:20, 4:30] = lab[3:20, 4:30] == 5
    cut = want.slice(1, 2)
    assert cut.areas()[0] == me.sum() and (cut.verts.min(0) >= [3, 4]).all() and (cut.verts.max(0) <= [20, 30]).all()


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


def test_three_images_in_one_launch_and_every_job_source():
    H, W = 40, 67
    ns = [7, 0, 12]
    lab = np.stack([blob_map(H, W, 7, 1), np.zeros((H, W), np.int32), blob_map(H, W, 12, 2)])
    want = ct.contours_host(lab, ns)
    assert len(want) == 19 and want.counts()[:7].any() and want.counts()[7:].any() and want.is_hole().any()
    d = up(lab)
    assert ct.contours(d, ns) == want                                 # jobs given as n: boxes from label_stats
    stats = [ms.labelmetrics.label_stats_host(lab[i], ns[i]) for i in range(3)]
    assert ct.contours(d, ns, stats=stats) == want                    # boxes given
    jobs = np.concatenate([ms.jobs_from_stats(s, i) for i, s in enumerate(stats)])
    order = np.random.default_rng(3).permutation(len(jobs))           # host jobs, interleaved across the images
    got = same_as_host(lab, jobs[order], d)
    assert all(got.slice(k, k + 1) == want.slice(o, o + 1) for k, o in enumerate(order.tolist()))
    edges = ms.measure_host(lab, ns)[:, ms.GEOMETRY_COLUMNS.index("edges")]
    assert np.array_equal(want.perimeters(), edges) and np.array_equal(want.areas(), np.concatenate(stats)[:, 0])
    # the raw entries with device jobs: rows stay on the device
    cnt = ct.contour_counts(d, up(jobs.astype(np.int32)))
    c = cnt.cpu().numpy()
    R, V = int(c[:, 0].sum()), int(c[:, 1].sum())
    table = np.concatenate([jobs.astype(np.int64), np.cumsum(c[:, :2], 0) - c[:, :2]], 1)
    rings, verts = ct.contour_rows(d, up(table.astype(np.int32)), R, V)
    assert rings.is_cuda and verts.is_cuda and rings.dtype == torch.int64 and verts.dtype == torch.int32 and rings.shape == (R, 4) and verts.shape == (V, 2)
    r = rings.cpu().numpy()
    assert np.array_equal(r, np.stack([want.first, want.count, want.perimeter, want.area2], 1)) and np.array_equal(verts.cpu().numpy(), want.verts)
    assert ct.contours(d[2], ns[2]) == want.slice(7, 19) == ct.contours_host(lab[2], ns[2])


# ---- size rule ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h", [8190, 8191])
def test_size_rule_and_host_fallback(h):
    """8190 x 30 is the tallest box of width 30 the device traces; 8191 x 30 gets status 1 and the host tracer on its box copied back"""
    W = 30
    lab = (np.random.default_rng(h).integers(0, 4, (h // 6 + 1, W // 3)).repeat(6, 0).repeat(3, 1)[:h] > 0).astype(np.int32)
    assert ct.fits(h, W) == (h == 8190)
    jobs = [[0, 1, 0, 0, h, W], [0, 1, 1, 0, h, W], [0, 0, 0, 0, h, W], [0, 1, 5, 3, 60, 20]]
    want = same_as_host(lab, jobs)                                     # the status column equals not fits(h, w)
    assert want.counts().min() > 0 and want.areas()[0] == lab.sum()


# ---- tables ------------------------------------------------------------------------------------------------------------------------------

def rows_host(lab, table, R, V, fill):
    """kg_label_contours in NumPy, offsets and the store predicates included"""
    rings, verts = np.full((R, 4), fill, np.int64), np.full((V, 2), fill, np.int32)
    for row in np.asarray(table, np.int64).tolist():
        c = ct.contours_host(lab, [row[:6]])
        first = row[7]
        for k in range(len(c.count)):
            if 0 <= row[6] + k < R:
                rings[row[6] + k] = first, c.count[k], c.perimeter[k], c.area2[k]
            for i, v in enumerate(c.ring(k).tolist()):
                if 0 <= first + i < V:
                    verts[first + i] = v
            first += int(c.count[k])
    return rings, verts


def test_wrong_tables_between_guard_rows():
    """These tables check the clamps and the store predicates; the result is rows_host's, sentinel included, and the guard rows in front
    of and behind both outputs stay as they were."""
    H, W, nimg = 33, 47, 2
    lab = np.stack([blob_map(H, W, 9, 5), blob_map(H, W, 9, 6)])
    d = up(lab)
    c5 = ct.contours_host(lab, [[0, 5, 0, 0, H, W]])
    n5, v5 = len(c5.count), int(c5.count.sum())
    assert v5 >= 8
    R, V = 40, 400
    # no two jobs name the same slot
    table = np.array([[0, 5, -50, -50, H + 50, W + 50, 1, 10],                                 # an oversized box is clamped
                      [-1, 5, 0, 0, H, W, 0, 0], [nimg, 5, 0, 0, H, W, 0, 0], [I32.max, 5, 0, 0, H, W, 1, 1], [I32.min, 5, 0, 0, H, W, 2, 2],
                      [0, 5, 20, 30, 10, 40, 0, 0], [0, 5, 5, 5, 5, 9, 0, 0],                  # inverted, empty
                      [1, 3, 0, 0, H, W, -1, -3],                                              # negative: the first ring row and three vertices are dropped
                      [1, 4, 0, 0, H, W, I32.min, I32.min],
                      [0, 5, 0, 0, H, W, R - 1, V - 5],                                        # at the end: one ring row and five vertices are stored
                      [0, 5, 0, 0, H, W, R, I32.max], [0, 5, 0, 0, H, W, I32.max, V],          # beyond R and V
                      [1, 6, H - 1, W - 1, H + 9, W + 9, 20, 200], [1, 6, H, W, H + 9, W + 9, 0, 0],
                      [0, 77, 0, 0, H, W, 0, 0]], np.int64)
    want_r, want_v = rows_host(lab, table, R, V, -7)
    assert (want_r == -7).any() and (want_r[R - 1] != -7).all() and (want_v[V - 5:] != -7).any() and (want_v[:1] != -7).any() and (want_r[1] != -7).all()
    from kg_instance_segmentation_amd._lib import ptr, stream_ptr
    gr = torch.full((R + 2, 4), -7, dtype=torch.int64, device=DEV)                              # rows in front of and behind the outputs
    gv = torch.full((V + 2, 2), -7, dtype=torch.int32, device=DEV)
    dj = up(table.astype(np.int32))
    _lib.call("kg_label_contours", ptr(d), nimg, H, W, ptr(dj), len(table), ptr(gr[1:]), R, ptr(gv[1:]), V, stream_ptr())
    r, v = gr.cpu().numpy(), gv.cpu().numpy()
    assert (r[0] == -7).all() and (r[-1] == -7).all() and (v[0] == -7).all() and (v[-1] == -7).all()
    assert np.array_equal(r[1:-1], want_r) and np.array_equal(v[1:-1], want_v)
    cnt = torch.full((len(table) + 2, 4), -7, dtype=torch.int64, device=DEV)
    _lib.call("kg_label_contour_counts", ptr(d), nimg, H, W, ptr(up(table[:, :6].astype(np.int32))), len(table), ptr(cnt[1:]), stream_ptr())
    c = cnt.cpu().numpy()
    assert (c[0] == -7).all() and (c[-1] == -7).all() and c[1].tolist() == [n5, v5, int(c5.perimeter.sum()), 0]
    assert not c[2:8].any() and not c[-3:-1].any() and (c[1:-1, 3] == 0).all()
    # m == 0 and R == V == 0 launch nothing
    assert ct.contour_counts(d, np.zeros((0, 6), np.int64)).shape == (0, 4)
    r0, v0 = ct.contour_rows(d, np.zeros((0, 8), np.int64), 0, 0)
    assert r0.shape == (0, 4) and v0.shape == (0, 2) and len(ct.contours(d, jobs=np.zeros((0, 6), np.int64))) == 0
    r0, v0 = ct.contour_rows(d, table, 0, 0)
    assert r0.shape == (0, 4) and v0.shape == (0, 2)
    with pytest.raises(E):
        ct.contours(d.to(torch.int64), [3, 3])
    with pytest.raises(E):
        ct.contour_rows(d, table, -1, 0)
    with pytest.raises(E):
        ct.contour_rows(d, table, R, V, rings=gv)
    with pytest.raises(E):
        _lib.call("kg_label_contours", ptr(d), nimg, H, W, ptr(dj), 1, ptr(d), 4, ptr(gv), V, stream_ptr())      # rings aliases labels
    with pytest.raises(E):
        _lib.call("kg_label_contour_counts", ptr(d), 0, H, W, ptr(dj), 1, ptr(cnt), stream_ptr())


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


def contours_match_host(inst):
    n = len(inst)
    lab = inst.labels.cpu().numpy()
    t = np.asarray(inst.table)
    assert isinstance(inst.contours, ct.Contours) and len(inst.contours) == n
    jobs = np.concatenate([np.zeros((n, 1), np.int64), np.arange(1, n + 1)[:, None], np.where(t[:, 1:2] > 0, t[:, 2:6], 0)], 1)
    assert inst.contours == ct.contours_host(lab, jobs)
    assert np.array_equal(inst.contours.areas(), t[:, 1])            # the table's visible area
    assert np.array_equal(inst.contours.perimeters(), ms.measure_host(lab, jobs)[:, ms.GEOMETRY_COLUMNS.index("edges")])


def test_predict_tiled_with_contours(cal_model):
    H, W, S = 400, 600, 256
    img = np.random.default_rng(8).integers(0, 256, (H, W, 3), dtype=np.uint8)
    plain = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4)
    got = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4, contours=True)
    n = len(plain)
    print("instances", n, "rings", len(got.contours.count), "vertices", len(got.contours.verts))
    assert n > 0 and plain.contours is None and plain.runs is None and same_instances(got, plain)        # the default path is untouched
    assert tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4, contours=None).contours is None
    contours_match_host(got)
    host = tiling.TiledInstances(got.labels.cpu().numpy(), got.dets, got.table, got.tile, got.origin, None)      # a host map goes through contours_host
    assert ct.contours_instances(host) == got.contours
    policy = dict(min_area=4)
    final = dt.expand_instances(cc.clean_instances(plain, **policy), 3)
    both = tiling.predict_tiled(cal_model, up(img), tile=S, overlap=64, batch=4, clean=policy, expand=3, contours={}, runs=True)
    assert same_instances(both, final) and both.neighbours is None and both.runs is not None
    contours_match_host(both)                                         # taken last, on the cleaned and expanded map
    assert np.array_equal(both.contours.areas(), both.runs.areas())


def test_predict_instances_with_contours(cal_model):
    S = 256
    src = np.random.default_rng(9).integers(0, 256, (2, S, S, 3), dtype=np.uint8)
    x = torch.cat([tiling.cut_tiles(src[i], tiling.plan(S, S, S, 64)) for i in range(2)])
    plain = inference.predict_instances(cal_model, x)
    assert all(p is not None and len(p) > 0 and p.contours is None for p in plain)
    assert all(p.contours is None for p in inference.predict_instances(cal_model, x, contours=None, measure=True))
    got = inference.predict_instances(cal_model, x, contours=True)
    full = inference.predict_instances(cal_model, x, clean=dict(min_area=4), expand=2, contours=True)
    assert len(got) == len(full) == 2
    for p, g, f in zip(plain, got, full):
        assert same_instances(p, g) and len(f) == len(p)
        contours_match_host(g)
        contours_match_host(f)
