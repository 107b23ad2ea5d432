"""GPU: the touching-neighbour graph (csrc/neighbours.hip, neighbours.py) against the host statements of the same semantics
(neighbours.neighbours_host, neighbours_rows_host).  Every comparison is exact integer equality.  Shapes are the smallest at which the
kernel can go wrong: one-pixel and one-row maps, box widths on both sides of the 256-thread walk, a box of more than one trip per thread,
rows of 1 to 64 slots, a hub with more neighbours than a row holds, INT_MIN and INT_MAX as values, jobs that reach beyond the map or name
no image, more than one image in a launch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from kg_instance_segmentation_amd import KGnet, _lib, inference, tiling  # noqa: E402
from kg_instance_segmentation_amd import components as cc  # noqa: E402
from kg_instance_segmentation_amd import distance as dt  # noqa: E402
from kg_instance_segmentation_amd import measure as ms  # noqa: E402
from kg_instance_segmentation_amd import neighbours as nb  # noqa: E402

DEV = "cuda"
I32 = np.iinfo(np.int32)


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


def row_jobs(jobs, resume=0, after=0):
    j = np.asarray(jobs, np.int64).reshape(-1, 6)
    return np.concatenate([j, np.full((len(j), 1), resume), np.full((len(j), 1), after)], 1)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 130), (130, 1)])
def test_smallest_maps(H, W, connectivity):
    n = 6
    lab = np.ones((1, 1), np.int32) if H * W == 1 else blob_map(H, W, n, 10 + H)
    want = nb.neighbours_host(lab, n, connectivity)
    got = nb.neighbours(up(lab), n, connectivity=connectivity)
    assert isinstance(got, nb.Neighbours) and got.values.dtype == np.int64 and got == want
    assert not want.corners.any() and (H * W == 1) == (len(want.values) == 0)               # a one-pixel-wide map has no diagonal inside it
    rows = nb.neighbours_rows(up(lab), row_jobs([[0, 1, 0, 0, H, W]]), 3, connectivity)
    assert np.array_equal(rows.cpu().numpy(), nb.neighbours_rows_host(lab, row_jobs([[0, 1, 0, 0, H, W]]), 3, connectivity))


@pytest.fixture(scope="module")
def blobs():
    H, W, n = 70, 131, 40
    lab = blob_map(H, W, n, 170)
    return lab, up(lab), n, {c: nb.neighbours_host(lab, n, c) for c in (4, 8)}


@pytest.mark.parametrize("connectivity", [4, 8])
def test_blobs_every_slot_count_and_job_source(blobs, connectivity):
    lab, d, n, graphs = blobs
    want = graphs[connectivity]
    assert want.degree().max() >= 9 and (want.degree() == 0).any() and (connectivity == 4 or want.corners.any())
    for slots in (1, 2, 16, 64):
        assert nb.neighbours(d, n, connectivity=connectivity, slots=slots) == want           # boxes from label_stats
    stats = ms.labelmetrics.label_stats_host(lab, n)
    assert nb.neighbours(d, n, stats=stats, connectivity=connectivity) == want                # boxes given
    jobs = ms.jobs_from_stats(stats)
    assert nb.neighbours(d, jobs=jobs, connectivity=connectivity, slots=2) == want            # host jobs
    assert np.array_equal(want.contact_length(), ms.measure(d, n, stats=stats).raw[:, 8])     # measure's device edges_contact
    for slots, resume, after in ((3, 0, 0), (64, 0, 0), (2, 1, 12), (5, 1, -3)):
        table = row_jobs(jobs, resume, after)
        ref = nb.neighbours_rows_host(lab, table, slots, connectivity)
        rows = nb.neighbours_rows(d, up(table.astype(np.int32)), slots, connectivity)        # the raw entry: device jobs, rows stay on the device
        assert rows.is_cuda and rows.dtype == torch.int64 and rows.shape == (n, 2 + 3 * slots)
        assert np.array_equal(rows.cpu().numpy(), ref)                                       # `more` and the zero padding included
        assert np.array_equal(nb.neighbours_rows(d, table, slots, connectivity).cpu().numpy(), ref)      # host jobs
        assert ref[:, 1].any() == (slots < 64) and (ref[:, 0] < slots).any()


@pytest.mark.parametrize("connectivity", [4, 8])
def test_box_widths_around_the_walk(connectivity):
    H, W = 300, 300
    lab = np.ones((H, W), np.int32)
    lab[:, 1::2] = 2                                                  # two-value stripes: every pixel touches the other value
    jobs = np.array([[0, 1, 3, 6, 40, 6 + w] for w in (1, 2, 255, 256, 257)] + [[0, 2, 3, 7, 40, 7 + w] for w in (1, 2, 255, 256, 257)]
                    + [[0, 1, 0, 0, H, W], [0, 2, 0, 0, H, W], [0, 1, 299, 0, 300, 300], [0, 2, 0, 299, 300, 300]])
    want = nb.neighbours_host(lab, jobs, connectivity)
    assert want.degree().tolist() == [1] * len(jobs)
    assert want.sides[:5].tolist() == [74, 74, 37 * 256, 37 * 256, 37 * 258] and want.sides[10] == 300 * 299
    assert want.sides[13] == 300 and want.corners[13] == (598 if connectivity == 8 else 0)  # a box edge inside the map is no object edge
    d = up(lab)
    assert nb.neighbours(d, jobs=jobs, connectivity=connectivity, max_job_pixels=2 ** 30) == want        # nothing split: the kernel's own walk
    assert nb.neighbours(d, jobs=jobs, connectivity=connectivity) == want                   # and in bands
    assert nb.neighbours(d, jobs=jobs, connectivity=connectivity, max_job_pixels=1000, slots=1) == want


def hub_map():
    """A 12 x 40 rectangle of id 7 ringed by 100 single pixels of distinct values, INT_MIN and INT_MAX among them"""
    lab = np.zeros((20, 50), np.int32)
    lab[4:16, 5:45] = 7
    ring = [(3, x) for x in range(5, 45)] + [(16, x) for x in range(5, 45)] + [(y, 4) for y in range(4, 16)] + [(y, 45) for y in range(4, 16)]
    vals = (np.arange(100) * 37 % 100 + 1000).astype(np.int64)        # distinct, not in order of position
    vals[13], vals[71] = I32.min, I32.max
    for (y, x), v in zip(ring[:100], vals.tolist()):
        lab[y, x] = v
    return lab, vals


@pytest.mark.parametrize("connectivity", [4, 8])
def test_hub_pages_even_at_64_slots(connectivity):
    lab, vals = hub_map()
    jobs = np.array([[0, 7, 4, 5, 16, 45], [0, 7, 0, 0, 20, 50], [0, int(vals[0]), 0, 0, 20, 50]])
    want = nb.neighbours_host(lab, jobs, connectivity)
    assert want.degree().tolist() == [100, 100, connectivity // 4 + 1] and want.values[0] == I32.min and want.values[99] == I32.max
    assert want.of(2)[0][0] == 7                                      # the ring pixels touch the hub and each other
    assert want.values[:100].tolist() == sorted(vals.tolist()) and (want.sides[:100] == 1).all()
    assert (want.corners[:100] > 0).any() == (connectivity == 8)
    d = up(lab)
    for slots in (64, 16, 7):
        assert nb.neighbours(d, jobs=jobs, connectivity=connectivity, slots=slots) == want
    assert nb.neighbours(d, jobs=jobs, connectivity=connectivity, slots=64, max_job_pixels=100) == want      # paged bands, merged by value
    first = nb.neighbours_rows(d, row_jobs(jobs), 64, connectivity).cpu().numpy()
    assert first[:, :2].tolist() == [[64, 1], [64, 1], [connectivity // 4 + 1, 0]] and first[0, 2] == I32.min
    rest = nb.neighbours_rows(d, row_jobs(jobs, 1, int(first[0, 2 + 3 * 63])), 64, connectivity).cpu().numpy()
    assert rest[0, :2].tolist() == [36, 0] and rest[0, 2 + 3 * 35] == I32.max and not rest[0, 2 + 3 * 36:].any()
    assert np.array_equal(rest, nb.neighbours_rows_host(lab, row_jobs(jobs, 1, int(first[0, 2 + 3 * 63])), 64, connectivity))
    for after, left in ((I32.min, 99), (I32.max, 0), (I32.max - 1, 1)):
        r = nb.neighbours_rows(d, row_jobs(jobs[:1], 1, after), 64, connectivity).cpu().numpy()
        assert r[0, 0] == min(left, 64) and r[0, 1] == (left > 64)
        assert np.array_equal(r, nb.neighbours_rows_host(lab, row_jobs(jobs[:1], 1, after), 64, connectivity))
    same = nb.neighbours_rows(d, row_jobs(jobs, 0, I32.max), 64, connectivity).cpu().numpy()
    assert np.array_equal(same, first)                                # resume == 0 ignores after


def test_hostile_job_table():
    H, W, nimg, slots = 33, 47, 2, 5
    lab = np.stack([blob_map(H, W, 9, 5), blob_map(H, W, 9, 6)])
    jobs = [[0, 5, -50, -50, H + 50, W + 50], [1, 3, -1, -1, H + 1, W + 1], [0, 4, I32.min, I32.min, I32.max, I32.max],
            [0, 5, 20, 30, 10, 40], [0, 5, 10, 40, 20, 30], [0, 5, 5, 5, 5, 9],        # inverted, inverted, empty
            [0, 77, 0, 0, H, W], [0, 0, 0, 0, H, W],                                    # an absent id; the background is a value like any other
            [nimg, 5, 0, 0, H, W], [-1, 5, 0, 0, H, W], [I32.max, 5, 0, 0, H, W], [I32.min, 5, 0, 0, H, W],
            [1, 4, H - 1, W - 1, H + 9, W + 9], [1, 4, H, W, H + 9, W + 9], [1, 4, I32.max - 1, I32.max - 1, I32.max, I32.max],
            [0, 5, I32.min, I32.min, I32.min + 1, I32.min + 1]]
    table = row_jobs(np.array(jobs + [[1, 5, 2, 3, 30, 44]] * 3000, np.int64))
    table[9, 6:], table[3, 6:], table[1, 6:] = (1, -5), (1, I32.min), (I32.min, -2)     # resume on bad jobs; any non-zero resume is a resume
    for connectivity in (4, 8):
        want = nb.neighbours_rows_host(lab, table, slots, connectivity)
        assert want[0, 0] > 0 and want[1, 0] > 0 and want[2, 0] > 0 and want[7, 0] == slots and want[7, 1] == 1 and want[16, 0] > 0
        assert not want[3:7].any() and not want[8:12].any() and not want[13:16].any()
        guard = torch.full((len(table) + 2, 2 + 3 * slots), -7, dtype=torch.int64, device=DEV)           # rows in front of and behind the output
        d, dj = up(lab), up(table.astype(np.int32))
        from kg_instance_segmentation_amd._lib import ptr, stream_ptr
        _lib.call("kg_label_neighbours", ptr(d), nimg, H, W, connectivity, ptr(dj), len(table), slots, ptr(guard[1:]), stream_ptr())
        g = guard.cpu().numpy()
        assert np.array_equal(g[1:-1], want) and (g[0] == -7).all() and (g[-1] == -7).all()
        assert (g[17:-1] == g[17]).all()                              # every copy of the repeated job is identical
    assert nb.neighbours_rows(d, np.zeros((0, 8), np.int64), slots).shape == (0, 2 + 3 * slots)          # m == 0 launches nothing
    E = _lib.KGLibraryError
    for bad in (dict(slots=0), dict(slots=65), dict(connectivity=6)):
        with pytest.raises(E):
            nb.neighbours(d, jobs=np.zeros((1, 6), np.int64), **bad)
    with pytest.raises(E):
        _lib.call("kg_label_neighbours", ptr(d), nimg, H, W, 4, ptr(dj), 1, 65, ptr(guard), stream_ptr())
    with pytest.raises(E):
        _lib.call("kg_label_neighbours", ptr(d), nimg, H, W, 5, ptr(dj), 1, 4, ptr(guard), stream_ptr())
    with pytest.raises(E):
        nb.neighbours(d.to(torch.int64), 3)


def test_three_images_in_one_launch():
    H, W = 40, 67
    ns = [7, 0, 12]
    lab = np.stack([blob_map(H, W, 7, 1), np.zeros((H, W), np.int32), blob_map(H, W, 12, 2)])
    want = nb.neighbours_host(lab, ns, 8)
    assert len(want) == 19 and want.degree()[:7].any() and want.degree()[7:].any()
    d = up(lab)
    assert nb.neighbours(d, ns, connectivity=8, slots=2) == want
    stats = [ms.labelmetrics.label_stats_host(lab[i], ns[i]) for i in range(3)]
    jobs = np.concatenate([ms.jobs_from_stats(s, i) for i, s in enumerate(stats)])
    order = np.random.default_rng(3).permutation(len(jobs))          # jobs interleaved across the images
    got = nb.neighbours(d, jobs=jobs[order], connectivity=8, slots=3)
    assert got == nb.neighbours_host(lab, jobs[order], 8)
    assert all(np.array_equal(a, b) for k, o in enumerate(order) for a, b in zip(got.of(k), want.of(o)))


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


def test_predict_tiled_with_neighbours(cal_model):
    H, W, S = 400, 600, 256
    img = np.random.default_rng(8).integers(0, 256, (H, W, 3), dtype=np.uint8)
    plain = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4)
    got = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4, neighbours=True)
    n = len(plain)
    print("instances", n)
    assert n > 0 and plain.neighbours is None and plain.measurements is None and same_instances(got, plain)    # the default path is untouched
    assert isinstance(got.neighbours, nb.Neighbours) and len(got.neighbours) == n and got.measurements is None
    lab = got.labels.cpu().numpy()
    assert got.neighbours == nb.neighbours_host(lab, n)
    print("pairs", len(got.neighbours.pairs()), "max degree", int(got.neighbours.degree().max()))
    # the graph after expansion, the instances themselves unchanged
    before = got.labels.clone()
    grown = nb.neighbours_instances(got, connectivity=8, expand=4, slots=3)
    assert torch.equal(got.labels, before) and len(grown) == n
    assert grown == nb.neighbours_host(dt.expand_labels_host(lab, 4), n, 8)
    assert len(grown.values) >= len(got.neighbours.values)
    host = tiling.TiledInstances(lab, got.dets, got.table, got.tile, got.origin, None)      # a host map goes through neighbours_host
    assert nb.neighbours_instances(host, connectivity=8, expand=4) == grown
    # with clean= and expand= as well: taken after both, on the final map
    policy = dict(min_area=4)
    final = dt.expand_instances(cc.clean_instances(plain, **policy), 3)
    both = tiling.predict_tiled(cal_model, up(img), tile=S, overlap=64, batch=4, clean=policy, expand=3, measure=True,
                                neighbours=dict(connectivity=8, slots=2))
    assert same_instances(both, final) and both.measurements is not None
    assert both.neighbours == nb.neighbours_host(both.labels.cpu().numpy(), n, 8)
    assert np.array_equal(both.neighbours.contact_length(), both.measurements.raw[:, 8])


def test_predict_instances_with_neighbours(cal_model):
    S = 256
    src = np.random.default_rng(9).integers(0, 256, (2, S, S, 3), dtype=np.uint8)
    x = torch.cat([tiling.cut_tiles(src[i], tiling.plan(S, S, S, 64)) for i in range(2)])
    plain = inference.predict_instances(cal_model, x)
    assert all(p is not None and len(p) > 0 and p.neighbours is None for p in plain)
    assert all(p.neighbours is None for p in inference.predict_instances(cal_model, x, neighbours=None, measure=True))
    got = inference.predict_instances(cal_model, x, neighbours=True)
    policy = dict(min_area=4)
    full = inference.predict_instances(cal_model, x, clean=policy, expand=2, neighbours=dict(connectivity=8, expand=4))
    assert len(got) == len(full) == 2
    for p, g, f in zip(plain, got, full):
        assert same_instances(p, g) and g.neighbours == nb.neighbours_host(p.labels.cpu().numpy(), len(p))
        lab = f.labels.cpu().numpy()                                  # cleaned and expanded by 2; the graph is taken 4 further out
        assert f.neighbours == nb.neighbours_host(dt.expand_labels_host(lab, 4), len(f), 8) and len(f.neighbours) == len(p)
