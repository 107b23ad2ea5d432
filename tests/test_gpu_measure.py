"""GPU: per-instance measurements (csrc/measure.hip, measure.py) against the host statement of the same semantics (measure.measure_host).
Every comparison is exact integer equality.  Shapes are the smallest at which the kernel can go wrong: one-pixel and one-row maps, an odd
width under 3- and 6-byte pixels, box widths on both sides of the 256-thread walk, jobs that reach beyond the map or name no image,
16-bit sums of squares past 2^32, bands, more than one image in a launch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from kg_instance_segmentation_amd import KGnet, _lib, inference, instances, tiling  # noqa: E402
from kg_instance_segmentation_amd import components as cc  # noqa: E402
from kg_instance_segmentation_amd import measure as ms  # noqa: E402
from kg_instance_segmentation_amd.bitmasks import BitMasks  # noqa: E402

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


def seeded_image(shape, C, dtype, seed):
    top = np.iinfo(dtype).max
    img = np.random.default_rng(seed).integers(0, top + 1, tuple(shape) + (C,)).astype(dtype)
    img.reshape(-1)[::7] = 0
    img.reshape(-1)[3::11] = top
    return img


@pytest.mark.parametrize("H,W", [(1, 1), (1, 130), (130, 1)])
def test_smallest_maps(H, W):
    n = 6
    lab = np.ones((1, 1), np.int32) if H * W == 1 else blob_map(H, W, n, 10 + H)
    img = seeded_image((H, W), 3, np.uint8, 1)
    want = ms.measure_host(lab, n, img)
    got = ms.measure(up(lab), n, image=img)
    assert isinstance(got, ms.Measurements) and got.raw.dtype == np.int64 and np.array_equal(got.raw, want)
    assert want[:, 0].sum() == np.count_nonzero(lab) and want[:, 7].any()
    if H * W == 1:
        assert want[0].tolist()[:10] == [1, 0, 0, 0, 0, 0, 4, 4, 0, 1]


@pytest.mark.parametrize("C,dtype", [(0, None), (1, np.uint8), (3, np.uint8), (4, np.uint8), (1, np.uint16), (3, np.uint16)])
def test_blobs_every_channel_layout(C, dtype):
    H, W, n = 70, 131, 40                                            # odd W: 3- and 6-byte pixels at every alignment
    lab = blob_map(H, W, n, 170)
    img = seeded_image((H, W), C, dtype, 7) if C else None
    want = ms.measure_host(lab, n, img)
    assert (want[:, 0] > 0).sum() >= 20 and (want[:, 0] == 0).any() and want[:, 7].any() and want[:, 8].any()
    if C:
        top = np.iinfo(dtype).max
        assert (want[:, 12::4] == 0).any() and (want[:, 13::4] == top).any()                # values include 0 and the top of the type
    d = up(lab)
    got = ms.measure(d, n, image=img)                                # boxes from label_stats, the image uploaded here
    assert np.array_equal(got.raw, want) and got.channels == C
    stats = ms.labelmetrics.label_stats_host(lab, n)
    dimg = None if img is None else up(img.view(np.int16) if dtype == np.uint16 else img)
    assert np.array_equal(ms.measure(d, n, image=dimg, stats=stats).raw, want)              # boxes given, a device image
    jobs = ms.jobs_from_stats(stats)
    rows = ms.measure_rows(d, up(jobs), dimg)                        # the raw entry: device jobs, rows stay on the device
    assert rows.is_cuda and rows.dtype == torch.int64 and np.array_equal(rows.cpu().numpy(), want)
    p, q = got.props(), ms.Measurements(want).props()
    assert all(np.array_equal(p[k], q[k], equal_nan=True) for k in q)


def test_box_widths_around_the_walk():
    H, W = 300, 300
    lab = np.ones((H, W), np.int32)
    img = seeded_image((H, W), 1, np.uint8, 2)
    jobs = np.array([[0, 1, 3, 7, 40, 7 + w] for w in (1, 2, 255, 256, 257)] + [[0, 1, 0, 0, H, W], [0, 1, 299, 0, 300, 300], [0, 1, 0, 299, 300, 300]])
    want = ms.measure_host(lab, jobs, img)
    assert want[:, 0].tolist() == [37, 74, 37 * 255, 37 * 256, 37 * 257, 90000, 300, 300]
    assert want[5, 6:10].tolist() == [1200, 1200, 0, 1196] and not want[:5, 6].any()     # a box edge inside the map is no object edge
    got = ms.measure(up(lab), jobs=jobs, image=img, max_job_pixels=2 ** 30)                  # nothing split: the kernel's own walk
    assert np.array_equal(got.raw, want)
    assert np.array_equal(ms.measure(up(lab), jobs=jobs, image=img).raw, want)               # and in bands


def test_hostile_job_table():
    H, W, nimg = 33, 47, 2
    lab = np.stack([blob_map(H, W, 9, 5), blob_map(H, W, 9, 6)])
    img = seeded_image((nimg, H, W), 2, np.uint16, 3)
    jobs = [[0, 3, -50, -50, H + 50, W + 50], [1, 3, -1, -1, H + 1, W + 1], [0, 2, I32.min, I32.min, I32.max, I32.max],
            [0, 3, 20, 30, 10, 40], [0, 3, 10, 40, 20, 30], [0, 3, 5, 5, 5, 9],        # inverted, inverted, empty
            [0, 77, 0, 0, H, W], [0, 0, 0, 0, H, W],                                    # an absent id; the background is a value like any other
            [nimg, 3, 0, 0, H, W], [-1, 3, 0, 0, H, W], [I32.max, 3, 0, 0, H, W], [I32.min, 3, 0, 0, H, W],
            [1, 4, H - 1, W - 1, H + 9, W + 9], [1, 4, H, W, H + 9, W + 9]]
    jobs = np.array(jobs + [[1, 5, 2, 3, 30, 44]] * 3000, np.int64)
    want = ms.measure_host(lab, jobs, img)
    assert want[0, 0] > 0 and want[1, 0] > 0 and want[2, 0] > 0 and want[7, 0] == np.count_nonzero(lab[0] == 0) and want[14, 0] > 0
    assert not want[3:7].any() and not want[8:12].any() and not want[13].any()
    guard = torch.full((len(jobs) + 2, 18), -7, dtype=torch.int64, device=DEV)           # rows in front of and behind the output
    d, dj, di = up(lab), up(jobs.astype(np.int32)), up(img.view(np.int16))
    from kg_instance_segmentation_amd._lib import ptr, stream_ptr
    _lib.call("kg_label_measure", ptr(d), nimg, H, W, ptr(di), 2, 2, ptr(dj), len(jobs), ptr(guard[1:]), stream_ptr())
    g = guard.cpu().numpy()
    assert np.array_equal(g[1:-1], want) and (g[0] == -7).all() and (g[-1] == -7).all()
    assert (g[15:-1] == g[15]).all()                                  # every copy of the repeated job is identical
    assert np.array_equal(ms.measure_rows(d, jobs, img).cpu().numpy(), want)
    assert ms.measure_rows(d, np.zeros((0, 6), np.int64), img).shape == (0, 18)          # m == 0 launches nothing


def test_grid_stride():
    """More jobs than the grid cap of 2^20 blocks (C = 0): the blocks stride, and every copy of one small job gives the single job's row."""
    H, W, m = 9, 70, 2 ** 20 + 3
    lab = np.zeros((H, W), np.int32)
    lab[3:5, 10:13] = 4
    lab[4, 13] = 2
    job = np.array([[0, 4, 3, 10, 5, 14]], np.int32)                 # 8 pixels, 6 of them the id's
    want = ms.measure_host(lab, job)
    assert want[0, :3].tolist() == [6, 21, 66] and want[0, 8] > 0
    d = up(lab)
    one = ms.measure_rows(d, job)
    assert np.array_equal(one.cpu().numpy(), want)
    guard = torch.full((m + 2, 10), -7, dtype=torch.int64, device=DEV)                      # rows in front of and behind the output
    from kg_instance_segmentation_amd._lib import ptr, stream_ptr
    jd = up(job).repeat(m, 1)
    _lib.call("kg_label_measure", ptr(d), 1, H, W, None, 0, 1, ptr(jd), m, ptr(guard[1:]), stream_ptr())
    assert bool((guard[1:-1] == one).all()) and bool((guard[0] == -7).all()) and bool((guard[-1] == -7).all())


def test_extreme_label_values_are_contact():
    lab = np.zeros((9, 70), np.int32)
    lab[3:6, 10:60] = 5
    lab[2, 12], lab[6, 20], lab[4, 9], lab[4, 60] = I32.min, -1, I32.max, 6
    lab[0, 0], lab[8, 69] = I32.min, I32.max
    jobs = np.array([[0, 5, 0, 0, 9, 70], [0, I32.min, 0, 0, 9, 70], [0, I32.max, 0, 0, 9, 70], [0, -1, 0, 0, 9, 70]])
    want = ms.measure_host(lab, jobs)
    assert want[0, 6:9].tolist() == [106, 0, 4] and want[1, 0] == 2 and want[2, 0] == 2 and want[3].tolist()[:1] == [1]
    assert want[1, 7] == 2 and want[1, 8] == 1                        # INT_MIN in the corner: two frame edges; next to the object: contact
    assert np.array_equal(ms.measure(up(lab), jobs=jobs).raw, want)


@pytest.mark.parametrize("cap", [65536, 1000])
def test_sums_of_squares_past_32_bits_and_bands(cap):
    H = W = 512
    lab = np.ones((H, W), np.int32)
    img = np.full((H, W, 1), 65535, np.uint16)
    want = ms.measure_host(lab, 1, img)
    assert want[0, 11] == 512 * 512 * 65535 ** 2 > 2 ** 49 and want[0, 10] > 2 ** 33 and want[0, 3] > 2 ** 34
    got = ms.measure(up(lab), 1, image=img, max_job_pixels=cap)      # 4 bands of whole rows / 512 row pieces
    assert np.array_equal(got.raw, want)
    assert want[0, 6:10].tolist() == [2048, 2048, 0, 2044]           # no band edge became an object edge
    if cap == 65536:
        one = ms.measure_rows(up(lab), np.array([[0, 1, 0, 0, H, W]]), img)               # and unsplit: 1024 trips of the walk
        assert np.array_equal(one.cpu().numpy(), want)


def test_three_images_in_one_launch():
    H, W = 40, 67
    ns = [7, 0, 12]
    lab = np.stack([blob_map(H, W, 7, 1), np.zeros((H, W), np.int32), blob_map(H, W, 12, 2)])
    img = seeded_image((3, H, W), 3, np.uint8, 4)
    want = ms.measure_host(lab, ns, img)
    assert want.shape == (19, 22) and want[:7, 0].any() and want[7:, 0].any()
    got = ms.measure(up(lab), ns, image=up(img))
    assert np.array_equal(got.raw, want)
    swapped = ms.measure_host(lab[::-1], ns[::-1], img[::-1])
    assert np.array_equal(swapped[12:], want[:7]) and not np.array_equal(want[:7], ms.measure_host(lab, ns, img[::-1])[:7])   # content per image


def test_measure_instances_on_overlapping_masks():
    rng = np.random.default_rng(11)
    n, H, W = 14, 60, 90
    yy, xx = np.mgrid[0:H, 0:W]
    dense = np.zeros((n, H, W), np.uint8)
    for k in range(n):
        cy, cx, ry, rx = rng.integers(0, H), rng.integers(0, W), rng.integers(3, 14), rng.integers(3, 14)
        dense[k] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
    dense[5] = dense[2] & (yy % 2 == 0)                              # fully hidden under an earlier row
    m = BitMasks.from_dense(dense)
    labels, table = instances.label_map(m, with_table=True)
    inst = instances.Instances(labels[0], np.zeros((n, 5), np.float32), table.cpu().numpy(), m)
    assert inst.measurements is None and inst.table[5, 1] == 0 and inst.table[5, 0] > 0
    img = seeded_image((H, W), 3, np.uint8, 12)
    got = ms.measure_instances(inst, img)
    want = ms.measure_host(instances.label_map_host(dense), n, img)
    assert len(got) == n and np.array_equal(got.raw, want) and not got.raw[5].any() and got.raw[:, 8].any()
    assert np.array_equal(got.raw[:, :3], inst.table[:, [1, 6, 7]])  # area and coordinate sums agree with the table
    host = instances.Instances(labels[0].cpu().numpy(), inst.dets, inst.table, None)         # a host map goes through measure_host
    assert np.array_equal(ms.measure_instances(host, img).raw, want)
    assert np.array_equal(got.props()["centroid"], inst.centroids(), equal_nan=True)


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


def test_predict_tiled_with_measure(cal_model):
    H, W, S = 400, 600, 256
    img = np.random.default_rng(8).integers(0, 256, (H, W, 3), dtype=np.uint8)
    plain = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4)
    got = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4, measure=True)
    n = len(plain)
    print("instances", n)
    assert n > 0 and plain.measurements is None and same_instances(got, plain)               # the default path is untouched
    assert np.array_equal(got.tile, plain.tile) and np.array_equal(got.origin, plain.origin)
    assert isinstance(got.measurements, ms.Measurements) and got.measurements.channels == 3
    assert np.array_equal(got.measurements.raw, ms.measure_host(got.labels.cpu().numpy(), n, img))
    assert np.array_equal(got.measurements.raw[:, :3], got.table[:, [1, 6, 7]])
    # with clean= as well: measured after the clean-up, on the cleaned map (a device image this time)
    policy = dict(min_area=4)
    cleaned = cc.clean_instances(plain, **policy)
    both = tiling.predict_tiled(cal_model, up(img), tile=S, overlap=64, batch=4, clean=policy, measure=True)
    assert cleaned.measurements is None and same_instances(both, cleaned)
    assert np.array_equal(both.measurements.raw, ms.measure_host(both.labels.cpu().numpy(), n, img))
    assert np.array_equal(both.measurements.raw[:, 0], both.table[:, 1])
    p = both.measurements.props()
    assert p["mean"].shape == (n, 3) and p["touches_border"].dtype == bool


def test_predict_instances_with_measure(cal_model):
    S = 256
    src = np.random.default_rng(9).integers(0, 256, (2, S, S, 3), dtype=np.uint8)
    x = torch.cat([tiling.cut_tiles(src[i], tiling.plan(S, S, S, 64)) for i in range(2)])
    plain = inference.predict_instances(cal_model, x)
    assert all(p is not None and len(p) > 0 and p.measurements is None for p in plain)
    geom = inference.predict_instances(cal_model, x, measure=True)
    inten = np.random.default_rng(10).integers(0, 65536, (2, S, S, 2)).astype(np.uint16)
    full = inference.predict_instances(cal_model, x, measure=inten)
    assert len(geom) == len(full) == 2
    for i, (p, g, f) in enumerate(zip(plain, geom, full)):
        assert same_instances(p, g) and same_instances(p, f)
        lab = p.labels.cpu().numpy()
        assert np.array_equal(g.measurements.raw, ms.measure_host(lab, len(p))) and g.measurements.channels == 0
        assert np.array_equal(f.measurements.raw, ms.measure_host(lab, len(p), inten[i])) and f.measurements.channels == 2
