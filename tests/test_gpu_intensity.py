"""GPU: per-instance intensity quantiles and histograms (csrc/intensity.hip, intensity.py) against the host statement of the same
semantics (intensity.quantiles_host / histograms_host).  Every comparison is exact integer equality.  Shapes are the smallest at which
the kernels can go wrong: one-pixel, one-row and one-column maps, objects of 1, 2, 255, 256 and 257 pixels, box widths on both sides of
the 256-thread walk, every channel count under both element sizes, values that put every lane on one bin or every rank in another high
byte, hostile job and quantile tables between guard rows, the large-job route, more jobs than the grid cap, several images in a launch."""
from fractions import Fraction as F

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from kg_instance_segmentation_amd import KGnet, _lib, inference, tiling  # noqa: E402
from kg_instance_segmentation_amd import components as cc  # noqa: E402
from kg_instance_segmentation_amd import distance  # noqa: E402
from kg_instance_segmentation_amd import intensity as iq  # noqa: E402
from kg_instance_segmentation_amd import measure as ms  # noqa: E402
from kg_instance_segmentation_amd._lib import ptr, stream_ptr  # noqa: E402

DEV = "cuda"
I32 = np.iinfo(np.int32)
Q8 = [F(0), F(1), F(1, 2), F(1, 2), F(1, 3), F(999, 1000), F(1, 20), F(3, 4)]      # Q = 8: 0, 1, a repeated one, 1/3, 999/1000


def up(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(DEV)


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


def all_channel_jobs(jobs, C, shift, prefix=-1):
    return iq._hist_jobs(np.repeat(np.asarray(jobs, np.int64), C, 0), np.tile(np.arange(C), len(jobs)), shift, prefix)


def check(lab, img, q, n=None, jobs=None, **kw):
    """device quantiles == quantiles_host; returns the raw rows"""
    want = iq.quantiles_host(lab, n if jobs is None else jobs, img, q)
    got = iq.quantiles(up(lab), n, jobs, image=img, q=q, **kw)
    assert isinstance(got, iq.Quantiles) and got.raw.dtype == np.int64 and got.q == iq.as_fractions(q)
    assert np.array_equal(got.raw, want)
    return want


@pytest.mark.parametrize("H,W", [(1, 1), (1, 130), (130, 1)])
def test_smallest_maps(H, W):
    n = 6
    lab = np.ones((1, 1), np.int32) if H * W == 1 else blob_map(H, W, n, 10 + H)
    for dtype in (np.uint8, np.uint16):
        img = seeded_image((H, W), 3, dtype, 1)
        want = check(lab, img, None, n)
        assert want[:, 0, 0].sum() == np.count_nonzero(lab)
        if H * W == 1:
            v = img[0, 0].astype(np.int64)
            assert np.array_equal(want[0], np.concatenate([[[1]] * 3, np.repeat(v[:, None], 10, 1)], 1)) and not want[1:].any()
        h = iq.histograms(up(lab), n, image=img)
        jobs = ms.jobs_from_stats(ms.labelmetrics.label_stats_host(lab, n))
        assert h.shift == (8 if dtype == np.uint16 else 0)
        assert np.array_equal(h.counts.reshape(-1, 256), iq.histograms_host(lab, all_channel_jobs(jobs, 3, h.shift), img))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_object_sizes_and_box_widths(dtype):
    H, W = 300, 300
    lab = np.zeros((H, W), np.int32)
    for i, k in enumerate((1, 2, 255, 256, 257)):                    # objects of exactly that many pixels, one row each
        lab[2 * i, 5:5 + k] = i + 1
    lab[20:, :] = 9
    img = seeded_image((H, W), 1, dtype, 2)
    jobs = [[0, i + 1, 0, 0, 20, W] for i in range(5)] + [[0, 9, 23, 7, 60, 7 + w] for w in (1, 2, 255, 256, 257)] \
        + [[0, 9, 299, 0, 300, 300], [0, 9, 20, 299, 300, 300]]
    want = check(lab, img, Q8, jobs=np.array(jobs), max_job_pixels=2 ** 30)
    assert want[:, 0, 0].tolist() == [1, 2, 255, 256, 257, 37, 74, 37 * 255, 37 * 256, 37 * 257, 300, 280]
    assert want[1, 0, 5] != want[1, 0, 6]                            # n = 2, q = 1/2: k_lo != k_hi


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_blobs_every_channel_layout(C, dtype):
    H, W, n = 70, 131, 40                                            # odd W: 3-byte pixels at every alignment
    lab = blob_map(H, W, n, 170)
    img = seeded_image((H, W), C, dtype, 7)
    want = check(lab, img, None, n)
    assert (want[:, 0, 0] > 0).sum() >= 20 and (want[:, 0, 0] == 0).any() and (want[:, :, 1::2] != want[:, :, 2::2]).any()
    d, dimg = up(lab), up(img)
    stats = ms.labelmetrics.label_stats_host(lab, n)
    assert np.array_equal(iq.quantiles(d, n, image=dimg, stats=stats, q=Q8).raw, iq.quantiles_host(lab, n, img, Q8))   # a device image
    jobs = ms.jobs_from_stats(stats)
    rows = iq.quantile_rows(d, up(jobs), dimg, up(iq.q_table(None)))  # the raw entry: everything on the device, rows stay there
    assert rows.is_cuda and rows.dtype == torch.int32 and rows.shape == (n, C, 11) and np.array_equal(rows.cpu().numpy(), want)
    assert np.array_equal(iq.quantile_rows(d, jobs, img, [F(1, 2)]).cpu().numpy(), iq.quantiles_host(lab, n, img, [F(1, 2)]))   # Q = 1
    h = iq.histograms(d, n, image=dimg, stats=stats)
    assert np.array_equal(h.counts.reshape(-1, 256), iq.histograms_host(lab, all_channel_jobs(jobs, C, h.shift), img))
    assert np.array_equal(h.totals(), want[:, :, 0])
    if dtype == np.uint8:                                            # an independent check: the rank rule read off the histogram
        for k, f in enumerate(iq.DEFAULT_Q):
            assert np.array_equal(h.quantile(f.numerator, f.denominator), want[:, :, 1 + 2 * k:3 + 2 * k])
    p, q = iq.quantiles(d, n, image=img).props(), iq.Quantiles(want).props()
    assert all(np.array_equal(p[k], q[k], equal_nan=True) for k in q)


def test_values_uint8():
    lab = np.zeros((40, 64), np.int32)
    lab[0:30, :] = 1                                                 # constant: every lane hits one bin
    lab[30:34, :] = 2                                                # all 256 values once
    lab[34:40, 3:60] = 3                                             # only 0 and 255
    img = np.full((40, 64, 2), 93, np.uint8)
    img[30:34, :, 0] = np.random.default_rng(3).permutation(256).reshape(4, 64)
    img[30:34, :, 1] = np.arange(256).reshape(4, 64)[::-1]
    img[34:40, :, 0] = np.where(np.random.default_rng(4).random((6, 64)) < 0.3, 255, 0)
    img[34:40, :, 1] = 255
    img[35, 10, 1] = 0
    want = check(lab, img, Q8, 3)
    assert (want[0, :, 1:] == 93).all() and want[1, 0, 1:3].tolist() == [0, 0] and want[1, 0, 3:5].tolist() == [255, 255]
    assert want[1, 1, 5:7].tolist() == [127, 128] and set(want[2, 0, 1:].tolist()) == {0, 255} and want[2, 1, 1:5].tolist() == [0, 0, 255, 255]
    check(lab, img, [F(1, 2)], 3)                                    # Q = 1


def test_values_uint16():
    lab = np.zeros((40, 64), np.int32)
    img = np.zeros((40, 64, 1), np.uint16)
    lab[0:6, 3:60] = 1                                               # only 0 and 65535
    img[0:6, :, 0] = np.where(np.random.default_rng(5).random((6, 64)) < 0.4, 65535, 0)
    lab[6, 0:2] = 2                                                  # {0x00ff, 0x0100}: lo and hi of 1/2 in different high bytes
    img[6, 0:2, 0] = [0x0100, 0x00ff]
    lab[7:12, :] = 3                                                 # every high byte equal
    img[7:12, :, 0] = 0x4200 | np.random.default_rng(6).integers(0, 256, (5, 64))
    lab[12:30, 1:63] = 4                                             # 12-bit data
    img[12:30, :, 0] = np.random.default_rng(7).integers(0, 4096, (18, 64))
    lab[30:35, :] = 5                                                # 257 pixels, sorted value k has high byte min(k, 255): with
    lab[34, 1:] = 0                                                  # q_i = (64 i + 17) / 512 the ranks are 32 i + 8 and 32 i + 9
    k = np.random.default_rng(8).permutation(257)
    ys, xs = np.nonzero(lab == 5)
    img[ys, xs, 0] = (np.minimum(k, 255) << 8) | (k * 37 & 255)
    want = check(lab, img, Q8, 5)
    assert set(want[0, 0, 1:].tolist()) == {0, 65535} and want[1, 0, 5:7].tolist() == [0x00ff, 0x0100]
    assert ((want[2, 0, 1:] >> 8) == 0x42).all() and (want[3, 0, 1:] < 4096).all() and want[3, 0, 4] > 255
    spread = [F(64 * i + 17, 512) for i in range(8)]
    far = check(lab, img, spread, 5)
    assert sorted((far[4, 0, 1:] >> 8).tolist()) == sorted([32 * i + 8 for i in range(8)] + [32 * i + 9 for i in range(8)])   # 16 distinct
    # the same with 3 channels that select different bytes per channel, and a two-channel image with one constant channel
    img3 = np.concatenate([img, img[::-1, ::-1], (img >> 3).astype(np.uint16)], 2)
    check(lab, img3, spread, 5)
    check(lab, img3[..., 1:], Q8, 5)


def test_histogram_jobs():
    H, W, n = 50, 77, 8
    lab = blob_map(H, W, n, 31)
    jobs = ms.jobs_from_stats(ms.labelmetrics.label_stats_host(lab, n))
    wide = seeded_image((H, W), 2, np.uint16, 32)
    wide[..., 1] >>= 4                                               # channel 1: 12-bit camera data
    narrow = seeded_image((H, W), 3, np.uint8, 33)
    for img, C in ((wide, 2), (narrow, 3)):
        j9 = np.concatenate([all_channel_jobs(jobs, C, s, p) for s, p in ((0, -1), (4, -1), (8, -1), (0, 0), (0, 7), (4, 3), (2, 1))]
                            + [all_channel_jobs(jobs[:2], 1, 0) + [0, 0, 0, 0, 0, 0, ch, 0, 0] for ch in (C, -1, I32.max)]          # no such channel
                            + [all_channel_jobs(jobs[:2], 1, 0) + [0, 0, 0, 0, 0, 0, 0, sh, 0] for sh in (9, -1, 40)])             # no such shift
        want = iq.histograms_host(lab, j9, img)
        got = iq.histogram_rows(up(lab), j9, img)
        assert got.is_cuda and got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
        assert want[:len(jobs) * C].any() and not want[-12:].any() and want[3 * len(jobs) * C:5 * len(jobs) * C].any()
    h4 = iq.histograms(up(lab), n, image=wide[..., 1:], shift=4)     # the exact histogram of 12-bit data
    assert np.array_equal(h4.counts[0, 0], np.bincount(wide[..., 1][lab == 1] >> 4, minlength=256)) and h4.counts[0, 0].sum() > 0
    assert iq.histogram_rows(up(lab), np.zeros((0, 9), np.int64), narrow).shape == (0, 256)         # m == 0 launches nothing


def test_ids_and_bad_jobs():
    H, W = 33, 70
    lab = blob_map(H, W, 9, 5)
    lab[3:6, 10:60] = -1
    lab[8:11, 5:50] = I32.min
    lab[20:25, 30:69] = I32.max
    img = seeded_image((H, W), 3, np.uint8, 3)
    good = [[0, v, 0, 0, H, W] for v in (0, -1, I32.min, I32.max, 3)]
    bad = [[1, 3, 0, 0, H, W], [-1, 3, 0, 0, H, W], [I32.max, 3, 0, 0, H, W], [I32.min, 3, 0, 0, H, W],          # no such image
           [0, 3, 20, 30, 10, 40], [0, 3, 10, 40, 20, 30], [0, 3, 5, 5, 5, 9], [0, 3, H, W, H + 9, W + 9],        # inverted, empty, outside
           [0, 77, 0, 0, H, W]]                                                                                   # an absent id
    jobs = np.array([row for pair in zip(good * 2, bad) for row in pair] + [[0, 2, -50, -50, H + 50, W + 50]], np.int64)
    want = check(lab, img, None, jobs=jobs)
    assert (want[0:-1:2, 0, 0] > 0).all() and not want[1:-1:2].any() and want[-1, 0, 0] > 0
    assert want[0, 0, 0] == np.count_nonzero(lab == 0) and want[4, 0, 0] == np.count_nonzero(lab == I32.min)
    wide = seeded_image((H, W), 2, np.uint16, 4)
    check(lab, wide, Q8, jobs=jobs)


def test_three_images_interleaved():
    H, W = 40, 67
    lab = np.stack([blob_map(H, W, 7, 1), np.zeros((H, W), np.int32), blob_map(H, W, 12, 2)])
    img = seeded_image((3, H, W), 3, np.uint16, 4)
    want = check(lab, img, None, [7, 0, 12])
    assert want.shape == (19, 3, 11) and want[:7, 0, 0].any() and want[7:, 0, 0].any()
    jobs = np.concatenate([ms.jobs_from_stats(ms.labelmetrics.label_stats_host(lab[i], k), i) for i, k in ((0, 7), (2, 12))])
    mixed = jobs[np.random.default_rng(0).permutation(len(jobs))]    # jobs of the images interleaved
    got = check(lab, img, Q8, jobs=mixed)
    assert len(set(mixed[:6, 0].tolist())) == 2 and got[:, 0, 0].any()
    swapped = iq.quantiles_host(lab[::-1], [12, 0, 7], img[::-1])
    assert np.array_equal(swapped[12:], want[:7]) and not np.array_equal(want[:7], iq.quantiles_host(lab, [7, 0, 12], img[::-1])[:7])


def test_hostile_tables_between_guard_rows():
    H, W, nimg = 33, 47, 2
    lab = np.stack([blob_map(H, W, 9, 5), blob_map(H, W, 9, 6)])
    img = seeded_image((nimg, H, W), 2, np.uint16, 3)
    jobs = [[0, 3, -50, -50, H + 50, W + 50], [1, 3, -1, -1, H + 1, W + 1], [0, 2, I32.min, I32.min, I32.max, I32.max],
            [0, 3, 20, 30, 10, 40], [0, 3, I32.max, I32.max, I32.min, I32.min], [0, 3, I32.max - 1, I32.max - 1, I32.max, I32.max],
            [0, 77, 0, 0, H, W], [nimg, 3, 0, 0, H, W], [-1, 3, 0, 0, H, W], [I32.max, 3, 0, 0, H, W], [I32.min, 3, 0, 0, H, W],
            [1, 4, H - 1, W - 1, H + 9, W + 9], [1, 4, H, W, H + 9, W + 9], [1, 5, 2, 3, 30, 44]]
    jobs = np.array(jobs + [[1, 5, 2, 3, 30, 44]] * 600, np.int64)
    table = np.array([[1, 2], [1, 0], [3, 2], [-1, 4], [1, -4], [I32.max, I32.max], [I32.min, I32.min], [1, 3]], np.int32)
    valid = [0, 5, 7]                                                # the rows with 0 <= num <= den, den > 0 (INT_MAX / INT_MAX is 1)
    part = iq.quantiles_host(lab, jobs, img, [F(1, 2), F(1), F(1, 3)])
    want = np.zeros((len(jobs), 2, 17), np.int64)
    want[:, :, 0] = part[:, :, 0]
    for a, k in enumerate(valid):
        want[:, :, 1 + 2 * k:3 + 2 * k] = part[:, :, 1 + 2 * a:3 + 2 * a]
    assert want[0, 0, 0] > 0 and want[1, 0, 0] > 0 and want[2, 0, 0] > 0 and not want[3:11].any() and want[13, 0, 0] > 0
    guard = torch.full((len(jobs) + 2, 2, 17), -7, dtype=torch.int32, device=DEV)           # rows in front of and behind the output
    d, dj, di, dq = up(lab), up(jobs.astype(np.int32)), up(img), up(table)
    _lib.call("kg_label_quantiles", ptr(d), nimg, H, W, ptr(di), 2, 2, ptr(dj), len(jobs), ptr(dq), 8, ptr(guard[1:]), stream_ptr())
    g = guard.cpu().numpy()
    assert np.array_equal(g[1:-1], want) and (g[0] == -7).all() and (g[-1] == -7).all()
    assert (g[15:-1] == g[15]).all()                                  # every copy of the repeated job is identical
    # the histogram entry with the same boxes and hostile channel / shift / prefix columns
    tail = np.array([[0, 8, -1], [1, 0, -1], [2, 0, -1], [-1, 0, -1], [0, 9, -1], [0, -1, -1], [1, 4, I32.max], [1, 4, I32.min], [I32.min, I32.min, 0]])
    j9 = np.concatenate([np.repeat(jobs[:14], len(tail), 0), np.tile(tail, (14, 1))], 1)
    hw = iq.histograms_host(lab, j9, img)
    hg = torch.full((len(j9) + 2, 256), -7, dtype=torch.int32, device=DEV)
    _lib.call("kg_label_histograms", ptr(d), nimg, H, W, ptr(di), 2, 2, ptr(up(j9.astype(np.int32))), len(j9), ptr(hg[1:]), stream_ptr())
    g = hg.cpu().numpy()
    assert np.array_equal(g[1:-1], hw) and (g[0] == -7).all() and (g[-1] == -7).all() and hw.any()
    assert iq.quantile_rows(d, np.zeros((0, 6), np.int64), img).shape == (0, 2, 11)          # m == 0 launches nothing


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_large_object_unsplit_and_through_the_histogram_route(dtype):
    H = W = 300
    lab = np.ones((H, W), np.int32)
    lab[100:140, 100:150] = 2
    img = seeded_image((H, W), 3, dtype, 12)
    if dtype == np.uint16:
        img[..., 1] >>= 4
    want = iq.quantiles_host(lab, 2, img, Q8)
    d = up(lab)
    whole = iq.quantiles(d, 2, image=img, q=Q8, max_job_pixels=2 ** 30)                      # one workgroup walks 90000 pixels
    cut = iq.quantiles(d, 2, image=img, q=Q8, max_job_pixels=4096)                           # 300 x 300 in pieces, 40 x 50 in the kernel
    assert np.array_equal(whole.raw, want) and np.array_equal(cut.raw, whole.raw) and want[0, 0, 0] == 88000
    tiny = iq.quantiles(d, 2, image=img, q=Q8, max_job_pixels=1000)                          # both through the histogram route
    assert np.array_equal(tiny.raw, want)
    h = iq.histograms(d, 2, image=img, max_job_pixels=4096)
    jobs = ms.jobs_from_stats(ms.labelmetrics.label_stats_host(lab, 2))
    assert np.array_equal(h.counts.reshape(-1, 256), iq.histograms_host(lab, all_channel_jobs(jobs, 3, h.shift), img))


def test_grid_stride():
    """1 048 584 one-pixel jobs, more than the grid cap of 2^20 blocks: the workgroups stride and reuse their LDS.  The expected row is the
    closed form {1, v, v}, built vectorised on the device."""
    H, W, m = 1025, 1024, 2 ** 20 + 8
    lab = (torch.arange(H * W, dtype=torch.int32, device=DEV) % 7 + 1).view(H, W)
    img = ((torch.arange(H * W, dtype=torch.int64, device=DEV) * 2654435761 >> 13) & 255).to(torch.uint8).view(H, W, 1)
    p = torch.arange(m, dtype=torch.int32, device=DEV)
    y, x = p // W, p % W
    jobs = torch.stack([torch.zeros_like(p), lab.view(-1)[:m], y, x, y + 1, x + 1], 1).contiguous()
    guard = torch.full((m + 2, 1, 3), -7, dtype=torch.int32, device=DEV)
    qd = up(iq.q_table([F(1, 2)]))
    _lib.call("kg_label_quantiles", ptr(lab), 1, H, W, ptr(img), 1, 1, ptr(jobs), m, ptr(qd), 1, ptr(guard[1:]), stream_ptr())
    v = img.view(-1)[:m].to(torch.int32)
    want = torch.stack([torch.ones_like(v), v, v], 1).view(m, 1, 3)
    assert bool((guard[1:-1] == want).all()) and bool((guard[0] == -7).all()) and bool((guard[-1] == -7).all())
    assert int(v.max()) == 255 and int(v.min()) == 0
    jobs[:, 1] = 8                                                    # no pixel holds 8: zeros everywhere, from the same striding blocks
    _lib.call("kg_label_quantiles", ptr(lab), 1, H, W, ptr(img), 1, 1, ptr(jobs), m, ptr(qd), 1, ptr(guard[1:]), stream_ptr())
    assert not bool(guard[1:-1].any()) and bool((guard[0] == -7).all()) and bool((guard[-1] == -7).all())


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


def test_predict_tiled_with_quantiles(cal_model):
    H, W, S = 400, 600, 256
    img = np.random.default_rng(8).integers(0, 256, (H, W, 3), dtype=np.uint8)
    plain = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4)
    got = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4, quantiles=True)
    n = len(plain)
    assert n > 0 and plain.quantiles is None and got.measurements is None and same_instances(got, plain)   # the default path is untouched
    assert isinstance(got.quantiles, iq.Quantiles) and got.quantiles.channels == 3 and got.quantiles.q == iq.DEFAULT_Q
    assert np.array_equal(got.quantiles.raw, iq.quantiles_host(got.labels.cpu().numpy(), n, img))
    assert np.array_equal(got.quantiles.counts(), got.table[:, 1]) and got.quantiles.median().shape == (n, 3)
    # with clean=, expand= and measure= as well: taken on the final map (a device image and a dict this time)
    policy = dict(min_area=4)
    both = tiling.predict_tiled(cal_model, up(img), tile=S, overlap=64, batch=4, clean=policy, expand=2, measure=True,
                                quantiles={"q": [0.5, (1, 3)], "max_job_pixels": 64})
    final = distance.expand_instances(cc.clean_instances(plain, **policy), 2)
    assert final.quantiles is None and same_instances(both, final) and both.quantiles.q == (F(1, 2), F(1, 3))
    assert np.array_equal(both.quantiles.raw, iq.quantiles_host(both.labels.cpu().numpy(), n, img, [F(1, 2), F(1, 3)]))
    assert np.array_equal(both.quantiles.counts(), both.table[:, 1]) and np.array_equal(both.measurements.raw[:, 0], both.table[:, 1])
    assert ((both.table[:, 4] - both.table[:, 2]) * (both.table[:, 5] - both.table[:, 3]) > 64).any()   # some took the histogram route


def test_predict_instances_with_quantiles(cal_model):
    S = 256
    src = np.random.default_rng(9).integers(0, 256, (2, S, S, 3), dtype=np.uint8)
    x = torch.cat([tiling.cut_tiles(src[i], tiling.plan(S, S, S, 64)) for i in range(2)])
    plain = inference.predict_instances(cal_model, x)
    assert all(p is not None and len(p) > 0 and p.quantiles is None for p in plain)
    inten = np.random.default_rng(10).integers(0, 65536, (2, S, S, 2)).astype(np.uint16)
    full = inference.predict_instances(cal_model, x, quantiles=inten)
    policy = dict(min_area=4)
    opts = inference.predict_instances(cal_model, x, clean=policy, expand=1.5, quantiles={"image": up(src), "q": [F(1, 4), F(3, 4)]})
    final = distance.expand_instances_batch(cc.clean_instances_batch(inference.predict_instances(cal_model, x), **policy), 1.5)
    for i, (p, f, o, e) in enumerate(zip(plain, full, opts, final)):
        assert same_instances(p, f) and same_instances(o, e) and f.measurements is None
        assert np.array_equal(f.quantiles.raw, iq.quantiles_host(p.labels.cpu().numpy(), len(p), inten[i])) and f.quantiles.channels == 2
        assert np.array_equal(f.quantiles.counts(), f.table[:, 1])
        assert np.array_equal(o.quantiles.raw, iq.quantiles_host(o.labels.cpu().numpy(), len(o), src[i], [F(1, 4), F(3, 4)]))
        assert np.array_equal(o.quantiles.counts(), o.table[:, 1]) and o.quantiles.iqr().shape == (len(o), 3)
