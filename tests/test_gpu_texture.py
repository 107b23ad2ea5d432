"""GPU: per-instance co-occurrence matrices (csrc/texture.hip, texture.py) against the host statement of the same semantics
(texture.glcm_host / glcm_rows_host).  Every comparison is exact integer equality.  Shapes are the smallest at which the kernel can go
wrong: one-pixel, one-row and one-column maps, distances that reach past every side of the map, boxes smaller than their object, box
widths on both sides of the 256-thread walk, both sides of the staged / direct rule and the same object down each route, every level
count, every channel count under both element sizes, a constant image (every atomic on one bin) and a checkerboard, hostile job tables
between guard rows, a job in bands, more jobs than the grid cap, several images and several distances in one launch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from kg_instance_segmentation_amd import KGnet, _lib, inference, tiling  # noqa: E402
from kg_instance_segmentation_amd import components as cc  # noqa: E402
from kg_instance_segmentation_amd import distance as dt  # noqa: E402
from kg_instance_segmentation_amd import measure as ms  # noqa: E402
from kg_instance_segmentation_amd import split as sp  # noqa: E402
from kg_instance_segmentation_amd import texture as tx  # noqa: E402
from kg_instance_segmentation_amd._lib import ptr, stream_ptr  # noqa: E402

DEV = "cuda"
I32 = np.iinfo(np.int32)


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


def check(lab, img, n=None, jobs=None, max_job_pixels=65536, **kw):
    """device glcm == glcm_host; returns the counts"""
    want = tx.glcm_host(lab, n if jobs is None else jobs, img, **kw)
    got = tx.glcm(up(lab), n, jobs, image=img, max_job_pixels=max_job_pixels, **kw)
    assert isinstance(got, tx.CoMatrices) and got.counts.dtype == np.int64 and got.distances == want.distances and got.channels == want.channels
    assert np.array_equal(got.counts, want.counts)
    return want.counts


def rows(lab, img, jobs10, L, guard=-7):
    """kg_label_glcm over raw ten-column jobs between guard rows == glcm_rows_host; returns the rows"""
    lab3 = lab.reshape((-1,) + lab.shape[-2:])
    img4 = img.reshape(lab3.shape + (img.shape[-1],))
    j = np.asarray(jobs10, np.int64).reshape(-1, 10)
    want = tx.glcm_rows_host(lab3, j, img4, L)
    out = torch.full((len(j) + 2, 4, L, L), guard, dtype=torch.int32, device=DEV)
    d, di, dj = up(lab3), up(img4), up(j.astype(np.int32))
    _lib.call("kg_label_glcm", ptr(d), lab3.shape[0], lab3.shape[1], lab3.shape[2], ptr(di), img4.shape[3], img4.dtype.itemsize, ptr(dj), len(j), L,
              ptr(out[1:]), stream_ptr())
    g = out.cpu().numpy()
    assert np.array_equal(g[1:-1], want) and (g[0] == guard).all() and (g[-1] == guard).all()
    return want


@pytest.mark.parametrize("H,W", [(1, 1), (1, 130), (130, 1)])
def test_smallest_maps(H, W):
    n = 6
    lab = np.ones((1, 1), np.int32) if H * W == 1 else blob_map(H, W, n, 10 + H)
    for dtype in (np.uint8, np.uint16):
        img = seeded_image((H, W), 2, dtype, 1)
        c = check(lab, img, 1 if H * W == 1 else n, distance=(1, 2, 32))
        if H * W == 1:
            assert not c.any()
        elif H == 1:
            assert c[:, :, :, 0].any() and not c[:, :, :, 1:].any()      # one row: only direction 0 has pairs
        else:
            assert c[:, :, :, 2].any() and not c[:, :, :, (0, 1, 3)].any()


def test_distances_past_every_side_and_boxes_smaller_than_their_object():
    H, W = 20, 23
    lab = np.ones((H, W), np.int32)                                     # one object fills the map: every partner test is the map's edge
    lab[7:9, 5:17] = 2
    img = seeded_image((H, W), 1, np.uint8, 2)
    c = check(lab, img, 2, distance=(1, 2, 19, 22, 23, 32), levels=8)
    assert c[0, 0, 3, 0].any() and not c[0, 0, 4].any() and not c[0, 0, 5].any()      # d = 22: direction 0 alone; d >= 23: nothing
    assert c[0, 0, 2, 2].any() and not c[0, 0, 3, 2].any()
    # boxes that cut the object: partners lie outside the box, in every direction; pieces add up
    jobs = np.array([[0, 1, 5, 5, 9, 9], [0, 1, 0, 0, 3, W], [0, 1, H - 2, 0, H, W], [0, 1, 0, W - 2, H, W], [0, 1, 0, 0, H, 2], [0, 1, 6, 4, 10, 18],
                     [0, 2, 7, 5, 8, 17], [0, 2, 8, 5, 9, 17], [0, 2, 7, 5, 9, 17]])
    for d in (1, 3):
        c = check(lab, img, jobs=jobs, distance=d, levels=8)
        assert c[0, 0, 0, 0].sum() == 8 and np.array_equal(c[6] + c[7], c[8]) and c[6, 0, 0, 2].sum() == (12 if d == 1 else 0)


@pytest.mark.parametrize("w", [1, 255, 256, 257])
def test_box_widths_heights_and_distances(w):
    H, W = 140, 300
    lab = np.zeros((H, W), np.int32)
    img = seeded_image((H, W), 1, np.uint8, w)
    jobs = []
    for k, h in enumerate((1, 127, 128)):
        lab[:] = 0
        lab[5:5 + h, 7:7 + w] = 1
        lab[5:5 + h:9, 7:7 + w:5] = 0                                   # holes: the object is ragged inside its box
        jobs = [[0, 1, 5, 7, 5 + h, 7 + w]]
        c = check(lab, img, jobs=jobs, distance=(1, 2, 32), levels=16, max_job_pixels=2 ** 30)
        assert c.any() or (w == 1 and h == 1)
    lab[:] = 0
    lab[3:130, 40:45] = 3                                               # narrower than d
    c = check(lab, img, 3, distance=(4, 5, 6), levels=4)
    assert c[2, 0, 0, 0].any() and not c[2, 0, 1, 0].any() and c[2, 0, 2, 2].any() and not c[2, 0, 2, (0, 1, 3)].any()


def test_both_sides_of_the_route_rule():
    H, W = 200, 200
    lab = blob_map(H, W, 5, 7)
    lab[10:190, 10:190][lab[10:190, 10:190] == 0] = 6
    img = seeded_image((H, W), 2, np.uint16, 8)
    jobs = []
    for h, w, d in ((126, 126, 1), (127, 126, 1), (128, 126, 1), (127, 127, 1), (96, 64, 32), (97, 64, 32), (96, 65, 32), (126, 124, 2), (127, 124, 2)):
        jobs.append((tx.fits(h, w, d), d, [0, 6, 20, 30, 20 + h, 30 + w]))
    assert [f for f, _, _ in jobs] == [True, True, False, False, True, False, False, True, False]
    for d in (1, 2, 32):
        j = np.array([b for _, dd, b in jobs if dd == d])
        assert check(lab, img, jobs=j, distance=d, levels=32, max_job_pixels=2 ** 30).any()
    # the same object down each route: its own box is staged, a padded box is not; the rows are the same
    lab2 = np.zeros((H, W), np.int32)
    lab2[60:100, 50:120] = 1
    lab2[70:75, 60:70] = 0
    for d in (1, 7):
        tight, padded = [0, 1, 60, 50, 100, 120], [0, 1, 0, 0, H, W]
        assert tx.fits(40, 70, d) and not tx.fits(H, W, d)
        c = check(lab2, img, jobs=np.array([tight, padded]), distance=d, channels=1, max_job_pixels=2 ** 30)
        assert np.array_equal(c[0], c[1]) and c[0].any()


def test_large_object_unsplit_and_in_bands():
    H = W = 300
    lab = np.ones((H, W), np.int32)
    lab[100:140, 100:150] = 2
    img = seeded_image((H, W), 2, np.uint8, 12)
    whole = check(lab, img, 2, distance=(1, 3), max_job_pixels=2 ** 30)   # one workgroup walks 90000 pixels, straight from global memory
    cut = check(lab, img, 2, distance=(1, 3), max_job_pixels=4096)        # 300 x 300 in 13-row bands, staged; 40 x 50 whole
    assert np.array_equal(whole, cut) and whole[0, 0, 0, 0].sum() == 300 * 299 - 40 * 51


@pytest.mark.parametrize("L", [2, 3, 16, 32])
def test_levels_channels_and_ranges(L):
    H, W, n = 37, 53, 8                                                 # an odd width: pixels of 1 .. 8 bytes at odd offsets
    lab = blob_map(H, W, n, L)
    for dtype in (np.uint8, np.uint16):
        top = np.iinfo(dtype).max
        for C in (1, 2, 3, 4):
            img = seeded_image((H, W), C, dtype, 10 * C + L)
            assert check(lab, img, n, levels=L).any()
        lo, hi = top // 4, top // 2                                     # values below lo and above hi on both sides
        c = check(lab, img, n, levels=L, range=(lo, hi), channels=(3, 0))
        assert c[:, :, :, :, 0, 0].any() and c[:, :, :, :, L - 1, L - 1].any()
        check(lab, img, n, levels=L, range=[(0, 9), (lo, hi), (top - 1, top), (-5, top + 5)])
        check(lab, img, n, levels=L, range="object", distance=2)


def test_constant_image_and_checkerboard():
    H, W = 90, 110
    lab = blob_map(H, W, 4, 3)
    lab[lab == 0] = 5
    yy, xx = np.mgrid[0:H, 0:W]
    const = np.full((H, W, 1), 200, np.uint8)
    c = check(lab, const, 5, distance=(1, 2))
    assert np.array_equal(c[:, 0, :, :, 12, 12], c.sum((-1, -2))[:, 0]) and c.any()     # every atomic of a direction hits one bin
    chk = (((yy + xx) & 1) * 65535).astype(np.uint16)[..., None]
    c = check(lab, chk, 5, levels=2, distance=(1, 2))
    assert not c[:, 0, 0, (0, 2)][..., (0, 1), (0, 1)].any() and not c[:, 0, 0, (1, 3)][..., (0, 1), (1, 0)].any() and c[:, 0, 1].any()
    whole = check(lab, chk, jobs=np.array([[0, 5, 0, 0, H, W]]), levels=2, max_job_pixels=2 ** 30)   # the direct route on a constant pair of bins
    assert np.array_equal(whole[0], c[4][:, :1])


def test_ids():
    H, W = 33, 70
    lab = blob_map(H, W, 9, 5)
    lab[3:6, 10:60] = -1
    lab[8:11, 5:50] = I32.min
    lab[20:25, 30:69] = I32.max
    img = seeded_image((H, W), 3, np.uint8, 3)
    jobs = np.array([[0, v, 0, 0, H, W] for v in (0, -1, I32.min, I32.max, 3, 77)], np.int64)
    c = check(lab, img, jobs=jobs, levels=8)
    assert all(c[k].any() for k in range(5)) and not c[5].any()
    assert c[1, 0, 0, 0].sum() == 3 * 49 and c[2, 0, 0, 2].sum() == 2 * 45 and c[3, 0, 0, 1].sum() == 4 * 38


def test_hostile_jobs_between_guard_rows():
    H, W, nimg, L = 33, 47, 2, 8
    lab = np.stack([blob_map(H, W, 9, 5), blob_map(H, W, 9, 6)])
    for dtype, C in ((np.uint8, 3), (np.uint16, 2)):
        img = seeded_image((nimg, H, W), C, dtype, 3)
        good = [[0, 3, -50, -50, H + 50, W + 50, 0, 1, 0, 256], [1, 3, -1, -1, H + 1, W + 1, C - 1, 2, 10, 100],
                [0, 2, I32.min, I32.min, I32.max, I32.max, 0, 32, -7, 1], [1, 5, 2, 3, 30, 44, 1, 3, I32.min, I32.max],
                [1, 5, 2, 3, 30, 44, 1, 3, I32.max, I32.max], [1, 5, 2, 3, 30, 44, 1, 3, I32.min, 1], [1, 5, 2, 3, 30, 44, 0, 1, 0, I32.max],
                [0, 4, 0, 0, H, W, 0, 1, -65536, 3 * 65536]]
        base = [1, 5, 2, 3, 30, 44, 0, 1, 0, 256]

        def with_(col, v):
            r = list(base)
            r[col] = v
            return r
        bad = ([with_(0, v) for v in (nimg, -1, I32.max, I32.min)]                                  # no such image
               + [with_(6, v) for v in (C, 4, -1, I32.max, I32.min)]                                # no such channel
               + [with_(7, v) for v in (0, 33, -1, I32.max, I32.min)]                               # no such distance
               + [with_(9, v) for v in (0, -1, I32.min)]                                            # no span
               + [[0, 3, 20, 30, 10, 40, 0, 1, 0, 256], [0, 3, I32.max, I32.max, I32.min, I32.min, 0, 1, 0, 256],
                  [0, 3, 5, 5, 5, 9, 0, 1, 0, 256], [0, 3, H, W, H + 9, W + 9, 0, 1, 0, 256], [0, 77, 0, 0, H, W, 0, 1, 0, 256],
                  [I32.min, I32.min, I32.min, I32.min, I32.min, I32.min, I32.min, I32.min, I32.min, I32.min],
                  [I32.max, I32.max, I32.max, I32.max, I32.max, I32.max, I32.max, I32.max, I32.max, I32.max]])
        jobs = [r for k, b in enumerate(bad) for r in (good[k % len(good)], b)] + [base] * 300
        want = rows(lab, img, jobs, L)
        nb = len(bad)
        assert want[0].any() and want[2].any() and want[0:2 * nb:2].any((1, 2, 3)).sum() > nb // 2 and not want[1:2 * nb:2].any()
        assert (want[2 * nb:] == want[2 * nb]).all() and want[2 * nb].any()                         # every copy of the repeated job is identical
    assert tx.glcm_rows(up(lab), np.zeros((0, 10), np.int64), img, 4).shape == (0, 4, 4, 4)       # m == 0 launches nothing


def test_three_images_interleaved_and_several_distances():
    H, W = 40, 67
    lab = np.stack([blob_map(H, W, 7, 1), np.zeros((H, W), np.int32), blob_map(H, W, 12, 2)])
    img = seeded_image((3, H, W), 3, np.uint16, 4)
    c = check(lab, img, [7, 0, 12], distance=(1, 3, 2), levels=8, channels=(2, 0))
    assert c.shape == (19, 2, 3, 4, 8, 8) and c[:7].any() and c[7:].any()
    one = check(lab, img, [7, 0, 12], distance=3, levels=8, channels=2)
    assert np.array_equal(one[:, 0, 0], c[:, 0, 1])
    jobs = np.concatenate([ms.jobs_from_stats(ms.labelmetrics.label_stats_host(lab[i], k), i) for i, k in ((0, 7), (2, 12))])
    mixed = jobs[np.random.default_rng(0).permutation(len(jobs))]       # jobs of the images interleaved
    got = check(lab, img, jobs=mixed, levels=8)
    assert len(set(mixed[:6, 0].tolist())) == 2 and got.any()
    dj = tx.glcm(up(lab), jobs=up(mixed.astype(np.int32)), image=up(img), levels=8)              # device jobs, a device image
    assert np.array_equal(dj.counts, got)


def test_grid_stride():
    """1 048 584 one-pixel jobs at L = 2 and d = 1, more than the grid cap of 2^20 blocks: the workgroups stride and reuse their LDS.  A
    one-pixel box still has partners in the map; the expected rows are built vectorised on the device."""
    H, W, m, L = 1025, 1024, 2 ** 20 + 8, 2
    cell = torch.arange(H, dtype=torch.int64, device=DEV)[:, None] // 2 * W + torch.arange(W, dtype=torch.int64, device=DEV)[None, :] // 2
    lab = ((cell * 2654435761 >> 11) % 3 + 1).to(torch.int32).contiguous()          # 2 x 2 cells of three ids: partners of every direction
    img = ((torch.arange(H * W, dtype=torch.int64, device=DEV) * 2654435761 >> 13) & 255).to(torch.uint8).view(H, W, 1)
    p = torch.arange(m, dtype=torch.int32, device=DEV)
    y, x = p // W, p % W
    one, zero = torch.ones_like(p), torch.zeros_like(p)
    jobs = torch.stack([zero, lab.view(-1)[:m], y, x, y + 1, x + 1, zero, one, zero, one * 256], 1).contiguous()
    guard = torch.full((m + 2, 4, L, L), -7, dtype=torch.int32, device=DEV)
    _lib.call("kg_label_glcm", ptr(lab), 1, H, W, ptr(img), 1, 1, ptr(jobs), m, L, ptr(guard[1:]), stream_ptr())
    lev = (img.view(H, W) >> 7).to(torch.int64)
    want = torch.zeros((m, 4, L * L), dtype=torch.int32, device=DEV)
    yy, xx = y.long(), x.long()
    for k, (dy, dx) in enumerate(tx.OFFSETS):
        qy, qx = yy + dy, xx + dx
        inside = (qy < H) & (qx >= 0) & (qx < W)
        qy, qx = qy.clamp(max=H - 1), qx.clamp(0, W - 1)
        hit = inside & (lab[qy, qx] == lab[yy, xx])
        want[:, k].scatter_(1, (lev[yy, xx] * L + lev[qy, qx]).view(-1, 1), hit.to(torch.int32).view(-1, 1))
    assert bool((guard[1:-1].view(m, 4, L * L) == want).all()) and bool((guard[0] == -7).all()) and bool((guard[-1] == -7).all())
    assert all(int(want[:, k].sum()) > m // 8 for k in range(4)) and int(want.max()) == 1
    jobs[:, 1] = 8                                                      # no pixel holds 8: zeros everywhere, from the same striding blocks
    _lib.call("kg_label_glcm", ptr(lab), 1, H, W, ptr(img), 1, 1, ptr(jobs), m, L, ptr(guard[1:]), stream_ptr())
    assert not bool(guard[1:-1].any()) and bool((guard[0] == -7).all()) and bool((guard[-1] == -7).all())


def test_entry_refuses_bad_arguments_before_any_launch():
    import ctypes
    lib = _lib.load()
    name = "kg_label_glcm"
    lab = torch.zeros((8, 8), dtype=torch.int32, device=DEV)
    img = torch.zeros((8, 8, 3), dtype=torch.int16, device=DEV)
    jobs = torch.zeros((3, 10), dtype=torch.int32, device=DEV)
    out = torch.full((3, 4, 16, 16), -7, dtype=torch.int32, device=DEV)
    P, IMG, JOBS, OUT = (ctypes.c_void_p(t.data_ptr()) for t in (lab, img, jobs, out))

    def off(t, k):
        return ctypes.c_void_p(t.data_ptr() + k)

    def call(labels=P, nimg=1, H=8, W=8, image=IMG, channels=3, elem=1, jobs=JOBS, m=3, levels=16, out=OUT):
        return lib.kg_label_glcm(labels, nimg, H, W, image, channels, elem, jobs, m, levels, out, stream_ptr())

    def err(rc, text):
        msg = lib.kg_last_error().decode()
        assert rc != 0 and name in msg and text in msg, (rc, msg)

    err(call(labels=None), "null pointer")
    err(call(jobs=None), "null pointer")
    err(call(out=None), "null pointer")
    err(call(image=None), "null pointer")
    for v in (0, 5, -1):
        err(call(channels=v), f"channels {v}")
    for v in (3, 0):
        err(call(elem=v), f"elem_bytes {v}")
    for v in (1, 33, 0, -16):
        err(call(levels=v), f"levels {v}")
    err(call(H=32769), "32768")
    err(call(W=32769), "32768")
    err(call(nimg=0), "bad size")
    err(call(H=0), "bad size")
    err(call(W=-1), "bad size")
    err(call(m=-1), "bad size")
    err(call(nimg=3, H=32768, W=32768), "exceeds 2^31 - 1")
    err(call(out=off(out, 2)), "misaligned")
    err(call(labels=off(lab, 2)), "misaligned")
    err(call(jobs=off(jobs, 1)), "misaligned")
    err(call(image=off(img, 1), elem=2), "misaligned")
    assert call(m=0) == 0 and call(m=0, jobs=None, out=None) == 0
    torch.cuda.synchronize()
    assert bool((out == -7).all())                                      # nothing was launched by any refused call


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


def others_untouched(a):
    return all(getattr(a, k) is None for k in ("measurements", "neighbours", "runs", "contours", "hulls", "quantiles"))


def test_predict_tiled_with_texture(cal_model):
    H, W, S = 400, 600, 256
    img = np.random.default_rng(8).integers(0, 256, (H, W, 3), dtype=np.uint8)
    plain = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4)
    none = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4, texture=None)
    got = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4, texture=True)
    n = len(plain)
    assert n > 0 and plain.texture is None and none.texture is None and same_instances(none, plain) and others_untouched(none)
    assert same_instances(got, plain) and others_untouched(got) and got.parent is None                 # the other fields are untouched
    assert isinstance(got.texture, tx.CoMatrices) and got.texture.counts.shape == (n, 3, 1, 4, 16, 16)
    assert np.array_equal(got.texture.counts, tx.glcm_host(got.labels.cpu().numpy(), n, img).counts) and got.texture.counts.any()
    assert got.texture.haralick().shape == (n, 3, 1, 4, 13)
    # with clean=, split=, expand= and measure= as well: taken on the final map (a device image and a dict this time)
    policy = dict(min_area=4)
    kw = {"levels": 8, "distance": (1, 2), "range": "object", "channels": (2, 0), "max_job_pixels": 64}
    both = tiling.predict_tiled(cal_model, up(img), tile=S, overlap=64, batch=4, clean=policy, split=2, expand=2, measure=True, texture=kw)
    final = dt.expand_instances(sp.split_instances(cc.clean_instances(plain, **policy), 2), 2)
    assert final.texture is None and same_instances(both, final) and both.texture.distances == (1, 2) and both.texture.channels == (2, 0)
    host = both.labels.cpu().numpy()
    want = tx.glcm_host(host, len(both), img, levels=8, distance=(1, 2), range="object", channels=(2, 0))
    assert np.array_equal(both.texture.counts, want.counts) and want.counts.any()
    assert ((both.table[:, 4] - both.table[:, 2]) * (both.table[:, 5] - both.table[:, 3]) > 64).any()   # some went through in bands
    # range="object" without measure=: measured on the way, the same matrices; and another image through the dict
    alone = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4, clean=policy, split=2, expand=2, texture=dict(kw, max_job_pixels=65536))
    assert alone.measurements is None and np.array_equal(alone.texture.counts, want.counts)
    wide = np.random.default_rng(9).integers(0, 65536, (H, W, 1)).astype(np.uint16)
    other = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4, texture={"image": wide, "levels": 4, "range": (0, 4095)})
    assert np.array_equal(other.texture.counts, tx.glcm_host(plain.labels.cpu().numpy(), n, wide, levels=4, range=(0, 4095)).counts)


def test_predict_instances_with_texture(cal_model):
    S = 256
    src = np.random.default_rng(9).integers(0, 256, (2, S, S, 3), dtype=np.uint8)
    x = torch.cat([tiling.cut_tiles(src[i], tiling.plan(S, S, S, 64)) for i in range(2)])
    plain = inference.predict_instances(cal_model, x)
    none = inference.predict_instances(cal_model, x, texture=None)
    assert all(p is not None and len(p) > 0 and p.texture is None for p in plain)
    assert all(same_instances(a, b) and a.texture is None and others_untouched(a) for a, b in zip(none, plain))
    inten = np.random.default_rng(10).integers(0, 65536, (2, S, S, 2)).astype(np.uint16)
    full = inference.predict_instances(cal_model, x, texture=inten)
    policy = dict(min_area=4)
    kw = {"levels": 32, "distance": (2, 1), "range": "object"}
    opts = inference.predict_instances(cal_model, x, clean=policy, split=2, expand=1.5, texture=dict(kw, image=up(src)))
    meas = inference.predict_instances(cal_model, x, clean=policy, split=2, expand=1.5, measure=src, texture=dict(kw, image=src))
    final = dt.expand_instances_batch(sp.split_instances_batch(cc.clean_instances_batch(inference.predict_instances(cal_model, x), **policy), 2), 1.5)
    for i, (p, f, o, e, q) in enumerate(zip(plain, full, opts, final, meas)):
        assert same_instances(p, f) and same_instances(o, e) and same_instances(q, e) and others_untouched(f) and e.texture is None
        assert np.array_equal(f.texture.counts, tx.glcm_host(p.labels.cpu().numpy(), len(p), inten[i]).counts) and f.texture.counts.shape[1] == 2
        want = tx.glcm_host(o.labels.cpu().numpy(), len(o), src[i], **kw).counts
        assert np.array_equal(o.texture.counts, want) and np.array_equal(q.texture.counts, want) and want.any()
        assert o.texture.distances == (2, 1) and o.texture.props()["entropy"].shape == (len(o), 3, 2)
