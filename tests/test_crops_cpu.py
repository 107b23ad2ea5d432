"""CPU: the host statement of the instance crops (crops.crops_host, the yardstick of the GPU tests) against a per-pixel plain-Python
evaluation of the rule, its closed forms, the textbook align_corners=False formula and torch's interpolate; the job tables of
crops.affine_jobs; the `crops` slot, the crops=None defaults and the C entry's host checks.  No compute entry point is launched."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from kg_instance_segmentation_amd import _lib, inference, instances, tiling
from kg_instance_segmentation_amd import crops as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32 = np.iinfo(np.int32)
ONE = 65536


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


def brute(lab, jobs, img, OH, OW, nearest, masked, fill):
    """the rule of include/kgnet_hip.h, pixel by pixel, in Python integers"""
    lab = lab.reshape((-1,) + lab.shape[-2:])
    nimg, H, W = lab.shape
    img = None if img is None else img.reshape(lab.shape + (img.shape[-1],))
    C = 0 if img is None else img.shape[3]
    patches = np.zeros((len(jobs), C, OH, OW), np.int64)
    masks = np.zeros((len(jobs), OH, OW), np.uint8)
    for a, (im, v, oy, ox, ay, by, cy, ax, bx, cx) in enumerate(np.asarray(jobs).tolist()):
        live = 0 <= im < nimg

        def tap(y, x, c):
            return int(img[im, y, x, c]) if live and 0 <= y < H and 0 <= x < W else fill
        for i in range(OH):
            for j in range(OW):
                Y, X = (oy << 16) + ay * i + by * j + cy, (ox << 16) + ax * i + bx * j + cx
                yn, xn = (Y + 32768) >> 16, (X + 32768) >> 16
                mk = int(live and 0 <= yn < H and 0 <= xn < W and int(lab[im, yn, xn]) == v)
                masks[a, i, j] = mk
                for c in range(C):
                    if nearest:
                        r = tap(yn, xn, c)
                    else:
                        y0, x0, fy, fx = Y >> 16, X >> 16, Y & 65535, X & 65535
                        acc = (ONE - fy) * ((ONE - fx) * tap(y0, x0, c) + fx * tap(y0, x0 + 1, c)) \
                            + fy * ((ONE - fx) * tap(y0 + 1, x0, c) + fx * tap(y0 + 1, x0 + 1, c))
                        assert 0 <= acc < 2 ** 48
                        r = (acc + 2 ** 31) >> 32
                    patches[a, c, i, j] = fill if masked and not mk else r
    return patches, masks


def ragged_jobs(nimg, H, W, rng, k):
    """k jobs with ragged scales, shears, negative coefficients and origins on every side of the map"""
    j = np.zeros((k, 10), np.int64)
    j[:, 0] = rng.integers(0, nimg, k)
    j[:, 1] = rng.integers(0, 7, k)
    j[:, 2] = rng.integers(-6, H + 3, k); j[:, 3] = rng.integers(-6, W + 3, k)
    j[:, [4, 8]] = rng.integers(-3 * ONE, 3 * ONE, (k, 2))
    j[:, [5, 7]] = rng.integers(-ONE, ONE, (k, 2))
    j[:, [6, 9]] = rng.integers(-2 * ONE, 2 * ONE, (k, 2))
    j[0] = [0, 1, 2, 3, ONE, 0, 0, 0, ONE, 0]
    return j


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_host_against_a_per_pixel_loop(dtype, C):
    nimg, H, W, OH, OW = 2, 19, 23, 5, 7
    rng = np.random.default_rng(10 * C + np.dtype(dtype).itemsize)
    lab = np.stack([blob_map(H, W, 6, 1), blob_map(H, W, 6, 2)])
    img = seeded_image((nimg, H, W), C, dtype, C)
    jobs = ragged_jobs(nimg, H, W, rng, 9)
    for mode in cr.MODES:
        for masked in (False, True):
            wp, wm = brute(lab, jobs, img, OH, OW, mode == "nearest", masked, 7)
            gp, gm = cr.crops_host(lab, jobs, img, (OH, OW), mode, masked, 7)
            assert gp.dtype == dtype and gm.dtype == np.uint8 and gp.shape == (9, C, OH, OW) and gm.shape == (9, OH, OW)
            assert np.array_equal(gp, wp) and np.array_equal(gm, wm) and wm.any() and not wm.all() and (wp != 7).any()
    gp, none = cr.crops_host(lab, jobs, img, (OH, OW), masks=False)
    assert none is None and np.array_equal(gp, brute(lab, jobs, img, OH, OW, False, False, 0)[0])
    none, gm = cr.crops_host(lab, jobs, None, (OH, OW))
    assert none is None and np.array_equal(gm, wm)
    one = cr.crops_host(lab[0], jobs[:1], img[0], 4)                       # one map, one image
    assert np.array_equal(one[0][0], np.moveaxis(img[0, 2:6, 3:7], 2, 0))
    with pytest.raises(_lib.KGLibraryError):
        cr.crops_host(lab, jobs, None, 4, masks=False)


def job(img=0, v=1, oy=0, ox=0, ay=ONE, by=0, cy=0, ax=0, bx=ONE, cx=0):
    return [img, v, oy, ox, ay, by, cy, ax, bx, cx]


def test_closed_forms():
    H, W = 40, 52
    lab = blob_map(H, W, 5, 3)
    lab[9:17, 22:29] = 3                                                    # ragged inside the windows below
    lab[11, 23:26] = 2
    for dtype in (np.uint8, np.uint16):
        top = np.iinfo(dtype).max
        img = seeded_image((H, W), 3, dtype, 4)
        # ay = bx = 65536, the rest 0: an exact copy of the slice, in both modes
        for mode in cr.MODES:
            p, m = cr.crops_host(lab, [job(v=2, oy=5, ox=9)], img, (16, 24), mode)
            assert np.array_equal(p[0], np.moveaxis(img[5:21, 9:33], 2, 0)) and np.array_equal(m[0], lab[5:21, 9:33] == 2)
        # 2x down: the mean of each 2 x 2 block rounded half up
        p, _ = cr.crops_host(lab, [job(oy=4, ox=6, ay=2 * ONE, bx=2 * ONE, cy=ONE // 2, cx=ONE // 2)], img, (10, 12))
        blk = img[4:24, 6:30].astype(np.int64).reshape(10, 2, 12, 2, 3).sum((1, 3))
        assert np.array_equal(p[0], np.moveaxis((blk + 2) >> 2, 2, 0))
        # an image at the top of its type stays there under any fractions
        full = np.full((H, W, 2), top, dtype)
        rng = np.random.default_rng(5)
        jobs = [job(oy=10, ox=12, ay=int(a), bx=int(b), cy=int(c), cx=int(d), by=int(e), ax=int(f))
                for a, b, c, d, e, f in rng.integers(-40000, 40000, (12, 6))]
        p, _ = cr.crops_host(lab, jobs, full, (9, 9), fill=top)
        assert (p == top).all()
        # {ay, by, ax, bx} = {0, -65536, 65536, 0}: np.rot90(k=-1) of the unrotated patch and of its mask
        S = 12
        up, um = cr.crops_host(lab, [job(v=3, oy=8, ox=20)], img, S)
        rp, rm = cr.crops_host(lab, [job(v=3, oy=8 + S - 1, ox=20, ay=0, by=-ONE, ax=ONE, bx=0)], img, S)
        assert np.array_equal(rp[0], np.rot90(up[0], k=-1, axes=(1, 2))) and np.array_equal(rm[0], np.rot90(um[0], k=-1)) and um.any()


def test_windows_outside_the_map_and_over_every_side_and_corner():
    H, W, S = 14, 17, 8
    lab = np.full((H, W), 4, np.int32)
    img = seeded_image((H, W), 2, np.uint8, 6)
    img[img == 7] = 8
    pad = np.full((H + 4 * S, W + 4 * S, 2), 7, np.uint8)
    pad[2 * S:2 * S + H, 2 * S:2 * S + W] = img
    spots = [(-2 * S, 3), (H + 1, 3), (3, -S - 1), (3, W), (-3, 4), (H - 3, 4), (4, -3), (4, W - 3), (-3, -3), (-3, W - 4), (H - 4, -3), (H - 4, W - 4),
             (-S, -S), (H, W)]
    jobs = [job(v=4, oy=y, ox=x) for y, x in spots]
    for mode in cr.MODES:
        p, m = cr.crops_host(lab, jobs, img, S, mode, fill=7)
        for k, (y, x) in enumerate(spots):
            want = pad[2 * S + y:3 * S + y, 2 * S + x:3 * S + x]
            assert np.array_equal(p[k], np.moveaxis(want, 2, 0)), (mode, k)
            inside = np.zeros((H + 4 * S, W + 4 * S), bool)
            inside[2 * S:2 * S + H, 2 * S:2 * S + W] = True
            assert np.array_equal(m[k], inside[2 * S + y:3 * S + y, 2 * S + x:3 * S + x])
        assert (p[0] == 7).all() and (p[1] == 7).all() and (p[2] == 7).all() and (p[3] == 7).all() and not m[:4].any() and not m[12:].any()
    # half a pixel over the edge: the outside tap is fill, weighted; and a bad image index is fill and an empty mask
    p, m = cr.crops_host(lab, [job(v=4, oy=-1, ox=0, cy=ONE // 2), job(img=1, v=4), job(img=-1, v=4), job(img=I32.max, v=4)], img, 4, fill=7)
    assert np.array_equal(p[0, :, 0], (7 + img[0, :4].astype(np.int64).T + 1) >> 1) and m[0].all()
    assert (p[1:] == 7).all() and not m[1:].any()


def textbook(img, wy, wh, wx, ww, OH, OW):
    """align_corners=False bilinear over the whole image (the real context, not the clamped window), float64, rounded half up"""
    H, W = img.shape[:2]
    sy, sx = wy + (np.arange(OH) + 0.5) * wh / OH - 0.5, wx + (np.arange(OW) + 0.5) * ww / OW - 0.5
    y0, x0 = np.floor(sy).astype(int), np.floor(sx).astype(int)
    fy, fx = (sy - y0)[:, None, None], (sx - x0)[None, :, None]
    f = img.astype(np.float64)
    t = lambda y, x: f[np.clip(y, 0, H - 1)[:, None], np.clip(x, 0, W - 1)[None, :]]  # noqa: E731
    v = (1 - fy) * ((1 - fx) * t(y0, x0) + fx * t(y0, x0 + 1)) + fy * ((1 - fx) * t(y0 + 1, x0) + fx * t(y0 + 1, x0 + 1))
    return np.floor(v + 0.5).astype(np.int64)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_power_of_two_ratios_equal_the_textbook_formula_exactly(dtype):
    H, W = 150, 170
    lab = np.ones((H, W), np.int32)
    img = seeded_image((H, W), 2, dtype, 9)
    for (h, w), size in (((32, 64), (16, 16)), ((8, 8), (16, 32)), ((64, 16), (16, 16)), ((4, 128), (32, 32)), ((16, 16), (16, 16)), ((128, 128), (1, 2))):
        box = np.array([[0, 1, 11, 13, 11 + h, 13 + w]])
        t = cr.affine_jobs(box, size, window="box")
        assert t[0, 4] * size[0] == ONE * h and t[0, 8] * size[1] == ONE * w     # the coefficients are exact
        p, _ = cr.crops_host(lab, t, img, size)
        assert np.array_equal(p[0], np.moveaxis(textbook(img, 11, h, 13, w, *size), 2, 0)), (h, w, size)


def test_against_torch_interpolate_on_a_smooth_image():
    """|diff| <= 0.5 + 0.05 against F.interpolate(bilinear, align_corners=False) in float64 at the output positions whose taps lie inside
    the window (torch clamps at the window edge, the rule reads the real context).  0.5 is the rounding; coefficient rounding moves a
    position by at most 2^-9 pixel per axis over 256 steps, and the image's neighbour differences are at most 9 grey levels, so the
    remainder is below 2 * 9 * 2^-9 = 0.036 < 0.05."""
    H, W = 300, 320
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.floor(127.5 + 100 * np.sin(yy / 17.0) * np.cos(xx / 23.0) + 0.5).astype(np.uint8)[..., None]
    assert np.abs(np.diff(img[..., 0].astype(int), axis=0)).max() <= 9 and np.abs(np.diff(img[..., 0].astype(int), axis=1)).max() <= 9
    lab = np.ones((H, W), np.int32)
    worst = 0.0
    for (h, w), size in (((37, 37), (16, 16)), ((50, 71), (64, 64)), ((100, 93), (256, 256)), ((255, 290), (256, 256)), ((201, 17), (33, 5))):
        wy, wx = 21, 14
        t = cr.affine_jobs(np.array([[0, 1, wy, wx, wy + h, wx + w]]), size, window="box")
        p, _ = cr.crops_host(lab, t, img, size)
        ref = torch.nn.functional.interpolate(torch.from_numpy(img[wy:wy + h, wx:wx + w, 0].astype(np.float64))[None, None], size=size,
                                              mode="bilinear", align_corners=False)[0, 0].numpy()
        sy, sx = (np.arange(size[0]) + 0.5) * h / size[0] - 0.5, (np.arange(size[1]) + 0.5) * w / size[1] - 0.5
        ok = ((sy >= 0) & (sy <= h - 1))[:, None] & ((sx >= 0) & (sx <= w - 1))[None, :]
        assert ok.sum() > ok.size // 2
        d = np.abs(p[0, 0].astype(np.float64) - ref)[ok].max()
        worst = max(worst, d)
        assert d <= 0.5 + 0.05, (h, w, size, d)
    print("worst |diff| against torch:", worst)


# ---- affine_jobs ------------------------------------------------------------------------------------------------------------------------

def test_unrotated_tables():
    box = np.array([[0, 5, 10, 20, 26, 36], [1, 6, 10, 20, 25, 36], [2, 7, 3, 4, 40, 9]])
    t = cr.affine_jobs(box, 16)
    assert t.dtype == np.int64 and t.tolist()[0] == [0, 5, 10, 20, ONE, 0, 0, 0, ONE, 0]
    assert t.tolist()[1] == [1, 6, 9, 20, ONE, 0, ONE // 2, 0, ONE, 0]       # 15 x 16: a window of 16 around y = 17.5, [9.5, 25.5)
    assert t.tolist()[2] == [2, 7, 3, -12, 151552, 0, 43008, 0, 151552, 43008]   # 37 -> 16: 37 * 4096, rhu(65536 * 21 / 32)
    assert cr.affine_jobs(box[:1], 8).tolist()[0] == [0, 5, 10, 20, 2 * ONE, 0, ONE // 2, 0, 2 * ONE, ONE // 2]
    assert cr.affine_jobs(box[:1], 32).tolist()[0] == [0, 5, 10, 20, ONE // 2, 0, -ONE // 4, 0, ONE // 2, -ONE // 4]
    assert cr.affine_jobs(box[:1], 16, margin=8).tolist()[0] == [0, 5, 2, 12, 2 * ONE, 0, ONE // 2, 0, 2 * ONE, ONE // 2]
    assert cr.affine_jobs(box[1:2], (19, 20), window="box", margin=2).tolist()[0] == [1, 6, 8, 18, ONE, 0, 0, 0, ONE, 0]
    assert cr.affine_jobs(box[2:], (37, 10), window="box").tolist()[0] == [2, 7, 3, 4, ONE, 0, 0, 0, ONE // 2, -ONE // 4]
    third = cr.affine_jobs(np.array([[0, 1, 0, 0, 1, 1]]), 3)[0]             # 1 -> 3: rhu(65536 / 3), rhu(-65536 / 3)
    assert third.tolist()[4:7] == [21845, 0, -21845]
    assert cr.affine_jobs(np.zeros((0, 6), np.int64), 4).shape == (0, 10)
    for bad in (dict(size=0), dict(size=257), dict(size=(4, 4, 4)), dict(window="round"), dict(margin=-1), dict(flip="x"), dict(side=9),
                dict(angle=0.0, size=(4, 5)), dict(angle=[0.0, 1.0]), dict(angle=float("nan")), dict(angle=0.0, side=0)):
        with pytest.raises(_lib.KGLibraryError):
            cr.affine_jobs(box[:1], **{"size": 16, **bad})


def test_rotated_tables_flips_and_empty_instances():
    box = np.array([[0, 5, 10, 20, 26, 36]])
    S = 16
    q = cr.affine_jobs(box, S, angle=math.pi / 2, side=2 * S)[0].tolist()
    assert [q[4], q[5], q[7], q[8]] == [0, -2 * ONE, 2 * ONE, 0]             # exactly {0, -65536 s', 65536 s', 0}
    assert cr.affine_jobs(box, S, angle=0.0, side=S).tolist() == cr.affine_jobs(box, S).tolist()
    assert cr.affine_jobs(box, S, angle=0.0)[0, 4] == math.floor(ONE * 23 / 16 + 0.5)     # side None: ceil(sqrt(2) * 16) = 23
    lab = blob_map(50, 60, 4, 8)
    lab[11:23, 22:31] = 5                                                   # id 5, ragged inside its box
    lab[14:16, 24:40] = 2
    img = seeded_image((50, 60), 3, np.uint8, 8)
    # the quarter turn about the box centre is the closed form: rot90 of the unrotated patch
    up, um = cr.crops_host(lab, cr.affine_jobs(box, S), img, S)
    rp, rm = cr.crops_host(lab, cr.affine_jobs(box, S, angle=math.pi / 2, side=S), img, S)
    assert np.array_equal(rp[0], np.rot90(up[0], k=-1, axes=(1, 2))) and np.array_equal(rm[0], np.rot90(um[0], k=-1))
    # the centre of the patch is the centre of the box, whatever the angle
    for a in (0.3, -1.2, 2.0):
        c = cr.Crops(None, None, cr.affine_jobs(box, S, angle=a), (S, S))
        y, x = c.source_yx(0, 7.5, 7.5)
        assert abs(y - 17.5) < 1e-4 and abs(x - 27.5) < 1e-4
        y, x = c.source_yx(0, 8.5, 7.5)                                     # one step along the rows axis: along (cos, sin), 23 / 16 long
        assert abs(y - 17.5 - 23 / 16 * math.cos(a)) < 1e-3 and abs(x - 27.5 - 23 / 16 * math.sin(a)) < 1e-3
    # flips mirror the patch exactly, under a ragged scale and an angle
    for kw in (dict(), dict(angle=0.7, side=21.5), dict(window="box", margin=3)):
        size = (12, 9) if kw.get("window") == "box" else 12
        p0, m0 = cr.crops_host(lab, cr.affine_jobs(box, size, **kw), img, size)
        for flip, sl in (("h", np.s_[..., ::-1]), ("v", np.s_[..., ::-1, :]), ("hv", np.s_[..., ::-1, ::-1])):
            p1, m1 = cr.crops_host(lab, cr.affine_jobs(box, size, flip=flip, **kw), img, size)
            assert np.array_equal(p1, p0[sl]) and np.array_equal(m1, m0[sl]) and m0.any()
    # an empty box: img = -1, hence fill and an empty mask
    t = cr.affine_jobs(np.array([[0, 1, 0, 0, 0, 0], [0, 2, 3, 3, 3, 9], [0, 3, 2, 2, 9, 9]]), 8, angle=[0.1, float("nan"), 0.2])
    assert t[:, 0].tolist() == [-1, -1, 0]
    p, m = cr.crops_host(lab, t, img, 8, fill=9)
    assert (p[:2] == 9).all() and not m[:2].any() and (p[2] != 9).any()
    with pytest.raises(_lib.KGLibraryError):
        cr.affine_jobs(np.array([[0, 1, 0, 0, 30000, 30000]]), 1, angle=0.0, side=131072.0, flip="hv")     # a coefficient leaves int32


def host_instances(lab):
    """an Instances over a host label map, with the table of its ids 1 .. max"""
    n = int(lab.max())
    table = np.zeros((n, 8), np.int64)
    for v in range(1, n + 1):
        ys, xs = np.nonzero(lab == v)
        if len(ys):
            table[v - 1] = [len(ys), len(ys), ys.min(), xs.min(), ys.max() + 1, xs.max() + 1, ys.sum(), xs.sum()]
    return instances.Instances(torch.from_numpy(lab), np.zeros((n, 5), np.float32), table, None)


def test_major_axis_of_an_elongated_rectangle_and_an_empty_instance():
    H, W, S = 48, 64, 32
    lab = np.zeros((H, W), np.int32)
    lab[20:26, 10:50] = 1                                                   # 6 x 40, elongated along x: orientation pi / 2
    lab[5:45, 55:60] = 3                                                    # 40 x 5, along y: orientation 0; id 2 holds no pixel
    img = seeded_image((H, W), 1, np.uint16, 2)
    inst = host_instances(lab)
    got = cr.crops_instances(inst, img, S, angle="major", fill=11)
    assert isinstance(got, cr.Crops) and len(got) == 3 and got.size == (S, S) and got.jobs[:, 0].tolist() == [0, -1, 0] and inst.crops is None
    m = got.masks.numpy()
    for k in (0, 2):                                                        # the long side lies along the patch's rows axis: taller than wide
        rows, cols = np.nonzero(m[k].any(1))[0], np.nonzero(m[k].any(0))[0]
        assert rows.max() - rows.min() > 3 * (cols.max() - cols.min()) and m[k].sum() > 30
    assert not m[1].any() and (got.patches[1].numpy().view(np.uint16) == 11).all()
    assert got.patches.dtype == torch.int16 and got.patches.shape == (3, 1, S, S)
    # the same through measurements that are already there, and against the table built by hand
    from kg_instance_segmentation_amd import measure as ms
    inst.measurements = ms.measure_instances(inst)
    again = cr.crops_instances(inst, img, S, angle="major", fill=11)
    theta = np.nan_to_num(inst.measurements.props()["orientation"])
    assert abs(theta[0] - math.pi / 2) < 1e-12 and theta[2] == 0
    want = cr.affine_jobs(ms.jobs_from_stats(inst.table[:, 1:6]), S, angle=theta)
    assert np.array_equal(again.jobs, want) and np.array_equal(got.jobs, want) and torch.equal(again.patches, got.patches)
    p, k = cr.crops_host(lab, want, img, S, fill=11)
    assert np.array_equal(got.patches.numpy().view(np.uint16), p) and np.array_equal(m, k)
    # to_float reads uint16 storage unsigned; mean and std per channel
    f = got.to_float()
    assert f.dtype == torch.float32 and np.array_equal(f.numpy(), p.astype(np.float32)) and p.max() > 40000
    g = got.to_float(mean=[100.0], std=2.0)
    assert np.array_equal(g.numpy(), (p.astype(np.float32) - 100) / 2)
    masks_only = cr.crops_instances(inst, None, (8, 12), window="box")
    assert masks_only.patches is None and masks_only.masks.shape == (3, 8, 12) and masks_only.masks[0].all()
    with pytest.raises(_lib.KGLibraryError):
        masks_only.to_float()


def test_source_yx_maps_a_patch_pixel_back():
    box = np.array([[0, 1, 10, 20, 47, 57]])
    c = cr.Crops(None, None, cr.affine_jobs(box, 16), (16, 16))
    y, x = c.source_yx(0, np.arange(16), 0)
    assert np.allclose(y, 10 + (np.arange(16) + 0.5) * 37 / 16 - 0.5, atol=1e-3) and np.allclose(x, 20 + 0.5 * 37 / 16 - 0.5, atol=1e-4)


# ---- the option, the slot and the C entry -------------------------------------------------------------------------------------------------

def test_crops_keyword_defaults_to_none():
    for fn in (inference.predict_instances, tiling.predict_tiled):
        assert inspect.signature(fn).parameters["crops"].default is None
    a = instances.Instances(None, np.zeros((0, 5), np.float32), None, None)
    b = tiling.TiledInstances(None, np.zeros((0, 5), np.float32), None, None, None, None)
    assert a.crops is None and b.crops is None and "crops" in instances.Instances.__slots__ and not hasattr(a, "__dict__")


@pytest.fixture(scope="module")
def lib():
    from kg_instance_segmentation_amd import build
    build.build()
    return _lib.load()


def test_entry_is_declared_bound_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "kgnet_hip.h")).read()
    m = re.search(r"\bint\s+kg_label_crops\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m and len(m.group(1).split(",")) == 16
    assert "kg_label_crops" in _lib.SYMBOLS and hasattr(lib, "kg_label_crops") and len(_lib._SIGS["kg_label_crops"]) == 16


def test_entry_refuses_bad_arguments_before_any_launch(lib):
    """every host check of kg_label_crops, on host memory: the entry may never get as far as a launch"""
    name = "kg_label_crops"
    buf = (ctypes.c_longlong * 8192)()
    p = ctypes.addressof(buf)
    LAB, IMG, JOBS, PAT, MSK = (ctypes.c_void_p(p + k * 8192) for k in range(5))

    def call(labels=LAB, nimg=1, H=8, W=8, image=IMG, channels=3, elem=1, jobs=JOBS, m=3, OH=4, OW=4, flags=0, fill=0, patches=PAT, masks=MSK):
        return lib.kg_label_crops(labels, nimg, H, W, image, channels, elem, jobs, m, OH, OW, flags, fill, patches, masks, None)

    def err(rc, text):
        msg = lib.kg_last_error().decode()
        assert rc != 0 and name in msg and text in msg, (rc, msg)

    err(call(labels=None), "null pointer")
    err(call(jobs=None), "null pointer")
    err(call(image=None), "null pointer")                                   # patches without an image
    err(call(patches=None, masks=None), "at least one output")
    err(call(image=None, patches=None, masks=None), "at least one output")
    for v in (0, 5, -1):
        err(call(channels=v), f"channels {v}")
    for v in (3, 0):
        err(call(elem=v), f"elem_bytes {v}")
    for oh, ow in ((0, 4), (4, 0), (257, 4), (4, 257), (-1, 4)):
        err(call(OH=oh, OW=ow), "output size")
    for v in (4, -1, 8):
        err(call(flags=v), f"flags {v}")
    for v in (-1, 65536):
        err(call(fill=v), f"fill {v}")
    err(call(fill=256), "does not fit")
    err(call(H=32769), "32768")
    err(call(W=32769), "32768")
    err(call(nimg=0), "bad size")
    err(call(H=0), "bad size")
    err(call(m=-1), "bad size")
    err(call(nimg=3, H=32768, W=32768), "exceeds 2^31 - 1")
    err(call(m=2 ** 31 - 1, OH=1, OW=2, channels=1, patches=None, image=None), "exceeds 2^31 - 1")
    err(call(m=10923, OH=256, OW=256, channels=3), "exceeds 2^31 - 1")      # 10923 * 3 * 65536 = 2^31 + 65536
    err(call(labels=ctypes.c_void_p(p + 2)), "misaligned")
    err(call(jobs=ctypes.c_void_p(p + 2 * 8192 + 1)), "misaligned")
    err(call(image=ctypes.c_void_p(p + 8193), elem=2), "misaligned")
    err(call(patches=ctypes.c_void_p(p + 3 * 8192 + 1), elem=2), "misaligned")
    err(call(patches=LAB), "overlaps")
    err(call(patches=ctypes.c_void_p(p + 8192 + 100)), "overlaps")          # inside the image
    err(call(patches=ctypes.c_void_p(p + 2 * 8192 + 40)), "overlaps")       # inside the jobs
    err(call(masks=ctypes.c_void_p(p + 255)), "overlaps")                   # the last byte of the map
    err(call(masks=ctypes.c_void_p(p + 8192 + 191)), "overlaps")            # the last byte of the image
    err(call(masks=ctypes.c_void_p(p + 2 * 8192 + 119)), "overlaps")
    err(call(masks=ctypes.c_void_p(p + 3 * 8192 + 143)), "overlaps")        # the last byte of the patches
    assert call(m=0) == 0 and call(m=0, jobs=None, patches=None, masks=None) == 0 and call(m=0, image=None, patches=None) == 0
    assert call(m=0, fill=255) == 0 and call(m=0, fill=65535, elem=2) == 0 and call(m=0, fill=65535, image=None, patches=None) == 0
    assert call(m=0, flags=3, OH=256, OW=1) == 0 and call(m=0, patches=ctypes.c_void_p(p + 3 * 8192 + 1)) == 0   # a byte patch needs no alignment
