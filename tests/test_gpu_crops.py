"""GPU: instance crops (csrc/crops.hip, crops.py) against the host statement of the same semantics (crops.crops_host).  Every comparison
is exact equality.  Shapes are the smallest at which the kernel can go wrong: one-pixel, one-row and one-column maps, output sizes on
both sides of the 1024-position chunk and of the 4-position store, plane offsets that are not 4-byte aligned (odd OH * OW with 3
channels, and outputs that start inside a guarded buffer), every channel count under both element sizes, windows outside the map and
over every side and corner, hostile job tables between guard rows and guard bytes, several images in one launch and more work items
than the grid cap."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from kg_instance_segmentation_amd import KGnet, _lib, inference, instances, tiling  # noqa: E402
from kg_instance_segmentation_amd import components as cc  # noqa: E402
from kg_instance_segmentation_amd import crops as cr  # noqa: E402
from kg_instance_segmentation_amd import distance as dt  # noqa: E402
from kg_instance_segmentation_amd import split as sp  # noqa: E402
from kg_instance_segmentation_amd._lib import ptr, stream_ptr  # noqa: E402

DEV = "cuda"
I32 = np.iinfo(np.int32)
ONE = 65536


def up(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(DEV)


def down(t):
    """a device tensor -> the host array, int16 storage read as uint16"""
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


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


def job(img=0, v=1, oy=0, ox=0, ay=ONE, by=0, cy=0, ax=0, bx=ONE, cx=0):
    return [img, v, oy, ox, ay, by, cy, ax, bx, cx]


def ragged_jobs(nimg, H, W, ids, rng, k, scale=3):
    """k jobs with ragged scales, shears, negative coefficients and origins on every side of the map"""
    j = np.zeros((k, 10), np.int64)
    j[:, 0] = rng.integers(0, nimg, k)
    j[:, 1] = rng.choice(ids, k)
    j[:, 2] = rng.integers(-6, H + 3, k); j[:, 3] = rng.integers(-6, W + 3, k)
    j[:, [4, 8]] = rng.integers(-scale * ONE, scale * ONE, (k, 2))
    j[:, [5, 7]] = rng.integers(-ONE, ONE, (k, 2))
    j[:, [6, 9]] = rng.integers(-2 * ONE, 2 * ONE, (k, 2))
    return j


def check(lab, jobs, img, size, mode="linear", masked=False, fill=0, masks=True):
    """crop_rows on the device == crops_host; returns the host pair"""
    wp, wm = cr.crops_host(lab, jobs, img, size, mode, masked, fill, masks)
    gp, gm = cr.crop_rows(up(lab), np.asarray(jobs, np.int64).reshape(-1, 10), img, size, mode, masked, fill, masks)
    assert (gp is None) == (wp is None) and (gm is None) == (wm is None)
    if wp is not None:
        assert tuple(gp.shape) == wp.shape and gp.dtype == (torch.uint8 if wp.dtype == np.uint8 else torch.int16) and np.array_equal(down(gp), wp)
    if wm is not None:
        assert tuple(gm.shape) == wm.shape and gm.dtype == torch.uint8 and np.array_equal(down(gm), wm)
    return wp, wm


def guarded(lab, jobs, img, size, flags=0, fill=0, lead=1):
    """kg_label_crops over raw jobs, its outputs inside guarded buffers -- `lead` guard rows before (so that an odd row size misaligns every
    plane) and one after -- == crops_host; the guards are untouched.  Returns the host pair."""
    OH, OW = size
    lab3 = lab.reshape((-1,) + lab.shape[-2:])
    img4 = img.reshape(lab3.shape + (img.shape[-1],))
    j = np.asarray(jobs, np.int64).reshape(-1, 10)
    m, C = len(j), img4.shape[3]
    wp, wm = cr.crops_host(lab3, j, img4, size, cr.MODES[flags & 1], bool(flags & 2), fill)
    g8, gp = 0xA5, (0xA5 if img4.dtype == np.uint8 else 0x5AA5)
    pat = torch.full((m + lead + 1, C, OH, OW), gp if gp < 32768 else gp - 65536, dtype=torch.uint8 if img4.dtype == np.uint8 else torch.int16, device=DEV)
    msk = torch.full((m + lead + 1, OH, OW), g8, dtype=torch.uint8, device=DEV)
    d, di, dj = up(lab3), up(img4), up(j.astype(np.int32))
    _lib.call("kg_label_crops", ptr(d), lab3.shape[0], lab3.shape[1], lab3.shape[2], ptr(di), C, img4.dtype.itemsize, ptr(dj), m, OH, OW, flags, fill,
              ptr(pat[lead:]), ptr(msk[lead:]), stream_ptr())
    p, k = down(pat), down(msk)
    assert np.array_equal(p[lead:-1], wp) and (p[:lead] == gp).all() and (p[-1] == gp).all()
    assert np.array_equal(k[lead:-1], wm) and (k[:lead] == g8).all() and (k[-1] == g8).all()
    return wp, wm


@pytest.mark.parametrize("H,W", [(1, 1), (1, 130), (130, 1)])
def test_smallest_maps(H, W):
    lab = np.ones((1, 1), np.int32) if H * W == 1 else blob_map(H, W, 6, 10 + H)
    rng = np.random.default_rng(H + 2 * W)
    ids = np.unique(lab)
    for dtype in (np.uint8, np.uint16):
        img = seeded_image((H, W), 2, dtype, 1)
        jobs = np.concatenate([ragged_jobs(1, H, W, ids, rng, 12, scale=1 if H * W == 1 else 3), [job(v=int(lab[0, 0])), job(v=int(lab[0, 0]), oy=-2, ox=-2)]])
        for mode in cr.MODES:
            p, m = check(lab, jobs, img, (5, 6), mode, fill=7)
            assert m.any() and (p != 7).any() and (p == 7).any()


@pytest.mark.parametrize("size", [(1, 1), (1, 256), (256, 1), (3, 3), (4, 4), (5, 7), (33, 33), (255, 255), (256, 256)])
def test_output_sizes(size):
    """both sides of the 4-position store and of the 1024-position chunk (33 x 33: a partial last chunk; 255 x 255: an odd plane under 3
    channels, so every second plane is misaligned; 256 x 256: 64 full chunks)"""
    H, W = 45, 61
    lab = blob_map(H, W, 6, 3)
    rng = np.random.default_rng(size[0] * 7 + size[1])
    OH, OW = size
    v = 5
    lab[8:38, 10:52][lab[8:38, 10:52] == 0] = v                         # the middle of the map is id 5 with the other blobs as holes
    # windows a little larger than the map, ragged steps, a little shear; the last one mirrored
    jobs = np.array([job(v=v, oy=-5, ox=-4, ay=(H + 9) * ONE // OH + 1, bx=(W + 9) * ONE // OW + 3, by=int(rng.integers(1, ONE)) // (4 * OW),
                         ax=-int(rng.integers(1, ONE)) // (4 * OH), cy=int(rng.integers(0, ONE)), cx=int(rng.integers(0, ONE))),
                     job(v=v, oy=3, ox=7, ay=(H - 9) * ONE // OH + 5, bx=(W - 9) * ONE // OW + 7, cy=-12345, cx=54321),
                     job(v=v, oy=H, ox=W, ay=-((H + 3) * ONE // OH) - 1, bx=-((W + 3) * ONE // OW) - 1, cy=777, cx=-777)], np.int64)
    for dtype, C in ((np.uint8, 3), (np.uint16, 3), (np.uint8, 1)):
        img = seeded_image((H, W), C, dtype, 5)
        p, m = guarded(lab, jobs, img, size, fill=3, lead=1)
        assert (m.any() and not m.all() and (p != 3).any()) or min(size) < 3
    guarded(lab, jobs, img, size, flags=cr.NEAREST | cr.MASKED, fill=3, lead=2)


@pytest.mark.parametrize("OW", [1, 3, 4, 5])
def test_misaligned_planes_with_three_channels(OW):
    """OH * OW odd with C = 3: the planes of a job start at every residue of 4 bytes, so the packed and the element stores both run"""
    H, W = 30, 41
    lab = blob_map(H, W, 5, 4)
    rng = np.random.default_rng(OW)
    for OH in (1, 3, 7, 8):
        jobs = ragged_jobs(1, H, W, np.arange(6), rng, 9, scale=2)
        for dtype in (np.uint8, np.uint16):
            img = seeded_image((H, W), 3, dtype, OW)
            for lead in (1, 2):
                guarded(lab, jobs, img, (OH, OW), fill=9, lead=lead)


def test_channels_and_element_sizes_with_an_odd_width():
    H, W = 37, 53                                                       # an odd width: pixels of 1 .. 8 bytes at odd offsets
    lab = blob_map(H, W, 8, 2)
    rng = np.random.default_rng(1)
    jobs = ragged_jobs(1, H, W, np.arange(9), rng, 10)
    for dtype in (np.uint8, np.uint16):
        for C in (1, 2, 3, 4):
            img = seeded_image((H, W), C, dtype, 10 * C)
            for mode in cr.MODES:
                p, m = check(lab, jobs, img, (9, 11), mode, fill=1)
                assert p.shape == (10, C, 9, 11) and m.any()


def test_no_image_no_masks_modes_masked_and_fills():
    H, W = 40, 47
    lab = blob_map(H, W, 6, 5)
    rng = np.random.default_rng(2)
    jobs = ragged_jobs(1, H, W, np.arange(7), rng, 12, scale=2)
    none, m = check(lab, jobs, None, (13, 6))
    assert none is None and m.any()
    for dtype, fills in ((np.uint8, (0, 7, 255)), (np.uint16, (0, 7, 65535))):
        img = seeded_image((H, W), 3, dtype, 6)
        p, none = check(lab, jobs, img, (13, 6), masks=False)
        assert none is None and np.array_equal(p, cr.crops_host(lab, jobs, img, (13, 6))[0])
        for fill in fills:
            for mode in cr.MODES:
                for masked in (False, True):
                    p, k = check(lab, jobs, img, (13, 6), mode, masked, fill)
                    assert not masked or (p[np.broadcast_to(k[:, None] == 0, p.shape)] == fill).all()
                pm, none = check(lab, jobs, img, (13, 6), mode, True, fill, masks=False)    # masked without the masks output
                assert np.array_equal(pm, p)
    with pytest.raises(_lib.KGLibraryError):
        cr.crop_rows(up(lab), jobs, None, 4, masks=False)
    with pytest.raises(_lib.KGLibraryError):
        cr.crop_rows(up(lab), jobs, seeded_image((H, W), 1, np.uint8, 1), 4, fill=256)
    assert cr.crop_rows(up(lab), np.zeros((0, 10), np.int64), img, 4)[0].shape == (0, 3, 4, 4)     # m == 0 launches nothing


def test_scales_flips_quarter_turn_and_angles():
    H, W = 90, 2048
    lab = blob_map(H, W, 9, 6)
    lab[20:57, 100:137][lab[20:57, 100:137] == 0] = 4
    for dtype in (np.uint8, np.uint16):
        img = seeded_image((H, W), 2, dtype, 7)
        box = np.array([[0, 4, 20, 100, 52, 132]])
        p, m = check(lab, cr.affine_jobs(box, 32), img, 32)                                    # identity: the slice itself
        assert np.array_equal(p[0], np.moveaxis(img[20:52, 100:132], 2, 0)) and np.array_equal(m[0], lab[20:52, 100:132] == 4) and m.any()
        p, _ = check(lab, cr.affine_jobs(box, 16), img, 16)                                    # 2x down: 2 x 2 means, rounded half up
        blk = img[20:52, 100:132].astype(np.int64).reshape(16, 2, 16, 2, 2).sum((1, 3))
        assert np.array_equal(p[0], np.moveaxis((blk + 2) >> 2, 2, 0))
        check(lab, cr.affine_jobs(box, 64), img, 64)                                           # 2x up
        ragged = np.array([[0, 4, 20, 100, 57, 137]])
        t = cr.affine_jobs(ragged, 16)
        assert t[0, 4] == 151552 and t[0, 6] == 43008
        check(lab, t, img, 16)                                                                  # 37 -> 16
        wide = cr.affine_jobs(np.array([[0, 2, 10, 24, 60, 2024]]), 8, window="box")            # a 2000-pixel window -> 8
        assert wide[0, 8] == 250 * ONE
        check(lab, wide, img, 8)
        check(lab, cr.affine_jobs(np.array([[0, 2, 0, 24, 90, 2024]]), 8), img, 8)              # the square of it: mostly outside
        for flip in ("h", "v", "hv"):
            for kw in (dict(), dict(angle=0.7, side=41.5)):
                check(lab, cr.affine_jobs(ragged, 24, flip=flip, **kw), img, 24)
        up_, um = cr.crops_host(lab, cr.affine_jobs(box, 32), img, 32)
        q = cr.affine_jobs(box, 32, angle=math.pi / 2, side=32)
        assert [q[0, 4], q[0, 5], q[0, 7], q[0, 8]] == [0, -ONE, ONE, 0]
        rp, rm = check(lab, q, img, 32)                                                         # the exact quarter turn
        assert np.array_equal(rp[0], np.rot90(up_[0], k=-1, axes=(1, 2))) and np.array_equal(rm[0], np.rot90(um[0], k=-1))
        boxes = np.array([[0, v, 5 + 3 * v, 40 * v, 30 + 5 * v, 40 * v + 60 - 4 * v] for v in range(1, 10)])
        angles = np.linspace(-3.0, 3.0, 9)
        for mode in cr.MODES:
            check(lab, cr.affine_jobs(boxes, 20, angle=angles, margin=2), img, 20, mode, masked=True, fill=5)


def test_windows_outside_and_over_every_side_and_corner():
    H, W, S = 14, 17, 8
    lab = np.full((H, W), 4, np.int32)
    spots = [(-2 * S, 3), (H + 1, 3), (3, -S - 1), (3, W), (-3, 4), (H - 3, 4), (4, -3), (4, W - 3), (-3, -3), (-3, W - 4), (H - 4, -3), (H - 4, W - 4),
             (-S, -S), (H, W)]
    for dtype in (np.uint8, np.uint16):
        img = seeded_image((H, W), 2, dtype, 6)
        jobs = [job(v=4, oy=y, ox=x, cy=c, cx=c) for y, x in spots for c in (0, ONE // 2, -ONE // 3)]
        for mode in cr.MODES:
            p, m = guarded(lab, jobs, img, (S, S), flags=mode == "nearest", fill=7)
            assert (p[0] == 7).all() and not m[0].any() and (p[3 * 12] == 7).all() and m[3 * 4].any() and not m[3 * 4].all()


def test_top_of_the_type_with_ragged_fractions():
    H, W = 33, 35
    lab = blob_map(H, W, 4, 1)
    full = np.full((H, W, 3), 65535, np.uint16)
    rng = np.random.default_rng(5)
    jobs = [job(oy=10, ox=12, ay=int(a), bx=int(b), cy=int(c), cx=int(d), by=int(e), ax=int(f)) for a, b, c, d, e, f in rng.integers(-40000, 40000, (40, 6))]
    p, _ = check(lab, jobs, full, (9, 9), fill=65535)
    assert (p == 65535).all()
    p, _ = check(lab, jobs, np.full((H, W, 3), 255, np.uint8), (9, 9), fill=255)
    assert (p == 255).all()


def test_ids():
    H, W = 33, 70
    lab = blob_map(H, W, 9, 5)
    lab[3:6, 10:60] = -1
    lab[8:11, 5:50] = I32.min
    lab[20:25, 30:69] = I32.max
    img = seeded_image((H, W), 3, np.uint8, 3)
    jobs = cr.affine_jobs(np.array([[0, v, 0, 0, H, W] for v in (0, -1, I32.min, I32.max, 3, 77)], np.int64), (33, 70), window="box")
    p, m = check(lab, jobs, img, (33, 70), masked=True, fill=1)
    assert all(np.array_equal(m[k], lab == v) for k, v in enumerate((0, -1, I32.min, I32.max, 3))) and not m[5].any() and (p[5] == 1).all()
    assert m[1].sum() == 150 and m[2].sum() == 135 and m[3].sum() == 195


def test_hostile_jobs_between_guard_rows():
    """Every table is in range by construction of the predicates: a bad image index gives fill, extreme coefficients and origins give
    fill wherever the int64 position leaves the map.  The rows before and after each hostile row are correct, the guards untouched."""
    H, W, nimg = 33, 47, 2
    lab = np.stack([blob_map(H, W, 9, 5), blob_map(H, W, 9, 6)])
    lab[1, 5:20, 8:30:2] = 5                                                                       # the base job's window holds its id
    rng = np.random.default_rng(3)
    good = ragged_jobs(nimg, H, W, np.arange(10), rng, 8, scale=2).tolist() + [job(v=3, oy=2, ox=3), job(img=1, v=5, oy=-3, ox=40)]
    base = job(img=1, v=5, oy=4, ox=6)

    def with_(cols, v):
        r = list(base)
        for c in np.atleast_1d(cols):
            r[c] = v
        return r
    bad = ([with_(0, v) for v in (nimg, -1, I32.max, I32.min)]                                     # no such image
           + [with_(c, v) for c in range(2, 10) for v in (I32.min, I32.max)]                       # one extreme origin or coefficient
           + [with_([2, 3], v) for v in (I32.min, I32.max)] + [with_([4, 5, 6], v) for v in (I32.min, I32.max)]
           + [with_([7, 8, 9], v) for v in (I32.min, I32.max)] + [with_(range(2, 10), v) for v in (I32.min, I32.max)]
           + [[I32.min] * 10, [I32.max] * 10, with_([4, 8], -1), with_([4, 8], 0),
              job(img=1, v=5, oy=I32.max, ox=I32.max, ay=I32.min, bx=I32.min), job(img=1, v=5, oy=I32.min, ox=I32.min, ay=I32.max, bx=I32.max)])
    jobs = [r for k, b in enumerate(bad) for r in (good[k % len(good)], b)] + [base] * 40
    nb = len(bad)
    for dtype, C, size in ((np.uint8, 3, (5, 7)), (np.uint16, 2, (33, 33)), (np.uint8, 4, (3, 3))):
        img = seeded_image((nimg, H, W), C, dtype, 3)
        for flags in (0, cr.NEAREST, cr.MASKED, cr.NEAREST | cr.MASKED):
            p, m = guarded(lab, jobs, img, size, flags=flags, fill=7)
            assert (p[1:8:2] == 7).all() and not m[1:8:2].any()                                    # the bad image indices
            assert (p[2 * nb:] == p[2 * nb]).all() and m[2 * nb].any() and not m[2 * nb].all()
            assert flags & cr.MASKED or (p[0:2 * nb:2] != 7).any((1, 2, 3)).sum() > nb // 2      # the rows between the hostile ones hold pixels


def test_three_images_interleaved():
    H, W = 40, 67
    lab = np.stack([blob_map(H, W, 7, 1), np.zeros((H, W), np.int32), blob_map(H, W, 12, 2)])
    img = seeded_image((3, H, W), 3, np.uint16, 4)
    rng = np.random.default_rng(0)
    jobs = ragged_jobs(3, H, W, np.arange(13), rng, 30, scale=2)
    p, m = check(lab, jobs, img, (12, 10))
    assert len(set(jobs[:6, 0].tolist())) >= 2 and m.any()
    gp, gm = cr.crop_rows(up(lab), up(jobs.astype(np.int32)), up(img), (12, 10))                 # device jobs, a device image
    assert np.array_equal(down(gp), p) and np.array_equal(down(gm), m)
    # crops(): the ids 1 .. n of every map inside their own boxes, stats measured on the device
    got = cr.crops(up(lab), [7, 0, 12], image=img, size=16, margin=1, masked=True, fill=2)
    assert isinstance(got, cr.Crops) and len(got) == 19 and got.size == (16, 16) and got.jobs.shape == (19, 10)
    wp, wm = cr.crops_host(lab, got.jobs, img, 16, masked=True, fill=2)
    assert np.array_equal(down(got.patches), wp) and np.array_equal(down(got.masks), wm) and wm[got.jobs[:, 0] >= 0].any((1, 2)).all()
    f = got.to_float(mean=[1.0, 2.0, 3.0], std=[2.0, 4.0, 8.0])
    assert f.dtype == torch.float32 and f.device.type == DEV
    assert np.array_equal(f.cpu().numpy(), (wp.astype(np.float32) - np.float32([1, 2, 3])[None, :, None, None]) / np.float32([2, 4, 8])[None, :, None, None])


def test_grid_stride():
    """1 048 584 jobs at 1 x 1 with one channel: more work items than the grid cap of 2^20 blocks, and the blocks that wrap take a
    different job.  The host statement is vectorised over jobs."""
    H, W, m = 61, 67, 2 ** 20 + 8
    lab = blob_map(H, W, 9, 4)
    img = seeded_image((H, W), 1, np.uint8, 4)
    rng = np.random.default_rng(7)
    jobs = np.zeros((m, 10), np.int64)
    jobs[:, 1] = rng.integers(0, 10, m)
    jobs[:, 2] = rng.integers(-1, H + 1, m); jobs[:, 3] = rng.integers(-1, W + 1, m)
    jobs[:, 6] = rng.integers(0, ONE, m); jobs[:, 9] = rng.integers(0, ONE, m)
    jobs[:, [4, 8]] = ONE
    jobs[-8:, 2:4] = [[5, 6]] * 8
    jobs[-8:, 1] = lab[5, 6]
    jobs[-8:, [6, 9]] = 0
    wp, wm = cr.crops_host(lab, jobs, img, 1, fill=9)
    pat = torch.full((m + 2, 1, 1, 1), 0xA5, dtype=torch.uint8, device=DEV)
    msk = torch.full((m + 2, 1, 1), 0xA5, dtype=torch.uint8, device=DEV)
    d, di, dj = up(lab[None]), up(img[None]), up(jobs.astype(np.int32))
    _lib.call("kg_label_crops", ptr(d), 1, H, W, ptr(di), 1, 1, ptr(dj), m, 1, 1, 0, 9, ptr(pat[1:]), ptr(msk[1:]), stream_ptr())
    p, k = down(pat), down(msk)
    assert np.array_equal(p[1:-1], wp) and np.array_equal(k[1:-1], wm) and p[0] == 0xA5 and p[-1] == 0xA5 and k[0] == 0xA5 and k[-1] == 0xA5
    assert (wp[-8:] == img[5, 6, 0]).all() and wm[-8:].all() and 0.05 < wm.mean() < 0.95 and len(np.unique(wp)) > 200


def test_entry_refuses_bad_arguments_before_any_launch():
    import ctypes
    lib = _lib.load()
    name = "kg_label_crops"
    lab = torch.zeros((8, 8), dtype=torch.int32, device=DEV)
    img = torch.zeros((8, 8, 3), dtype=torch.int16, device=DEV)
    jobs = torch.zeros((3, 10), dtype=torch.int32, device=DEV)
    pat = torch.full((3, 3, 4, 4), -7, dtype=torch.int16, device=DEV)
    msk = torch.full((3, 4, 4), 0xA5, dtype=torch.uint8, device=DEV)
    LAB, IMG, JOBS, PAT, MSK = (ctypes.c_void_p(t.data_ptr()) for t in (lab, img, jobs, pat, msk))

    def off(t, k):
        return ctypes.c_void_p(t.data_ptr() + k)

    def call(labels=LAB, nimg=1, H=8, W=8, image=IMG, channels=3, elem=2, jobs=JOBS, m=3, OH=4, OW=4, flags=0, fill=0, patches=PAT, masks=MSK):
        return lib.kg_label_crops(labels, nimg, H, W, image, channels, elem, jobs, m, OH, OW, flags, fill, patches, masks, stream_ptr())

    def err(rc, text):
        msg = lib.kg_last_error().decode()
        assert rc != 0 and name in msg and text in msg, (rc, msg)

    err(call(labels=None), "null pointer")
    err(call(jobs=None), "null pointer")
    err(call(image=None), "null pointer")
    err(call(patches=None, masks=None), "at least one output")
    err(call(channels=0), "channels 0")
    err(call(channels=5), "channels 5")
    err(call(elem=3), "elem_bytes 3")
    err(call(OH=0), "output size")
    err(call(OW=257), "output size")
    err(call(flags=4), "flags 4")
    err(call(fill=-1), "fill -1")
    err(call(fill=65536), "fill 65536")
    err(call(fill=256, elem=1), "does not fit")
    err(call(H=32769), "32768")
    err(call(nimg=0), "bad size")
    err(call(m=-1), "bad size")
    err(call(nimg=3, H=32768, W=32768), "exceeds 2^31 - 1")
    err(call(m=10923, OH=256, OW=256), "exceeds 2^31 - 1")
    err(call(labels=off(lab, 2)), "misaligned")
    err(call(jobs=off(jobs, 1)), "misaligned")
    err(call(image=off(img, 1)), "misaligned")
    err(call(patches=off(pat, 1)), "misaligned")
    err(call(patches=LAB), "overlaps")
    err(call(patches=off(img, 100)), "overlaps")
    err(call(masks=off(jobs, 40)), "overlaps")
    err(call(masks=off(pat, 280)), "overlaps")
    assert call(m=0) == 0 and call(m=0, jobs=None, patches=None, masks=None) == 0
    torch.cuda.synchronize()
    assert bool((pat == -7).all()) and bool((msk == 0xA5).all())        # nothing was launched by any refused call


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
    return all(getattr(a, k) is None for k in ("measurements", "neighbours", "runs", "contours", "hulls", "quantiles", "texture", "midlines"))


def host_crops(inst, image, **kw):
    """crops_instances down the host route (crops_host, measure_host) over the instance's label map copied back"""
    return cr.crops_instances(instances.Instances(inst.labels.cpu(), inst.dets, inst.table, None), image, **kw)


def same_crops(got, want):
    ok = isinstance(got, cr.Crops) and np.array_equal(got.jobs, want.jobs) and got.size == want.size and got.mode == want.mode and got.fill == want.fill
    for a, b in ((got.patches, want.patches), (got.masks, want.masks)):
        ok = ok and ((a is None and b is None) or (a.device.type == "cuda" and a.dtype == b.dtype and torch.equal(a.cpu(), b)))
    return ok


def test_predict_tiled_with_crops(cal_model):
    H, W, S = 400, 600, 256
    img = np.random.default_rng(8).integers(0, 256, (H, W, 3), dtype=np.uint8)
    plain = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4)
    none = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4, crops=None)
    got = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4, crops=True)
    n = len(plain)
    assert n > 0 and plain.crops is None and none.crops is None and same_instances(none, plain) and others_untouched(none)
    assert same_instances(got, plain) and others_untouched(got) and got.parent is None                 # the other fields are untouched
    assert tuple(got.crops.patches.shape) == (n, 3, 64, 64) and tuple(got.crops.masks.shape) == (n, 64, 64) and got.crops.patches.dtype == torch.uint8
    assert same_crops(got.crops, host_crops(plain, img)) and int(got.crops.masks.any(2).any(1).sum()) > n // 2
    # with clean=, split= and expand= as well: taken on the final map; a dict, a device image, the major axis, masked patches
    policy = dict(min_area=4)
    kw = {"size": 32, "angle": "major", "margin": 2, "masked": True, "fill": 3, "mode": "linear"}
    both = tiling.predict_tiled(cal_model, up(img), tile=S, overlap=64, batch=4, clean=policy, split=2, expand=2, crops=kw)
    final = dt.expand_instances(sp.split_instances(cc.clean_instances(plain, **policy), 2), 2)
    assert final.crops is None and same_instances(both, final) and both.measurements is None
    assert same_crops(both.crops, host_crops(final, img, **kw)) and both.crops.masks.any()
    # another image through the dict, anisotropic windows, nearest; and masks only
    wide = np.random.default_rng(9).integers(0, 65536, (H, W, 1)).astype(np.uint16)
    kw = {"size": (24, 40), "window": "box", "mode": "nearest", "flip": "h", "fill": 65535}
    other = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4, crops=dict(kw, image=wide))
    assert same_instances(other, plain) and same_crops(other.crops, host_crops(plain, wide, **kw)) and other.crops.patches.dtype == torch.int16
    only = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4, crops={"image": None, "size": 16})
    assert only.crops.patches is None and same_crops(only.crops, host_crops(plain, None, size=16))


def test_predict_instances_with_crops(cal_model):
    S = 256
    src = np.random.default_rng(9).integers(0, 256, (2, S, S, 3), dtype=np.uint8)
    x = torch.cat([tiling.cut_tiles(src[i], tiling.plan(S, S, S, 64)) for i in range(2)])
    plain = inference.predict_instances(cal_model, x)
    none = inference.predict_instances(cal_model, x, crops=None)
    assert all(p is not None and len(p) > 0 and p.crops is None for p in plain)
    assert all(same_instances(a, b) and a.crops is None and others_untouched(a) for a, b in zip(none, plain))
    inten = np.random.default_rng(10).integers(0, 65536, (2, S, S, 2)).astype(np.uint16)
    full = inference.predict_instances(cal_model, x, crops=inten)
    policy = dict(min_area=4)
    kw = {"size": 48, "angle": "major", "side": 40.0, "flip": "v"}
    opts = inference.predict_instances(cal_model, x, clean=policy, split=2, expand=1.5, crops=dict(kw, image=up(src)))
    meas = inference.predict_instances(cal_model, x, clean=policy, split=2, expand=1.5, measure=True, crops=dict(kw, image=src))
    final = dt.expand_instances_batch(sp.split_instances_batch(cc.clean_instances_batch(inference.predict_instances(cal_model, x), **policy), 2), 1.5)
    for i, (p, f, o, e, q) in enumerate(zip(plain, full, opts, final, meas)):
        assert same_instances(p, f) and same_instances(o, e) and same_instances(q, e) and others_untouched(f) and e.crops is None
        want = host_crops(p, inten[i])
        want.jobs[:, 0] = np.where(want.jobs[:, 0] >= 0, i, -1)                                   # in a batch img counts the images of one size
        assert same_crops(f.crops, want) and tuple(f.crops.patches.shape) == (len(p), 2, 64, 64) and f.crops.masks.any()
        want = host_crops(e, src[i], **kw)
        want.jobs[:, 0] = np.where(want.jobs[:, 0] >= 0, i, -1)
        assert same_crops(o.crops, want) and same_crops(q.crops, want) and q.measurements is not None and o.measurements is None
