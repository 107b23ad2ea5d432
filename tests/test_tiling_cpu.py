"""CPU: the semantics of tiled whole-image inference as tiling.py states them in NumPy -- the tile plan and its cores, ownership, duplicates
across tiles, the stitched label map and the table read back from it -- and the host-side argument validation of kg_tile_cut /
kg_bitmask_clip / kg_tile_stitch / kg_label_table.  Every comparison is exact."""
import ctypes
import os

import numpy as np
import pytest
import torch

from kg_instance_segmentation_amd import _lib, bitmasks, inference, instances, tiling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (1, 31, 64, 65, 97, 129, 160, 1388)
TILES = ((64, 32), (96, 32), (64, 0), (512, 128))


@pytest.mark.parametrize("t,overlap", TILES)
def test_plan_axis(t, overlap):
    for L in LENGTHS:
        og = tiling.plan_axis(L, t, overlap)
        assert og[0] == 0 and np.all(np.diff(og) > 0), (L, og)                      # strictly increasing
        cov = np.zeros(L, np.int64)
        for a in og:
            cov[a:a + t] += 1
        assert cov.min() >= 1                                                        # every pixel is covered
        if L <= t:
            assert og.tolist() == [0]
        else:
            assert len(og) == 1 + -(-(L - t) // (t - overlap))
            assert np.all(np.diff(og) <= t - overlap) and og[-1] + t == L            # the overlap holds; the last tile ends at L
        b = tiling.axis_bounds(og, t)
        lo, hi = np.concatenate([[-np.inf], b]), np.concatenate([b, [np.inf]])
        assert np.all(lo < hi) and np.array_equal(lo[1:], hi[:-1])                   # the cores partition the axis
        for k, a in enumerate(og):                                                   # each core, clipped to the image, lies in its tile
            assert a <= max(lo[k], 0) and min(hi[k], L) <= a + t


def test_plan_grid_and_validation():
    p = tiling.plan(150, 170, 64, 32)
    assert p.shape == (4, 5) and len(p) == 20 and p.origins.dtype == np.int32 and p.ys.dtype == np.int32
    assert p.origins[7].tolist() == [p.ys[1], p.xs[2]]
    assert p.cores[0, 0] == -np.inf and p.cores[-1, 1] == np.inf and p.cores[7].tolist() == [p.ybounds[0], p.ybounds[1], p.xbounds[1], p.xbounds[2]]
    q = tiling.plan(20, 50, (32, 64), 8)
    assert len(q) == 1 and q.valid(0) == (20, 50)
    d = tiling.plan(1040, 1388)
    assert (d.th, d.tw) == (512, 512) and d.shape == (3, 4)
    for kw in (dict(tile=48), dict(tile=(64, 40)), dict(tile=0), dict(overlap=64), dict(overlap=-1), dict(overlap=1.5), dict(H=0)):
        with pytest.raises(_lib.KGLibraryError):
            tiling.plan(**{**dict(H=100, W=100, tile=64, overlap=16), **kw})


def test_every_box_has_exactly_one_owner():
    p = tiling.plan(150, 170, 64, 32)
    rng = np.random.default_rng(3)
    cy = np.concatenate([rng.uniform(-40, 200, 500), p.ybounds.astype(np.float64), p.ybounds - 0.5, [-1e9, 1e9]])
    cx = np.concatenate([rng.uniform(-40, 220, 500), np.resize(p.xbounds.astype(np.float64), len(p.ybounds)), np.resize(p.xbounds - 0.5, len(p.ybounds)),
                         [1e9, -1e9]])
    own = tiling.owner(p, cy, cx)
    inside = (cy[:, None] >= p.cores[None, :, 0]) & (cy[:, None] < p.cores[None, :, 1]) & (cx[:, None] >= p.cores[None, :, 2]) & \
             (cx[:, None] < p.cores[None, :, 3])
    assert np.array_equal(inside.sum(1), np.ones(len(cy), np.int64)) and np.array_equal(inside.argmax(1), own)
    # the same through owner_keep: a box given to every tile in that tile's pixels is kept by exactly one
    for y1, x1, y2, x2 in [(40, 40, 52, 50), (float(p.ybounds[0]) - 3, float(p.xbounds[1]) - 4, float(p.ybounds[0]) + 3, float(p.xbounds[1]) + 4),
                           (-30, -30, -10, -10), (140, 160, 190, 230)]:
        kept = [t for t in range(len(p))
                if tiling.owner_keep(p, t, np.array([[y1 - p.origins[t, 0], x1 - p.origins[t, 1], y2 - p.origins[t, 0], x2 - p.origins[t, 1], 0.9]]))[0]]
        assert kept == [int(tiling.owner(p, (y1 + y2) / 2, (x1 + x2) / 2))], (y1, x1, kept)
    # a centre exactly on a boundary belongs to the later tile
    b = float(p.ybounds[0])
    assert tiling.owner(p, b, 0.0) == len(p.xs) and tiling.owner(p, np.nextafter(b, -np.inf), 0.0) == 0


def random_tile_boxes(p, n, rng, smax=30):
    tile = rng.integers(0, len(p), n)
    y1, x1 = rng.integers(0, p.th - 4, n), rng.integers(0, p.tw - 4, n)
    y2, x2 = np.minimum(y1 + rng.integers(2, smax, n), p.th - 1), np.minimum(x1 + rng.integers(2, smax, n), p.tw - 1)
    local = np.stack([y1, x1, y2, x2], 1)
    return tile, local, local + np.concatenate([p.origins[tile], p.origins[tile]], 1)


@pytest.mark.parametrize("thresh", [0.5, 0.1, 0.0])
def test_suppress_equals_the_plain_rule(thresh):
    p = tiling.plan(150, 170, 64, 32)
    rng = np.random.default_rng(11)
    tile, _, glob = random_tile_boxes(p, 400, rng)
    glob = np.concatenate([glob, glob[:40] + rng.integers(-2, 3, (40, 4))]).astype(np.float64)      # near-duplicates of the first 40 ...
    near = np.array([t - 1 if t % len(p.xs) == len(p.xs) - 1 else t + 1 for t in tile[:40]])            # ... in the neighbouring tile
    tile = np.concatenate([tile, near])
    order = rng.permutation(len(tile))
    glob, tile = glob[order], tile[order]
    want = tiling.suppress_across_tiles_plain(glob, tile, thresh)
    assert np.array_equal(tiling.suppress_across_tiles(glob, tile, thresh), want)
    assert 0 < (~want).sum() < len(want)
    inside = np.all((glob[:, :2] >= p.origins[tile]) & (glob[:, 2:] <= p.origins[tile] + [p.th, p.tw]), 1)      # the skip rule's premise
    touch = tiling.touches_other_tile(p, glob[inside], tile[inside])
    assert 0 < touch.sum() < inside.sum()
    assert np.array_equal(tiling.suppress_across_tiles(glob[inside], tile[inside], thresh, p),
                          tiling.suppress_across_tiles_plain(glob[inside], tile[inside], thresh))


def test_suppress_rules():
    a = [10., 10., 30., 30.]
    near = [10., 11., 30., 30.]                                                      # IoU 0.95 with a
    assert tiling.suppress_across_tiles([a, near], [3, 3]).tolist() == [True, True]  # one tile: what the per-tile NMS decided stands
    assert tiling.suppress_across_tiles([a, near], [3, 4]).tolist() == [True, False]
    assert tiling.suppress_across_tiles([a, near, near], [3, 3, 4]).tolist() == [True, True, False]
    assert tiling.suppress_across_tiles([a, [10., 10., 30., 70.]], [3, 4]).tolist() == [True, True]        # IoU 1/3
    assert tiling.suppress_across_tiles([a, a, [50., 50., 50., 50.]], [0, 1, 2], 0.5).tolist() == [True, False, True]      # a box of zero area overlaps nothing
    # a dropped detection drops nothing: b (tile 1) falls to a (tile 0); c (tile 2) overlaps b alone (IoU 1/3) and stays
    b, c = [10., 16., 30., 36.], [10., 26., 30., 46.]
    assert tiling.suppress_across_tiles([a, b, c], [0, 1, 2], 0.3).tolist() == [True, False, True]
    # through select: the same global box seen by two tiles whose cores meet at its centre
    p = tiling.plan(64, 96, 64, 32)
    assert p.xs.tolist() == [0, 32] and p.xbounds.tolist() == [48]
    box = np.array([20., 40., 30., 56.])                                             # centre x = 48: tile 1 owns it

    def dets(t, conf, b=box):
        return np.array([[b[0], b[1] - p.xs[t], b[2], b[3] - p.xs[t], conf]], np.float32)
    s = tiling.select(p, [dets(0, 0.9), dets(1, 0.8)])
    assert s.tile.tolist() == [1] and s.dets.tolist() == [[20., 40., 30., 56., np.float32(0.8)]]       # ownership: tile 0 never keeps it
    left = np.array([20., 36., 30., 58.])                                            # centre x = 47: tile 0; IoU with box 16 / 22
    s = tiling.select(p, [dets(0, 0.7, left), dets(1, 0.8)])
    assert s.tile.tolist() == [1]                                                    # the lower confidence goes
    s = tiling.select(p, [dets(0, 0.8, left), dets(1, 0.8)])
    assert s.tile.tolist() == [0] and s.row.tolist() == [0]                          # a tie: the later tile's goes
    s = tiling.select(p, [dets(0, 0.7, left), dets(1, 0.8)], nms_thresh=0.8)
    assert s.tile.tolist() == [1, 0] and s.origin.tolist() == [[0, 32], [0, 0]] and s.boxes.tolist() == [[20, 40, 30, 56], [20, 36, 30, 58]]


def seeded_instances(p, n, seed):
    """n seeded instances: per instance a tile, a tile-local mask uint8 [th, tw] inside a box, a confidence"""
    rng = np.random.default_rng(seed)
    tile, local, _ = random_tile_boxes(p, n, rng)
    masks = np.zeros((n, p.th, p.tw), np.uint8)
    for i, (y1, x1, y2, x2) in enumerate(local):
        masks[i, y1:y2, x1:x2] = rng.random((y2 - y1, x2 - x1)) < 0.8
    conf = rng.random(n).astype(np.float32)
    conf[n // 2] = conf[n // 3]                                                      # a tie
    return tile, local, masks, conf


def global_masks(p, tile, masks):
    out = np.zeros((len(masks), p.H, p.W), np.uint8)
    for i, t in enumerate(tile):
        y0, x0 = p.origins[t]
        vh, vw = p.valid(t)
        out[i, y0:y0 + vh, x0:x0 + vw] = masks[i, :vh, :vw]
    return out


@pytest.mark.parametrize("H,W,tile,overlap,n", [(150, 170, 64, 32, 60), (20, 50, (32, 64), 8, 12)])
def test_stitch_and_table_equal_the_global_masks(H, W, tile, overlap, n):
    p = tiling.plan(H, W, tile, overlap)
    assert len(p) == (20 if n == 60 else 1)
    tile_of, local, masks, conf = seeded_instances(p, n, 5)
    order = np.lexsort((np.arange(n), tile_of, -conf.astype(np.float64)))            # ids: position in (-conf, tile, row) order + 1
    tile_of, local, masks = tile_of[order], local[order], masks[order]
    tile_of[-1], local[-1], masks[-1] = tile_of[0], local[0], masks[0]               # the last instance lies under the first: hidden
    glob = global_masks(p, tile_of, masks)
    want = instances.label_map_host(glob)
    tl = np.zeros((len(p), p.th, p.tw), np.int32)
    for t in range(len(p)):
        k = np.flatnonzero(tile_of == t)
        vh, vw = p.valid(t)
        m = masks[k].copy()
        m[:, vh:] = 0
        m[:, :, vw:] = 0
        tl[t] = instances.label_map_host(m, ids=k + 1)
    got = tiling.stitch_host(tl, p)
    assert got.dtype == np.int32 and np.array_equal(got, want) and (want > 0).mean() > 0.2
    # table, columns 1-7, from det-box jobs
    org = np.concatenate([p.origins[tile_of], p.origins[tile_of]], 1)
    box = np.clip(local + org, 0, [H, W, H, W])
    jobs = np.concatenate([np.arange(1, n + 1)[:, None], box], 1)
    full = glob.reshape(n, -1).sum(1)
    tab = tiling.table_from_labels_host(got, jobs, full)
    assert tab.dtype == np.int64 and np.array_equal(tab, instances.table_host(glob))
    assert tab[-1, 0] == tab[0, 0] and not tab[-1, 1:].any()                         # the hidden instance: zeros
    assert np.array_equal(tiling.table_from_labels_host(got, jobs)[:, 1:], tab[:, 1:])
    for bad in ([[0, 0, 0, 1, 1]], [[1, 2, 0, 1, 1]], [[1, 0, 0, H + 1, 1]], [[1, 0, -1, 1, 1]], [[1, 0, 0, 1]]):
        with pytest.raises(_lib.KGLibraryError):
            tiling.table_from_labels_host(got, np.array(bad))


def test_assemble_host_equals_the_global_masks():
    """assemble_host over overlapping tiles: ownership and duplicate removal first, then the map and the table of what is left."""
    p = tiling.plan(150, 170, 64, 32)
    tile_of, local, masks, conf = seeded_instances(p, 80, 6)
    preds = [None] * len(p)
    for t in range(len(p)):
        k = np.flatnonzero(tile_of == t)
        k = k[np.argsort(-conf[k], kind="stable")]
        if len(k):
            preds[t] = [masks[k], np.concatenate([local[k].astype(np.float32), conf[k, None]], 1)]
    r = tiling.assemble_host(p, preds)
    n = len(r)
    assert 10 < n < 80 and len(np.unique(r.tile)) > 5
    assert np.all(np.diff(r.dets[:, 4]) <= 0) and np.array_equal(r.origin, p.origins[r.tile])
    cy, cx = (r.dets[:, 0] + r.dets[:, 2]) / 2, (r.dets[:, 1] + r.dets[:, 3]) / 2
    assert np.array_equal(tiling.owner(p, cy.astype(np.float64), cx.astype(np.float64)), r.tile)
    glob = global_masks(p, r.tile, r.tile_masks)
    assert np.array_equal(r.labels, instances.label_map_host(glob)) and np.array_equal(r.table, instances.table_host(glob))
    assert r.masks is None and r.centroids().shape == (n, 2)


def test_assemble_without_detections():
    p = tiling.plan(97, 101, (32, 64), 16)
    for r in (tiling.assemble_host(p, [None] * len(p)), tiling.assemble(p, [None] * len(p), device="cpu"),
              tiling.assemble_host(p, [[np.zeros((0, 32, 64), np.uint8), np.zeros((0, 5), np.float32)]] + [None] * (len(p) - 1))):
        lab = np.asarray(r.labels)
        assert lab.shape == (97, 101) and lab.dtype == np.int32 and not lab.any()
        assert len(r) == 0 and r.dets.shape == (0, 5) and r.dets.dtype == np.float32 and r.table.shape == (0, 8) and r.table.dtype == np.int64
        assert r.tile.shape == (0,) and r.origin.shape == (0, 2) and len(r.tile_masks) == 0 and r.masks is None
    with pytest.raises(_lib.KGLibraryError):
        tiling.assemble_host(p, [None])


def test_cut_tiles_host():
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (20, 50, 3), dtype=np.uint8)
    img[0, 0] = (0, 255, 1)
    p = tiling.plan(20, 50, (32, 64), 8)
    x = tiling.cut_tiles_host(img, p)
    assert x.shape == (1, 3, 32, 64) and x.dtype == np.float32
    assert x[0, :, 0, 0].tolist() == [-0.5, 0.5, np.float32(1) / np.float32(255) - np.float32(0.5)]
    assert np.all(x[0, :, 20:] == -0.5) and np.all(x[0, :, :, 50:] == -0.5)
    assert np.array_equal(x[0, :, :20, :50], (img.astype(np.float32) / np.float32(255) - np.float32(0.5)).transpose(2, 0, 1))
    with pytest.raises(_lib.KGLibraryError):
        tiling.cut_tiles_host(img[:, :, :2], p)
    with pytest.raises(_lib.KGLibraryError):
        tiling.cut_tiles_host(img.astype(np.float32), p)


@pytest.fixture(scope="module")
def lib():
    from kg_instance_segmentation_amd import build
    lib = ctypes.CDLL(build.build())
    lib.kg_last_error.restype = ctypes.c_char_p
    for name in ("kg_tile_cut", "kg_bitmask_clip", "kg_tile_stitch", "kg_label_table"):
        assert name in _lib.SYMBOLS
        getattr(lib, name).argtypes = _lib._SIGS[name]
        getattr(lib, name).restype = ctypes.c_int
    return lib


def test_entry_points_validate_on_the_host(lib):
    buf = (ctypes.c_char * 4096)()                         # stands for every device buffer: a failed check returns before any HIP call
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)

    def ints(*v):
        return (ctypes.c_int * len(v))(*v)

    def cut(image=p, H=70, W=131, ys=ints(0, 19, 38), ny=3, xs=ints(0, 33, 67), nx=3, th=32, tw=64, out=p):
        return lib.kg_tile_cut(image, H, W, ys, ny, xs, nx, th, tw, out, None)

    def stitch(tl=p, ys=ints(0, 19, 38), ny=3, xs=ints(0, 33, 67), nx=3, th=32, tw=64, H=70, W=131, labels=p):
        return lib.kg_tile_stitch(tl, ys, ny, xs, nx, th, tw, H, W, labels, None)

    grid_bad = [dict(ys=None), dict(xs=None), dict(H=0), dict(W=-1), dict(th=0), dict(tw=0), dict(ny=0), dict(nx=257), dict(ys=ints(-1, 19, 38)),
                dict(ys=ints(0, 19, 19)), dict(xs=ints(0, 67, 33)), dict(ys=ints(0, 19, 70)), dict(xs=ints(0, 33, 131)), dict(H=1 << 16, W=1 << 15),
                dict(th=1 << 14, tw=1 << 15)]
    for kw in grid_bad + [dict(image=None), dict(out=None), dict(tw=62), dict(out=ctypes.c_void_p(p.value + 4))]:
        assert cut(**kw) != 0 and b"kg_tile_cut" in lib.kg_last_error(), kw
    for kw in grid_bad + [dict(tl=None), dict(labels=None)]:
        assert stitch(**kw) != 0 and b"kg_tile_stitch" in lib.kg_last_error(), kw

    H, W = 5, 130
    ld = bitmasks.ld_words(H, W)

    def clip(words=p, ld_words=ld, n=2, H=H, W=W, vh=3, vw=70):
        return lib.kg_bitmask_clip(words, ld_words, n, H, W, vh, vw, None)

    for kw in (dict(words=None), dict(ld_words=ld + 1), dict(ld_words=ld - 2), dict(n=-1), dict(H=0), dict(W=0), dict(vh=-1), dict(vh=6), dict(vw=131),
               dict(vw=-1), dict(words=ctypes.c_void_p(p.value + 8))):
        assert clip(**kw) != 0 and b"kg_bitmask_clip" in lib.kg_last_error(), kw
    assert clip(n=0, words=None) == 0 and clip(vh=H, vw=W) == 0      # nothing to do: no launch, no device needed

    def table(labels=p, H=24, W=70, jobs=p, n=3, area=p, out=p):
        return lib.kg_label_table(labels, H, W, jobs, n, area, out, None)

    for kw in (dict(labels=None), dict(jobs=None), dict(out=None), dict(n=-1), dict(H=0), dict(W=0), dict(H=1 << 16, W=1 << 15),
               dict(jobs=ctypes.c_void_p(p.value + 2)), dict(out=ctypes.c_void_p(p.value + 4)), dict(area=ctypes.c_void_p(p.value + 4))):
        assert table(**kw) != 0 and b"kg_label_table" in lib.kg_last_error(), kw
    assert table(n=0, jobs=None, out=None, area=None) == 0


def test_cpu_tensors_are_refused():
    p = tiling.plan(20, 50, (32, 64), 8)
    m = bitmasks.BitMasks(torch.zeros(2, bitmasks.ld_words(32, 64), dtype=torch.int64), 32, 64)
    with pytest.raises(_lib.KGLibraryError):
        tiling.cut_tiles(torch.zeros(20, 50, 3, dtype=torch.uint8), p)
    with pytest.raises(_lib.KGLibraryError):
        tiling.stitch(torch.zeros(1, 32, 64, dtype=torch.int32), p)
    with pytest.raises(_lib.KGLibraryError):
        tiling.table_from_labels(torch.zeros(20, 50, dtype=torch.int32), np.zeros((0, 5), np.int32))
    with pytest.raises(_lib.KGLibraryError):
        tiling.clip_masks(m, 20, 50)
    with pytest.raises(_lib.KGLibraryError):
        tiling.assemble(p, [[m, np.zeros((2, 5), np.float32)]])
    with pytest.raises(_lib.KGLibraryError):
        instances.label_map(m, ids=np.arange(2))
    assert inference.predict_tiled is tiling.predict_tiled


def test_product_module_stands_alone():
    src = open(os.path.join(ROOT, "kg_instance_segmentation_amd", "tiling.py")).read()
    assert "oracle" not in src
