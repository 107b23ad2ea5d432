"""GPU: the tiled polygon fill on the device (csrc/polygons.hip, polygons.py) against the host statement of the same rule
(polygons.fill_host; polygons.fill_tables_host for tables no binning would build).  Every comparison is exact integer equality.  Shapes
are the smallest at which the kernel can go wrong: one-pixel, one-row and one-column maps, sides one pixel either side of and on every
tile seam, a polygon over 3 x 3 tiles, edge counts around the staging chunk with the y-filter keeping all or few, ties across a tile
corner, deep item lists, any int32 as a value, vertices far outside, empty rows and parts, several images in a launch, wrong tables
between guard rows, and every host check."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from kg_instance_segmentation_amd import KGnet, _lib, tiling  # noqa: E402
from kg_instance_segmentation_amd import contours as ct  # noqa: E402
from kg_instance_segmentation_amd import labelmetrics as lm  # noqa: E402
from kg_instance_segmentation_amd import polygons as pg  # noqa: E402

DEV = "cuda"
I32 = np.iinfo(np.int32)
E = _lib.KGLibraryError
TH, TW, CHUNK = pg.TILE_H, pg.TILE_W, pg.EDGE_CHUNK


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(p, H, W, **kw):
    """fill with and without cover against fill_host -> the host (out, cover)"""
    want, want_cover = pg.fill_host(p, H, W, cover=True, **kw)
    got, cover = pg.fill(p, H, W, DEV, cover=True, **kw)
    assert got.is_cuda and cover.is_cuda and got.dtype == cover.dtype == torch.int32 and tuple(got.shape) == tuple(cover.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(cover.cpu().numpy(), want_cover)
    plain = pg.fill(p, H, W, DEV, **kw)                               # cover=None: the kernel that may skip the rest of a list
    assert torch.is_tensor(plain) and np.array_equal(plain.cpu().numpy(), want)
    return want, want_cover


def square(x, y, w, h=None):
    h = w if h is None else h
    return [(x, y), (x + w, y), (x + w, y + h), (x, y + h)]


def disc(cx, cy, r, n=24, phase=0.1):
    a = phase + 2 * np.pi * np.arange(n) / n
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], 1)


def star(n, cx, cy, r1, r2):
    a = 0.1 + 2 * np.pi * np.arange(n) / n
    r = np.where(np.arange(n) % 2 == 0, r1, r2)
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], 1)


def rows_of(*rings):
    """one row, one part, one ring each"""
    return pg.from_rings([[[r]] for r in rings])


def ragged(H, W, n, seed):
    """n rows of 1 .. 3 parts of random rings, every other row on the half-pixel lattice (ties)"""
    rng = np.random.default_rng(seed)

    def ring(k):
        m = int(rng.integers(3, 10))
        if k % 2:
            return np.stack([rng.integers(-4, 2 * W + 8, m), rng.integers(-4, 2 * H + 8, m)], 1) / 2.0
        c = np.array([rng.uniform(0, W), rng.uniform(0, H)])
        return c + rng.uniform(-0.3, 0.3, (m, 2)) * [W, H]
    return pg.from_rings([[[ring(k)] for _ in range(1 + k % 3)] for k in range(n)])


# ---- smallest maps ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", [(1, 1), (1, 130), (130, 1)])
def test_smallest_maps(H, W):
    covering = square(-1, -1, W + 2, H + 2)
    missing = square(W + 3, H + 3, 4)
    tie_in = square(0.5, 0.5, W, H)                                   # its left and top sides pass through the centres of column 0 / row 0
    tie_out = square(-3, -3, 3.5)                                     # its right and bottom sides pass through the centre of pixel (0, 0)
    for rings in ([covering], [missing], [tie_in], [tie_out], [missing, tie_out, tie_in, covering]):
        want, cover = same(rows_of(*rings), H, W)
        if rings == [covering]:
            assert (want == 1).all()
        if rings in ([missing], [tie_out]):
            assert not want.any()
        if rings == [tie_in]:
            assert want.all()
        if len(rings) == 4:
            assert (want == 3).all() and (cover == 2).all()
    if H * W > 1:
        same(ragged(H, W, 12, H), H, W, background=-3)


def test_ragged_map():
    want, cover = same(ragged(70, 131, 30, 7), 70, 131, background=-1)
    assert cover.max() > 3 and (want == -1).any() and len(np.unique(want)) > 15


# ---- tiles ---------------------------------------------------------------------------------------------------------------------------------

def test_sides_around_every_tile_seam():
    H, W = 70, 131                                                    # seams at y = 32, 64 and x = 64, 128
    rings = []
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            rings.append(square(TW + a, TH + a, TW + b - a, TH + b - a))              # from one seam to the next
            rings.append(square(3, 2, TW + a - 3, TH + b - 2))                          # ends at the first seams
            rings.append(square(2 * TW + a, 2 * TH + b, W, H))                         # starts at the last seams
            rings.append(square(TW + a + 0.5, TH + b + 0.5, TW, TH))                    # sides through the centres next to the seams
    want, cover = same(rows_of(*rings), H, W)
    assert cover.max() >= 9
    for k, ring in enumerate(rings):                                  # each alone: a pixel short or long at a seam shows here
        alone, _ = same(rows_of(ring), H, W)
        (x1, y1), (x2, y2) = ring[0], ring[2]
        box = np.zeros((H, W), np.int32)
        box[int(np.ceil(y1 - 0.5)):int(np.ceil(y2 - 0.5)), int(np.ceil(x1 - 0.5)):int(np.ceil(x2 - 0.5))] = 1
        assert np.array_equal(alone, box), k


def test_one_polygon_over_three_by_three_tiles():
    H, W = 3 * TH - 5, 3 * TW - 9
    want, _ = same(pg.from_rings([[[disc(W / 2, H / 2, 200, 40), star(9, W / 2, H / 2, 40, 15)]]]), H, W, ids=[5])
    assert (want == 5).sum() > H * W // 2 and want[H // 2, W // 2] == 0


@pytest.mark.parametrize("n", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_edge_counts_around_the_staging_chunk(n):
    """a star of n edges inside one tile, where the staging filter keeps every edge, and over 5 x 3 tiles, where it keeps few"""
    for H, W, args in ((TH, TW, (31.3, 15.7, 14, 9)), (130, 130, (65.2, 64.6, 60, 35))):
        p = pg.from_rings([[[square(1, 1, 3)]], [[star(n, *args)]], [[square(W - 4, H - 4, 3)]]])
        assert pg.edge_table(p)[1][1].tolist() == [2, n]
        want, _ = same(p, H, W)
        assert (want == 2).sum() > 100


def test_watertight_fan_across_a_tile_corner():
    H, W = 2 * TH, 2 * TW
    cx, cy = TW + 0.5, TH + 0.5                                       # the centre of the first pixel of tile (1, 1)
    rim = [(cx - 9, cy - 9), (cx, cy - 9), (cx + 9, cy - 9), (cx + 9, cy), (cx + 9, cy + 9), (cx, cy + 9), (cx - 9, cy + 9), (cx - 9, cy)]
    fan = pg.from_rings([[[[(cx, cy), rim[k], rim[(k + 1) % 8]]]] for k in range(8)])
    want, cover = same(fan, H, W)
    inside = np.zeros((H, W), np.int32)
    inside[TH - 9:TH + 9, TW - 9:TW + 9] = 1
    assert np.array_equal(cover, inside) and np.array_equal(want > 0, inside > 0) and len(np.unique(want)) == 9


def test_forty_overlapping_discs():
    rng = np.random.default_rng(5)
    H, W = 70, 131
    p = rows_of(*[disc(rng.uniform(0, W), rng.uniform(0, H), rng.uniform(5, 25)) for _ in range(40)])
    first, cover = same(p, H, W)
    last, cover2 = same(p, H, W, top="last")
    assert cover.max() >= 5 and np.array_equal(cover, cover2) and (first != last).any()
    assert np.array_equal(first[cover == 1], last[cover == 1]) and (first[cover > 1] < last[cover > 1]).all()


def test_values_are_stored_only():
    ids = [0, -1, I32.min, I32.max, 7]
    p = rows_of(*[square(3 + 11 * k, 2, 9, 20) for k in range(5)])
    for background in (7, 0, I32.min):                                 # one of them equals a value each time
        want, cover = same(p, 24, 70, ids=ids, background=background)
        assert set(np.unique(want).tolist()) == set(ids) | {background} and cover.sum() == 5 * 9 * 20
    with pytest.raises(E):
        pg.fill(p, 24, 70, DEV, background=2 ** 31)
    with pytest.raises(E):
        pg.fill(p, 24, 70, "cpu")


def test_vertices_far_outside_the_map():
    far = 2.0 ** 20
    rings = [[(-far, -far), (far, -far), (far, far), (-far, far)], [(-far, 30.5), (far, 2), (40, far)], [(-far, -far), (66, 33), (-far, far)],
             [(far, -far), (far, far), (100.5, 20.5)], [(-2.0 ** 21, -2.0 ** 21), (2.0 ** 21, -2.0 ** 21), (0, 2.0 ** 21)]]
    want, cover = same(rows_of(*rings), 70, 131, top="last")
    assert cover.min() >= 2 and cover.max() >= 3
    for ring in rings[1:4]:
        alone, _ = same(rows_of(ring), 70, 131)
        assert alone.any() and not alone.all()


def test_rows_without_parts_and_parts_without_edges():
    live = square(2, 2, 60, 30)
    p = pg.from_rings([[[live]], [], [[[(1, 5), (90, 5)]]], [[], [[]], [[(4, 4)]]], [[square(50, 20, 60, 30)]], []])
    assert len(p) == 6 and p.counts().tolist() == [1, 0, 1, 3, 1, 0]
    want, cover = same(p, 70, 131)
    assert set(np.unique(want).tolist()) == {0, 1, 5} and cover.max() == 2
    none, zero = same(pg.from_rings([]), 70, 131, background=9)       # no row at all: every tile is empty
    assert (none == 9).all() and not zero.any()


def test_three_images_in_one_launch():
    H, W = 40, 67
    p = ragged(H, W, 21, 11)
    img = np.arange(21) % 3                                           # interleaved rows
    want, _ = same(p, H, W, img=img, ids=np.arange(21) + 10)
    assert want.shape == (3, H, W)
    for i in range(3):
        rows = np.flatnonzero(img == i)
        alone = pg.fill_host(pg.from_rings([p.of(k) for k in rows]), H, W, ids=rows + 10)
        assert np.array_equal(want[i], alone) and alone.any()
    four, _ = same(p, H, W, img=img, nimg=4, top="last")              # an image no row names is background
    assert four.shape == (4, H, W) and not four[3].any()


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


def test_round_trip_on_the_device():
    H, W, n = 70, 131, 14
    lab = blob_map(H, W, n, 3)
    d = up(lab)
    c = ct.contours(d, n)
    assert c.is_hole().any()
    got = pg.fill(pg.from_contours(c), H, W, DEV)
    assert torch.equal(got, d)
    some = [2, 5, 9]
    jobs = [[0, i, 0, 0, H, W] for i in some]
    got, cover = pg.fill(pg.from_contours(ct.contours(d, jobs=jobs)), H, W, DEV, ids=some, background=-1, cover=True)
    traced = np.isin(lab, some)
    assert np.array_equal(got.cpu().numpy(), np.where(traced, lab, -1)) and np.array_equal(cover.cpu().numpy(), traced.astype(np.int32))


# ---- the raw entry -----------------------------------------------------------------------------------------------------------------------

GUARD = 16                                                            # int32 words: 64 bytes, so the 16-byte rows stay aligned


def raw_between_guards(edges, items, tile_ptr, nimg, H, W, background, with_cover=True):
    """kg_polygons_fill on tables and outputs that each lie between guard words -> (out, cover); the guards and the tables must come back
    as they went"""
    parts = [np.asarray(a, np.int32).reshape(-1) for a in (edges, items, tile_ptr)]
    g = np.full(GUARD, -77, np.int32)
    host = np.concatenate([g, parts[0], g, parts[1], g, parts[2], g])
    buf = up(host)
    at = np.cumsum([GUARD, len(parts[0]) + GUARD, len(parts[1]) + GUARD])
    de = buf[at[0]:at[0] + len(parts[0])].view(-1, 4)
    di = buf[at[1]:at[1] + len(parts[1])].view(-1, 4)
    dp = buf[at[2]:at[2] + len(parts[2])]
    n = nimg * H * W
    outs = torch.full((2, n + 2 * GUARD), -77, dtype=torch.int32, device=DEV)
    out, cover = outs[0, GUARD:GUARD + n].view(nimg, H, W), outs[1, GUARD:GUARD + n].view(nimg, H, W)
    got = pg.fill_tables(de, di, dp, nimg, H, W, background, out=out, cover=cover if with_cover else None)
    assert (got[0] if with_cover else got) is out
    o = outs.cpu().numpy()
    assert (o[:, :GUARD] == -77).all() and (o[:, GUARD + n:] == -77).all() and np.array_equal(buf.cpu().numpy(), host)
    if not with_cover:
        assert (o[1] == -77).all()
    return o[0, GUARD:GUARD + n].reshape(nimg, H, W), o[1, GUARD:GUARD + n].reshape(nimg, H, W)


def test_wrong_tables_between_guard_rows():
    H, W = 70, 131
    p = ragged(H, W, 30, 13)
    edges, items, tile_ptr, nimg = pg.tables(p, H, W)
    En, n, nt = len(edges), len(items), len(tile_ptr) - 1
    assert nt == 9 and n > 40 and En > 100

    def check(items, tile_ptr):
        want, want_cover = pg.fill_tables_host(edges, items, tile_ptr, 1, H, W, -2)
        got, cover = raw_between_guards(edges, items, tile_ptr, 1, H, W, -2)
        assert np.array_equal(got, want) and np.array_equal(cover, want_cover)
        plain, _ = raw_between_guards(edges, items, tile_ptr, 1, H, W, -2, with_cover=False)
        assert np.array_equal(plain, want)
        return want
    right = check(items, tile_ptr)
    assert np.array_equal(right[0], pg.fill_host(p, H, W, background=-2))
    # the first level: decreasing pairs are empty ranges, ranges beyond n_items are clamped
    t = tile_ptr.copy()
    t[2], t[3] = tile_ptr[3], tile_ptr[2]
    t[5] = -5
    t[7] = I32.max
    t[9] = n + 1000
    wrong = check(items, t)
    assert (wrong != right).any()
    t = np.full(nt + 1, I32.min, np.int32); t[4:] = I32.max           # tile 3 walks every item, the others none
    wrong = check(items, t)
    assert (wrong[0, :TH, :] == -2).all() and (wrong[0, TH:2 * TH, TW:] == -2).all() and (wrong[0, TH:2 * TH, :TW] != -2).any()
    check(items, tile_ptr[::-1].copy())
    # the second level: a failing predicate empties the item
    it = items.copy()
    bad = [(-1, 3), (0, -1), (En, 1), (En - 1, 2), (0, I32.max), (I32.min, 4), (I32.max, I32.max), (-1, 1), (I32.min, I32.min), (1, En)]
    at = np.linspace(0, n - 1, len(bad)).astype(int)
    for k, (first, count) in zip(at.tolist(), bad):
        it[k, 1], it[k, 2] = first, count
    it[at[-1] - 1, 1:3] = En, 0                                       # passes, and holds no edge
    it[at[-1] - 2, 1:3] = 0, En                                       # passes: every edge of the table as one part
    wrong = check(it, tile_ptr)
    assert (wrong != right).any()
    # rows that come back in a list: cover counts an item whose row differs from the last one the pixel counted
    sq = pg.edge_table(rows_of(square(1, 1, 5), square(3, 3, 5)))[0]
    lists = np.array([[4, 0, 2, 5], [6, 2, 2, 6], [8, 0, 2, 5], [9, 0, 2, 5], [1, 2, 2, 5]], np.int32)
    want, want_cover = pg.fill_tables_host(sq, lists, [0, 5], 1, 9, 9, 0)
    got, cover = raw_between_guards(sq, lists, [0, 5], 1, 9, 9, 0)
    assert np.array_equal(got, want) and np.array_equal(cover, want_cover) and cover[0, 4, 4] == 3 and cover[0, 1, 1] == 1 and cover[0, 7, 7] == 2
    # no edge, no item
    got, cover = raw_between_guards(np.zeros((0, 4)), np.zeros((0, 4)), np.zeros(nt + 1), 1, H, W, 3)
    assert (got == 3).all() and not cover.any()


def test_every_host_check_raises_before_a_launch():
    from kg_instance_segmentation_amd._lib import ptr, stream_ptr
    H, W = 40, 70
    edges, items, tile_ptr, _ = pg.tables(rows_of(square(2, 2, 30)), H, W)
    de, di, dp = pg.upload_tables(edges, items, tile_ptr, torch.device(DEV))
    out = torch.full((2, H, W), -7, dtype=torch.int32, device=DEV)
    o, c = out[0], out[1]
    En, n = len(edges), len(items)

    def off(t, nbytes):
        return ctypes.c_void_p(t.data_ptr() + nbytes)

    def call(**kw):
        a = dict(edges=ptr(de), E=En, items=ptr(di), n=n, tile_ptr=ptr(dp), nimg=1, H=H, W=W, out=ptr(o), cover=ptr(c))
        a.update(kw)
        _lib.call("kg_polygons_fill", a["edges"], a["E"], a["items"], a["n"], a["tile_ptr"], a["nimg"], a["H"], a["W"], 0, a["out"], a["cover"], stream_ptr())
    bad = [dict(nimg=0), dict(H=0), dict(W=0), dict(H=-1), dict(W=32769), dict(H=32769), dict(nimg=3, H=32768, W=32768), dict(E=-1), dict(n=-1),
           dict(out=None), dict(tile_ptr=None), dict(edges=None), dict(items=None),
           dict(edges=off(de, 4)), dict(items=off(di, 8)), dict(tile_ptr=off(dp, 2)), dict(out=off(o, 1)), dict(cover=off(c, 2)),
           dict(cover=ptr(o)), dict(cover=off(o, 4 * W)), dict(out=ptr(dp)), dict(out=ptr(de)), dict(out=ptr(di)), dict(cover=ptr(de)),
           dict(cover=ptr(di)), dict(cover=ptr(dp))]
    for kw in bad:
        with pytest.raises(E, match="kg_polygons_fill"):
            call(**kw)
    torch.cuda.synchronize()
    assert (out == -7).all()                                          # nothing was launched
    call(edges=None, E=0, items=None, n=0, cover=None)                # valid: NULL tables with zero sizes, no cover
    assert (o == 0).all() and (c == -7).all()
    for kw in (dict(nimg=2), dict(background=2 ** 31), dict(out=o), dict(cover=out), dict(out=out.to(torch.int64)[:1])):
        with pytest.raises(E):
            pg.fill_tables(de, di, dp, kw.pop("nimg", 1), H, W, **kw)
    with pytest.raises(E):
        pg.fill_tables(de.cpu(), di, dp, 1, H, W)
    with pytest.raises(E):
        pg.fill_tables(de, di.view(-1), dp, 1, H, W)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cal_model():
    from oracle import weightgen
    m = KGnet.resnet50(pretrained=False)
    m.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    return m.to(DEV).eval()


def test_predict_tiled_round_trip_and_polygon_ground_truth(cal_model):
    H, W, S = 400, 600, 256
    img = np.random.default_rng(8).integers(0, 256, (H, W, 3), dtype=np.uint8)
    inst = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4, contours=True)
    n = len(inst)
    p = pg.from_contours(inst.contours)
    print("instances", n, "edges", len(pg.edge_table(p)[0]))
    assert n > 2 and len(p) == n
    assert torch.equal(pg.fill(p, H, W, inst.labels.device), inst.labels)
    gt = pg.from_rings([p.of(k) for k in range(n - 2)] + [[[square(10, 10, 50)]]])     # not the prediction: two rows fewer, one that fills gaps
    a, b = lm.LabelEvaluator(), lm.LabelEvaluator()
    a.add(inst, gt)
    b.add(inst, (pg.fill_host(gt, H, W), len(gt)))
    sa, sb = a.summary(), b.summary()
    print("summary", {k: sa[k] for k in ("kaggle", "pq", "aji", "dice")})
    for k in sa:                                                      # a threshold nothing matched at has a NaN mean IoU in both
        assert (sa[k] is None and sb[k] is None) or np.array_equal(np.asarray(sa[k], np.float64), np.asarray(sb[k], np.float64), equal_nan=True), k
    assert sa["images"] == 1 and 0 < sa["pq"] <= 1
