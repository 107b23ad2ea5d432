"""CPU: the polygon fill rule (polygons.py) in its host statement.  fill_host against a per-pixel loop that evaluates the rule in exact
rationals, against matplotlib's point-in-path where no centre lies on an edge, the two consequences of the rule (top-left inclusive and
watertight; exact round trip of contours_host), union / cover / painter's order / even-odd, degenerate and rejected input, the
constructors, the binning, and the binding table."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from kg_instance_segmentation_amd import _lib
from kg_instance_segmentation_amd import contours as ct
from kg_instance_segmentation_amd import polygons as pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = _lib.KGLibraryError


def one(ring, *more):
    """Polygons of one row, one part, the given rings"""
    return pg.from_rings([[[ring, *more]]])


def random_ring(rng, n, H, W, half):
    """n vertices in and a little around an H x W map; half: on the half-pixel lattice (centres on vertices and edges), else random floats"""
    if half:
        return np.stack([rng.integers(-2, 2 * W + 4, n), rng.integers(-2, 2 * H + 4, n)], 1) / 2.0
    return np.stack([rng.uniform(-1.5, W + 1.5, n), rng.uniform(-1.5, H + 1.5, n)], 1)


def rule_in_fractions(ring, H, W):
    """The rule per pixel in exact rationals, on the quantised vertices: an edge counts iff y0 <= cy < y1 and the x of its intersection
    with the scanline, a Fraction, is > cx.  No int64 cross-multiplication."""
    q = [(Fraction(int(np.rint(x * 256)), 256), Fraction(int(np.rint(y * 256)), 256)) for x, y in np.asarray(ring).tolist()]
    out = np.zeros((H, W), np.int32)
    for y in range(H):
        cy = Fraction(2 * y + 1, 2)
        xs = []
        for (xa, ya), (xb, yb) in zip(q, q[1:] + q[:1]):
            if ya == yb:
                continue
            if ya > yb:
                xa, ya, xb, yb = xb, yb, xa, ya
            if ya <= cy < yb:
                xs.append(xa + (xb - xa) * (cy - ya) / (yb - ya))
        for x in range(W):
            cx = Fraction(2 * x + 1, 2)
            out[y, x] = sum(v > cx for v in xs) & 1
    return out


def test_fill_host_equals_the_rule_in_fractions():
    rng = np.random.default_rng(0)
    for k in range(50):
        H, W = int(rng.integers(1, 25)), int(rng.integers(1, 25))
        ring = random_ring(rng, int(rng.integers(3, 13)), H, W, k % 3 == 0)
        assert np.array_equal(pg.fill_host(one(ring), H, W), rule_in_fractions(ring, H, W)), k


def centres_on_an_edge(ring, H, W):
    """bool [H, W]: the centre lies on an edge of the ring (in exact integers on the quantised vertices)"""
    q = np.rint(np.asarray(ring) * 256).astype(np.int64)
    cy, cx = np.meshgrid(256 * np.arange(H) + 128, 256 * np.arange(W) + 128, indexing="ij")
    on = np.zeros((H, W), bool)
    for (xa, ya), (xb, yb) in zip(q.tolist(), np.roll(q, -1, 0).tolist()):
        cross = (xb - xa) * (cy - ya) - (cx - xa) * (yb - ya)
        on |= (cross == 0) & (np.minimum(xa, xb) <= cx) & (cx <= np.maximum(xa, xb)) & (np.minimum(ya, yb) <= cy) & (cy <= np.maximum(ya, yb))
    return on


def test_fill_host_equals_matplotlib_off_the_edges():
    path = pytest.importorskip("matplotlib.path")
    rng = np.random.default_rng(1)
    total = left_out = left_out_float = 0
    for k in range(200):
        H, W = int(rng.integers(4, 33)), int(rng.integers(4, 33))
        half = k % 3 == 0
        ring = random_ring(rng, int(rng.integers(3, 13)), H, W, half)
        q = np.rint(ring * 256) / 256                                 # matplotlib sees the quantised vertices
        yy, xx = np.mgrid[0:H, 0:W]
        pts = np.stack([xx.reshape(-1) + 0.5, yy.reshape(-1) + 0.5], 1)
        codes = [path.Path.MOVETO] + [path.Path.LINETO] * (len(q) - 1) + [path.Path.CLOSEPOLY]
        inside = path.Path(np.concatenate([q, q[:1]]), codes).contains_points(pts, radius=0).reshape(H, W)
        on = centres_on_an_edge(ring, H, W)
        got = pg.fill_host(one(ring), H, W).astype(bool)
        assert np.array_equal(got[~on], inside[~on]), k
        total += H * W; left_out += int(on.sum()); left_out_float += 0 if half else int(on.sum())
    print("centres on an edge", left_out, "of", total)
    assert left_out_float == 0 and left_out <= total // 100


# ---- consequence 1: top-left inclusive, watertight ---------------------------------------------------------------------------------------

def test_ties_of_a_half_pixel_rectangle():
    """sides through pixel centres: the left column and the top row are inside, the right column and the bottom row outside"""
    out = pg.fill_host(one([(1.5, 0.5), (4.5, 0.5), (4.5, 3.5), (1.5, 3.5)]), 5, 6)
    want = np.zeros((5, 6), np.int32)
    want[0:3, 1:4] = 1
    assert np.array_equal(out, want)


def watertight(rows, H, W):
    out, cover = pg.fill_host(pg.from_rings(rows), H, W, cover=True)
    return out, cover


def test_watertight_rectangles_triangles_and_fan():
    # two rectangles that share the side x = 3.5, through centres, and two more below across y = 2.5
    rects = [[[[(0.5, 0.5), (3.5, 0.5), (3.5, 2.5), (0.5, 2.5)]]], [[[(3.5, 0.5), (6.5, 0.5), (6.5, 2.5), (3.5, 2.5)]]],
             [[[(0.5, 2.5), (3.5, 2.5), (3.5, 5.5), (0.5, 5.5)]]], [[[(3.5, 2.5), (6.5, 2.5), (6.5, 5.5), (3.5, 5.5)]]]]
    out, cover = watertight(rects, 7, 8)
    inside = np.zeros((7, 8), bool)
    inside[0:5, 0:6] = True
    assert np.array_equal(cover, inside.astype(np.int32)) and np.array_equal(out[0:5, 0:6], np.repeat(np.repeat([[1, 2], [3, 4]], [2, 3], 0), 3, 1))
    # two triangles along the diagonal of a square, through centres
    out, cover = watertight([[[[(0.5, 0.5), (6.5, 0.5), (6.5, 6.5)]]], [[[(0.5, 0.5), (6.5, 6.5), (0.5, 6.5)]]]], 8, 8)
    inside = np.zeros((8, 8), bool)
    inside[0:6, 0:6] = True
    assert np.array_equal(cover, inside.astype(np.int32)) and set(np.unique(out).tolist()) == {0, 1, 2}
    # a fan of 8 triangles around a vertex at a pixel centre, its rim through centres as well
    rim = [(0.5, 0.5), (4.5, 0.5), (8.5, 0.5), (8.5, 4.5), (8.5, 8.5), (4.5, 8.5), (0.5, 8.5), (0.5, 4.5)]
    fan = [[[[(4.5, 4.5), rim[k], rim[(k + 1) % 8]]]] for k in range(8)]
    out, cover = watertight(fan, 10, 10)
    inside = np.zeros((10, 10), bool)
    inside[0:8, 0:8] = True
    assert np.array_equal(cover, inside.astype(np.int32)) and (out[inside] > 0).all() and len(np.unique(out)) == 9


# ---- consequence 2: the exact round trip --------------------------------------------------------------------------------------------------

def round_trip(lab, ids):
    H, W = lab.shape
    c = ct.contours_host(lab, [[0, int(i), 0, 0, H, W] for i in ids])
    out = pg.fill_host(pg.from_contours(c), H, W, ids=ids, background=-5)
    traced = np.isin(lab, ids)
    assert np.array_equal(out[traced], lab[traced]) and (out[~traced] == -5).all()


def test_round_trip_of_contours_host():
    rng = np.random.default_rng(2)
    for k in range(12):
        H, W = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        round_trip(rng.integers(0, 4, (H, W)).astype(np.int32), [1, 2, 3])
    nested = np.array([[1, 1, 1, 1, 1], [1, 0, 0, 0, 1], [1, 0, 1, 0, 1], [1, 0, 0, 0, 1], [1, 1, 1, 1, 1]], np.int32)
    round_trip(np.kron(nested, np.ones((3, 4), np.int32)), [1])       # a ring with a hole and an island in it
    round_trip(nested, [1, 0])
    board = ((np.add.outer(np.arange(16), np.arange(16)) % 2) == 0).astype(np.int32)
    round_trip(board, [1])
    round_trip(board, [0, 1])


# ---- union, cover, order, even-odd -------------------------------------------------------------------------------------------------------

def square(x, y, s):
    return [(x, y), (x + s, y), (x + s, y + s), (x, y + s)]


def test_union_cover_and_painters_order():
    # row 0: two overlapping parts; row 1 overlaps both; row 2 apart
    p = pg.from_rings([[[square(1, 1, 4)], [square(3, 3, 4)]], [[square(4, 0, 5)]], [[square(10, 10, 2)]]])
    out, cover = pg.fill_host(p, 14, 14, ids=[7, 8, 9], cover=True)
    a = np.zeros((14, 14), bool); a[1:5, 1:5] = True; a[3:7, 3:7] = True
    b = np.zeros((14, 14), bool); b[0:5, 4:9] = True
    c = np.zeros((14, 14), bool); c[10:12, 10:12] = True
    assert np.array_equal(cover, a.astype(np.int32) + b + c) and cover.max() == 2         # a row counts once where its parts overlap
    assert np.array_equal(out, np.where(a, 7, np.where(b, 8, np.where(c, 9, 0))))
    last = pg.fill_host(p, 14, 14, ids=[7, 8, 9], top="last")
    assert np.array_equal(last, np.where(c, 9, np.where(b, 8, np.where(a, 7, 0))))
    with pytest.raises(E):
        pg.fill_host(p, 14, 14, top="middle")
    with pytest.raises(E):
        pg.fill_host(p, 14, 14, ids=[1, 2])
    with pytest.raises(E):
        pg.fill_host(p, 14, 14, ids=[1, 2, 2 ** 31])
    assert pg.fill_host(p, 14, 14, ids=[0, -1, -2 ** 31], background=2 ** 31 - 1)[0, 0] == 2 ** 31 - 1
    stack = pg.fill_host(p, 14, 14, ids=[7, 8, 9], img=[1, 0, 1])
    assert stack.shape == (2, 14, 14) and np.array_equal(stack[0], np.where(b, 8, 0)) and np.array_equal(stack[1], np.where(a, 7, np.where(c, 9, 0)))


def test_even_odd_on_self_intersections():
    bow = pg.fill_host(one([(0, 0), (8, 8), (8, 0), (0, 8)]), 8, 8)   # a bow-tie: two triangles that meet at (4, 4)
    yy, xx = np.mgrid[0:8, 0:8] + 0.5
    off = np.abs(yy - 4) != np.abs(xx - 4)                            # the centres on the two diagonals are ties
    assert np.array_equal(bow.astype(bool)[off], (np.abs(yy - 4) < np.abs(xx - 4))[off]) and bow.sum() > 20
    ang = np.pi / 2 + 4 * np.pi / 5 * np.arange(5)
    star = np.stack([20 + 18 * np.cos(ang), 20 - 18 * np.sin(ang)], 1)      # a pentagram: its centre has winding number 2
    out = pg.fill_host(one(star), 40, 40)
    assert out[20, 20] == 0 and out[5, 20] == 1 and out.sum() > 100


# ---- degenerate and rejected input ----------------------------------------------------------------------------------------------------------

def test_degenerate_rings_and_far_vertices():
    sq = square(1, 1, 3)
    want = pg.fill_host(one(sq), 6, 6)
    assert want.sum() == 9
    assert np.array_equal(pg.fill_host(one(sq + sq[:1]), 6, 6), want)                     # a repeated closing vertex costs nothing
    assert pg.edge_table(one(sq + sq[:1]))[0].shape == pg.edge_table(one(sq))[0].shape == (2, 4)
    for ring in ([], [(2, 2)], [(1, 1), (4, 4)], [(1, 2), (5, 2), (3, 2)]):               # none, one, two vertices; all on one scanline
        assert not pg.fill_host(one(ring), 6, 6).any()
        assert np.array_equal(pg.fill_host(one(sq, ring), 6, 6), want)
    assert not pg.fill_host(pg.from_rings([]), 3, 3).any() and not pg.fill_host(pg.from_rings([[], [[]]]), 3, 3).any()
    far = 2.0 ** 20
    big = pg.fill_host(one([(-far, -far), (far, -far), (far, far), (-far, far)]), 5, 7)
    assert big.all()
    tri = pg.fill_host(one([(-far, 2), (far, 2), (3, far)]), 6, 7)                        # sides with slopes of 2^-20 and 2^20
    assert not tri[:2].any() and tri[3:].all()
    assert pg.fill_host(one([(-2 ** 21, -2 ** 21), (2 ** 21, -2 ** 21), (0, 2 ** 21)]), 4, 4).all()      # exactly 2^29 after scaling


def test_rejections():
    for bad in (np.nan, np.inf, -np.inf, 2 ** 21 + 1, -2 ** 21 - 1.0):
        with pytest.raises(E):
            pg.fill_host(one([(0, 0), (4, 0), (bad, 4)]), 4, 4)
        with pytest.raises(E):
            pg.edge_table(one([(0, 0), (4, bad), (0, 4)]))
    with pytest.raises(E):
        pg.from_rings([[[[(0, 0, 0), (1, 1, 1)]]]])
    with pytest.raises(E):
        pg.fill_host(one(square(0, 0, 1)), 0, 4)
    with pytest.raises(E):
        pg.fill_host(one(square(0, 0, 1)), 4, 32769)
    with pytest.raises(E):
        pg.fill_host([[square(0, 0, 1)]], 4, 4)
    with pytest.raises(E):
        pg.Polygons([0, 2], [0, 1], [0, 0], np.zeros((0, 2)))


# ---- the structure and its constructors ------------------------------------------------------------------------------------------------------

def test_polygons_structure():
    p = pg.from_rings([[[square(1, 1, 2), square(1.5, 1.5, 1)], [square(5, 5, 1)]], [], [[square(0, 0, 8)]]])
    assert len(p) == 3 and p.counts().tolist() == [2, 0, 1] and p.verts.shape == (16, 2) and p.verts.dtype == np.float64
    assert [len(part) for part in p.of(0)] == [2, 1] and p.of(1) == [] and p.of(2)[0][0].tolist() == [[0, 0], [8, 0], [8, 8], [0, 8]]
    assert p.slice(0, 3) == p and p.slice(2, 3) == pg.from_rings([[[square(0, 0, 8)]]]) and len(p.slice(1, 1)) == 0 and p.slice(1, 2).of(0) == []
    assert p != pg.from_rings([[[square(0, 0, 8)]]]) and p != 3
    b = p.boxes()
    assert b[0].tolist() == [1, 1, 6, 6] and b[2].tolist() == [0, 0, 8, 8] and np.isinf(b[1]).all()


def test_from_coco():
    p = pg.from_coco([[[1, 1, 4, 1, 4, 4, 1, 4], [6, 6, 8, 6, 8, 8]], [], [[0.5, 0.5, 2.5, 0.5, 2.5, 2.5]]])
    assert len(p) == 3 and p.counts().tolist() == [2, 0, 1] and np.diff(p.ring_ptr).tolist() == [1, 1, 1]
    assert p.of(0)[1][0].tolist() == [[6, 6], [8, 6], [8, 8]]
    out = pg.fill_host(p, 9, 9)
    assert out[1:4, 1:4].all() and out[7, 6] == 0 and out[6, 7] == 1 and out[0, 1] == 3
    for bad in ([[[1, 1, 4, 1, 4]]], [{"counts": [1, 2], "size": [3, 3]}], [[[[1, 1], [2, 2]]]], [7]):
        with pytest.raises(E):
            pg.from_coco(bad)


def test_from_geojson():
    poly = {"type": "Polygon", "coordinates": [[[1, 1], [7, 1], [7, 7], [1, 7], [1, 1]], [[3, 3], [3, 5], [5, 5], [5, 3], [3, 3]]]}
    multi = {"type": "MultiPolygon", "coordinates": [[[[0, 0], [2, 0], [2, 2], [0, 2], [0, 0]]], [[[8, 8], [9, 8], [9, 9], [8, 9], [8, 8]]]]}
    empty = {"type": "MultiPolygon", "coordinates": []}
    p = pg.from_geojson([poly, multi, empty])
    assert len(p) == 3 and p.counts().tolist() == [1, 2, 0] and np.diff(p.ring_ptr).tolist() == [2, 1, 1]
    coll = {"type": "FeatureCollection", "features": [{"type": "Feature", "properties": {"name": "a"}, "geometry": g} for g in (poly, multi, empty)]}
    assert pg.from_geojson(coll) == p and pg.from_geojson(poly) == p.slice(0, 1) and pg.from_geojson(coll["features"][1]) == p.slice(1, 2)
    out = pg.fill_host(p, 10, 10, top="last")
    assert out[2, 2] == 1 and out[4, 4] == 0 and out[1, 1] == 2 and out[0, 0] == 2 and out[8, 8] == 2 and out.sum() == 32 - 1 + 2 * 5
    for bad in ({"type": "Point", "coordinates": [1, 2]}, {"type": "Polygon"}, 5, {"type": "Polygon", "coordinates": [[[1, 2, 3, 4], [1, 2, 3, 4]]]}):
        with pytest.raises(E):
            pg.from_geojson(bad)


def test_from_contours_and_the_geojson_export():
    lab = np.zeros((12, 15), np.int32)
    lab[1:10, 2:12] = 1
    lab[3:8, 4:10] = 0
    lab[5, 6:8] = 1                                                   # an island in the hole
    lab[10:12, 13:15] = 1                                             # a second outer ring
    lab[0, 0] = 2
    c = ct.contours_host(lab, [[0, 1, 0, 0, 12, 15], [0, 2, 0, 0, 12, 15], [0, 3, 0, 0, 12, 15]])
    p = pg.from_contours(c)
    assert len(p) == 3 and p.counts().tolist() == [1, 1, 1] and np.diff(p.ring_ptr).tolist() == [4, 1, 0]
    assert np.array_equal(p.verts, c.verts[:, ::-1]) and p.verts.dtype == np.float64
    assert np.array_equal(pg.fill_host(p, 12, 15), np.where(lab == 1, 1, np.where(lab == 2, 2, 0)))
    g = pg.from_geojson([c.geojson(0), c.geojson(1), c.geojson(2)])
    assert g.counts().tolist() == [3, 1, 0]                           # outer + hole, the island, the second outer ring
    assert np.array_equal(pg.fill_host(g, 12, 15), pg.fill_host(p, 12, 15))
    with pytest.raises(E):
        pg.from_contours(p)


# ---- the binning and the binding table ---------------------------------------------------------------------------------------------------------

def test_tile_lists_cover_every_meeting_pair_once():
    rng = np.random.default_rng(3)
    H, W, nimg = 70, 131, 2
    rows = []
    for k in range(40):
        cx, cy, r = rng.uniform(-10, W + 10), rng.uniform(-10, H + 10), rng.uniform(0.3, 60)
        rows.append([[square(cx - r, cy - r, 2 * r)] for _ in range(1 + k % 2)])
    rows.insert(5, [])
    rows.insert(9, [[[(3, 3), (9, 3)]]])                              # a part with no edge
    p = pg.from_rings(rows)
    img = rng.integers(0, nimg, len(p))
    edges, ranges, boxes = pg.edge_table(p)
    part_rows = p.part_rows()
    assert int(ranges[:, 1].sum()) == len(edges) and np.array_equal(ranges[:, 0], np.cumsum(ranges[:, 1]) - ranges[:, 1])
    ty_n, tx_n = -(-H // pg.TILE_H), -(-W // pg.TILE_W)
    for top in ("first", "last"):
        items, tile_ptr = pg.tile_lists(ranges, boxes, part_rows + 100, part_rows, H, W, img[part_rows], nimg, top)
        assert items.dtype == tile_ptr.dtype == np.int32 and tile_ptr[0] == 0 and tile_ptr[-1] == len(items) and len(tile_ptr) == nimg * ty_n * tx_n + 1
        for t in range(nimg * ty_n * tx_n):
            i, rest = divmod(t, ty_n * tx_n)
            ty, tx = divmod(rest, tx_n)
            y1, x1, y2, x2 = ty * pg.TILE_H, tx * pg.TILE_W, min((ty + 1) * pg.TILE_H, H), min((tx + 1) * pg.TILE_W, W)
            meet = [k for k in range(len(ranges)) if img[part_rows[k]] == i and ranges[k, 1] > 0 and
                    max(boxes[k, 0], y1) < min(boxes[k, 2], y2) and max(boxes[k, 1], x1) < min(boxes[k, 3], x2)]
            got = items[tile_ptr[t]:tile_ptr[t + 1]]
            want = meet[::-1] if top == "last" else meet              # every meeting part once, in row order
            assert got[:, 1].tolist() == ranges[want, 0].tolist() and got[:, 2].tolist() == ranges[want, 1].tolist()
            assert got[:, 3].tolist() == part_rows[want].tolist() and got[:, 0].tolist() == (part_rows[want] + 100).tolist()
    out = pg.fill_tables_host(edges, items, tile_ptr, nimg, H, W)[0]
    assert np.array_equal(out, pg.fill_host(p, H, W, ids=np.arange(len(p)) + 100, top="last", img=img, nimg=nimg))


def test_tables_state_the_rule():
    """fill_tables_host over the tables of a ragged set equals fill_host, cover included: the binning loses nothing"""
    rng = np.random.default_rng(4)
    H, W = 70, 131
    rows = [[[random_ring(rng, int(rng.integers(3, 9)), H, W, k % 2 == 0)] for _ in range(1 + k % 3)] for k in range(25)]
    p = pg.from_rings(rows)
    edges, items, tile_ptr, nimg = pg.tables(p, H, W)
    out, cover = pg.fill_tables_host(edges, items, tile_ptr, nimg, H, W, background=-1)
    want, want_cover = pg.fill_host(p, H, W, background=-1, cover=True)
    assert np.array_equal(out[0], want) and np.array_equal(cover[0], want_cover) and want_cover.max() > 2


def test_binding_table_and_header():
    hdr = open(os.path.join(ROOT, "include", "kgnet_hip.h")).read()
    assert "kg_polygons_fill" in _lib._SIGS and len(_lib._SIGS["kg_polygons_fill"]) == 12
    assert re.search(r"\bint kg_polygons_fill\(", hdr)
    src = open(os.path.join(ROOT, "kg_instance_segmentation_amd", "csrc", "polygons.hip")).read()
    for name, value in (("KG_POLY_TILE_H", pg.TILE_H), ("KG_POLY_TILE_W", pg.TILE_W), ("KG_POLY_EDGE_CHUNK", pg.EDGE_CHUNK)):
        for text in (hdr, src):                                       # the header, the kernel and polygons.py hold one value
            assert re.search(rf"#define {name} (\d+)", text).group(1) == str(value), name


def test_label_evaluator_takes_polygons_for_a_host_prediction():
    from kg_instance_segmentation_amd import labelmetrics as lm
    lab = np.zeros((20, 30), np.int32)
    lab[2:9, 3:12] = 1
    lab[10:18, 15:28] = 2
    p = pg.from_rings([[[square(3, 2, 7)]], [[[(15, 10), (28, 10), (28, 18), (15, 18)]]], [[square(0, 15, 3)]]])
    a, b = lm.LabelEvaluator(), lm.LabelEvaluator()
    a.add((lab, 2), p, conf=np.array([0.9, 0.8]))
    b.add((lab, 2), (pg.fill_host(p, 20, 30), 3), conf=np.array([0.9, 0.8]))
    sa, sb = a.summary(), b.summary()
    assert all(np.array_equal(sa[k], sb[k]) for k in sa) and sa["images"] == 1 and 0 < sa["pq"] < 1
