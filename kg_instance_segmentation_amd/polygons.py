"""Polygon annotations to label maps on the device: the exact tiled polygon fill, the inverse of contours.py.

Nucleus ground truth ships as polygons (MoNuSeg's XML vertex lists, QuPath / GeoJSON exports, COCO annotation files, napari shapes).
Here the host turns the vertices into one integer edge table and per-tile item lists, the device fills every pixel of the map in one
launch (kg_polygons_fill, csrc/polygons.hip), and the map stays on the device for labelmetrics.LabelEvaluator.

    Polygons        host CSR: rows -> parts -> rings -> float64 vertices (x, y); of(k), slice, boxes()
    from_rings      nested lists: rows of parts of rings of (x, y)
    from_coco       COCO `segmentation` lists: per object a list of flat [x0, y0, x1, y1, ...] lists, each one a part of one ring
    from_geojson    Polygon / MultiPolygon geometries (Feature / FeatureCollection wrappers accepted)
    from_contours   a contours.Contours: one part per row holding all its rings
    edge_table      the quantisation: int32 [E, 4] edges, per-part ranges and pixel boxes
    tile_lists      the binning: items and tile_ptr of kg_polygons_fill
    fill_host       the rule below in plain NumPy: the yardstick
    fill            fill_host on the device: one upload, ONE launch, no copy back
    fill_tables     kg_polygons_fill as it is, on device tensors
    fill_tables_host  the statement of kg_polygons_fill for ANY tables, wrong ones included

The rule (include/kgnet_hip.h is the normative text)
  lattice      that of contours.py: pixel (y, x) is the square between vertices (x, y) and (x + 1, y + 1); its centre is (x + 0.5, y + 0.5).
  fixed point  F = 256: q = rint(v * 256) (round-half-even); non-finite values and |q| > 2^29 are rejected; a pixel centre is
               (256 x + 128, 256 y + 128).  Coordinate differences fit int32, products are 32 x 32 -> 64 bit.
  edges        every ring contributes its edges, the closing one included, each ordered upward as (x0, y0, x1, y1) with y0 < y1;
               horizontal edges are dropped.  A ring that repeats its first vertex costs nothing; a ring of one or two vertices covers
               nothing.
  crossing     an edge counts for a centre (cx, cy) iff y0 <= cy < y1 and (x1 - x0) * (cy - y0) > (cx - x0) * (y1 - y0): its
               intersection with the scanline lies strictly right of the centre.
  part         a list of rings; covers a pixel iff the number of counting edges over all its rings is odd (even-odd).
  row          a list of parts with one int32 value; covers a pixel iff any of its parts does (union).
  map          out[y, x] = the value of the first row, in row order, that covers the pixel, else background; top="last" reverses the row
               order.  cover[y, x] = the number of rows that cover the pixel.
Consequences: a centre exactly on a left or top edge is inside, on a right or bottom edge outside; polygons that share edges give every
pixel to exactly one of them; fill(from_contours(contours(lab, ...))) gives lab back exactly on the pixels of the traced ids."""
import numpy as np

from . import _lib
from ._labelmaps import MAX_SIDE, is_device

KGLibraryError = _lib.KGLibraryError
F = 256
Q_MAX = 2 ** 29
TILE_H, TILE_W = 32, 64                 # KG_POLY_TILE_H, KG_POLY_TILE_W of include/kgnet_hip.h
EDGE_CHUNK = 256                        # KG_POLY_EDGE_CHUNK


class Polygons:
    """Host CSR: row k owns the parts part_ptr[k] .. part_ptr[k + 1]; part p owns the rings ring_ptr[p] .. ring_ptr[p + 1]; ring r owns the
    vertices verts[vert_ptr[r] : vert_ptr[r + 1]] as (x, y).  The three pointers are int64, verts is float64 [V, 2]."""
    __slots__ = ("part_ptr", "ring_ptr", "vert_ptr", "verts")

    def __init__(self, part_ptr, ring_ptr, vert_ptr, verts):
        self.part_ptr, self.ring_ptr, self.vert_ptr = (np.ascontiguousarray(a, np.int64).reshape(-1) for a in (part_ptr, ring_ptr, vert_ptr))
        self.verts = np.ascontiguousarray(verts, np.float64).reshape(-1, 2)
        for name, p, total in (("part_ptr", self.part_ptr, len(self.ring_ptr) - 1), ("ring_ptr", self.ring_ptr, len(self.vert_ptr) - 1),
                               ("vert_ptr", self.vert_ptr, len(self.verts))):
            if len(p) < 1 or p[0] != 0 or p[-1] != total or (np.diff(p) < 0).any():
                raise KGLibraryError(f"Polygons: {name} of {len(p)} entries ending at {p[-1] if len(p) else None} for {total}")

    def __len__(self):
        return len(self.part_ptr) - 1

    def __eq__(self, other):
        return isinstance(other, Polygons) and all(np.array_equal(getattr(self, k), getattr(other, k)) for k in self.__slots__)

    __hash__ = None

    def counts(self):
        """int64 [m]: the number of parts of every row"""
        return np.diff(self.part_ptr)

    def part_rows(self):
        """int64 [P]: the row every part belongs to"""
        return np.repeat(np.arange(len(self), dtype=np.int64), self.counts())

    def slice(self, r0, r1):
        """The Polygons of rows r0 .. r1 - 1"""
        a, b = int(self.part_ptr[r0]), int(self.part_ptr[r1])
        ra, rb = int(self.ring_ptr[a]), int(self.ring_ptr[b])
        va, vb = int(self.vert_ptr[ra]), int(self.vert_ptr[rb])
        return Polygons(self.part_ptr[r0:r1 + 1] - a, self.ring_ptr[a:b + 1] - ra, self.vert_ptr[ra:rb + 1] - va, self.verts[va:vb])

    def ring(self, r):
        """float64 [count, 2] of (x, y): the vertices of ring r"""
        return self.verts[int(self.vert_ptr[r]):int(self.vert_ptr[r + 1])]

    def of(self, k):
        """The parts of row k: a list of parts, each a list of float64 [count, 2] arrays of (x, y)"""
        return [[self.ring(r) for r in range(int(self.ring_ptr[p]), int(self.ring_ptr[p + 1]))]
                for p in range(int(self.part_ptr[k]), int(self.part_ptr[k + 1]))]

    def boxes(self):
        """float64 [m, 4] = (x1, y1, x2, y2): the bounding box of the vertices of every row; (inf, inf, -inf, -inf) for a row with none"""
        out = np.empty((len(self), 4))
        out[:, :2], out[:, 2:] = np.inf, -np.inf
        first = self.vert_ptr[self.ring_ptr[self.part_ptr]]
        rows = np.repeat(np.arange(len(self)), np.diff(first))
        np.minimum.at(out[:, 0], rows, self.verts[:, 0]); np.minimum.at(out[:, 1], rows, self.verts[:, 1])
        np.maximum.at(out[:, 2], rows, self.verts[:, 0]); np.maximum.at(out[:, 3], rows, self.verts[:, 1])
        return out


# ---- constructors -------------------------------------------------------------------------------------------------------------------------

def _ring(fn, v):
    try:
        a = np.asarray(v, np.float64)
    except (TypeError, ValueError):
        raise KGLibraryError(f"{fn}: a ring must be numbers [n, 2] of (x, y)") from None
    if a.size == 0:
        return np.zeros((0, 2))
    if a.ndim != 2 or a.shape[1] != 2:
        raise KGLibraryError(f"{fn}: a ring must be numbers [n, 2] of (x, y), not an array of shape {a.shape}")
    return a


def from_rings(rows):
    """rows: a list of rows; a row: a list of parts; a part: a list of rings; a ring: [n, 2] of (x, y) -> Polygons.  MoNuSeg's XML is
    this over its vertex lists: one row per Region, one part, one ring."""
    part_ptr, ring_ptr, vert_ptr, verts = [0], [0], [0], []
    for row in rows:
        for part in row:
            for ring in part:
                a = _ring("from_rings", ring)
                verts.append(a)
                vert_ptr.append(vert_ptr[-1] + len(a))
            ring_ptr.append(len(vert_ptr) - 1)
        part_ptr.append(len(ring_ptr) - 1)
    return Polygons(part_ptr, ring_ptr, vert_ptr, np.concatenate(verts) if verts else np.zeros((0, 2)))


def from_coco(segmentations):
    """segmentations: per object, COCO's `segmentation` polygon list: flat [x0, y0, x1, y1, ...] lists, each one a part of one ring ->
    Polygons, one row per object.  An odd length is rejected (and so is the run-length form: runlengths.py reads that)."""
    rows = []
    for k, seg in enumerate(segmentations):
        if isinstance(seg, dict) or not isinstance(seg, (list, tuple)):
            raise KGLibraryError(f"from_coco: object {k} is no list of polygons (run lengths go through runlengths.py)")
        parts = []
        for flat in seg:
            a = np.asarray(flat, np.float64) if np.ndim(flat) == 1 else None
            if a is None or len(a) % 2:
                raise KGLibraryError(f"from_coco: a polygon of object {k} is not a flat list of an even number of coordinates")
            parts.append([a.reshape(-1, 2)])
        rows.append(parts)
    return from_rings(rows)


def _geometries(g):
    if isinstance(g, dict) and g.get("type") == "FeatureCollection":
        return [x for f in g.get("features", []) for x in _geometries(f)]
    if isinstance(g, dict) and g.get("type") == "Feature":
        return _geometries(g.get("geometry"))
    if isinstance(g, dict):
        return [g]
    if isinstance(g, (list, tuple)):
        return [x for f in g for x in _geometries(f)]
    raise KGLibraryError(f"from_geojson: {type(g).__name__} is no geometry, Feature or FeatureCollection")


def _position_ring(ring):
    """A linear ring of GeoJSON positions [x, y] or [x, y, z] -> [n, 2]"""
    try:
        a = np.asarray(ring, np.float64)
    except (TypeError, ValueError):
        a = None
    if a is None or not (a.size == 0 or (a.ndim == 2 and a.shape[1] in (2, 3))):
        raise KGLibraryError("from_geojson: a ring must be a list of positions [x, y]")
    return a.reshape(-1, a.shape[-1] if a.size else 2)[:, :2]


def from_geojson(geometries):
    """geometries: a GeoJSON geometry, Feature or FeatureCollection, or a list of them, in pixel coordinates [x, y] -> Polygons, one row per
    geometry: a Polygon is one part (its outer ring and its holes), a MultiPolygon one part per polygon (none for an empty one)."""
    rows = []
    for g in _geometries(geometries):
        kind, coords = g.get("type"), g.get("coordinates")
        if kind not in ("Polygon", "MultiPolygon") or not isinstance(coords, (list, tuple)):
            raise KGLibraryError(f"from_geojson: a geometry of type {kind!r} is no Polygon or MultiPolygon with coordinates")
        polys = [coords] if kind == "Polygon" else coords
        rows.append([[_position_ring(ring) for ring in poly] for poly in polys])
    return from_rings(rows)


def from_contours(c):
    """A contours.Contours -> Polygons with one part per row holding all its rings, (y, x) swapped to (x, y): outer rings, holes and
    islands in holes need no orientation under the even-odd rule."""
    from .contours import Contours
    if not isinstance(c, Contours):
        raise KGLibraryError("from_contours: a Contours")
    m = len(c)
    return Polygons(np.arange(m + 1), c.ring_ptr, np.concatenate([[0], np.cumsum(c.count)]), c.verts[:, ::-1].astype(np.float64))


# ---- quantisation and binning -----------------------------------------------------------------------------------------------------------------

def _ceil_div(a, b):
    return -((-a) // b)


def edge_table(polys):
    """The quantisation -> (edges int32 [E, 4] = (x0, y0, x1, y1) with y0 < y1, ranges int64 [P, 2] = (edge_first, edge_count) of every
    part, boxes int64 [P, 4] = (y1, x1, y2, x2): the half-open box of the pixels whose centres lie in the bounding box of the part's
    edges -- no pixel outside it can be covered; all zero for a part with no edge).  The edges of a part are contiguous, in ring order."""
    if not isinstance(polys, Polygons):
        raise KGLibraryError("edge_table: a Polygons")
    v = polys.verts
    if not np.isfinite(v).all():
        raise KGLibraryError("edge_table: a vertex is not finite")
    q = np.rint(v * F)
    if (np.abs(q) > Q_MAX).any():
        raise KGLibraryError(f"edge_table: a vertex lies beyond {Q_MAX // F} pixels")
    q = q.astype(np.int64)
    n = np.diff(polys.vert_ptr)
    nxt = np.arange(len(q), dtype=np.int64) + 1
    last = polys.vert_ptr[1:][n > 0] - 1
    nxt[last] = polys.vert_ptr[:-1][n > 0]                            # the closing edge
    a, b = q, q[nxt]
    keep = a[:, 1] != b[:, 1]
    up = (a[:, 1] < b[:, 1])[:, None]
    lo, hi = np.where(up, a, b)[keep], np.where(up, b, a)[keep]
    edges = np.concatenate([lo, hi], 1).astype(np.int32).reshape(-1, 4)
    ring_part = np.repeat(np.arange(len(polys.ring_ptr) - 1, dtype=np.int64), np.diff(polys.ring_ptr))
    part = np.repeat(ring_part, n)[keep]                              # non-decreasing
    P = len(polys.ring_ptr) - 1
    count = np.bincount(part, minlength=P).astype(np.int64)
    first = np.cumsum(count) - count
    boxes = np.zeros((P, 4), np.int64)
    live = np.flatnonzero(count)
    if len(live):
        e = edges.astype(np.int64)
        at = first[live]
        xmin, xmax = np.minimum.reduceat(np.minimum(e[:, 0], e[:, 2]), at), np.maximum.reduceat(np.maximum(e[:, 0], e[:, 2]), at)
        ymin, ymax = np.minimum.reduceat(e[:, 1], at), np.maximum.reduceat(e[:, 3], at)
        half = F // 2                                                 # ymin <= 256 y + 128 < ymax, xmin <= 256 x + 128 < xmax
        boxes[live] = np.stack([_ceil_div(ymin - half, F), _ceil_div(xmin - half, F), _ceil_div(ymax - half, F), _ceil_div(xmax - half, F)], 1)
    return edges, np.stack([first, count], 1), boxes


def _per_part(fn, polys, ids, img, nimg):
    """-> (value, row, image) of every part, and nimg"""
    m = len(polys)
    if ids is None:
        ids = np.arange(1, m + 1, dtype=np.int64)
    ids = np.asarray(ids)
    if ids.shape != (m,) or ids.dtype.kind not in "iu" or (m and (ids.min() < -2 ** 31 or ids.max() > 2 ** 31 - 1)):
        raise KGLibraryError(f"{fn}: ids must be {m} integers that fit int32")
    if img is None:
        img, nimg = np.zeros(m, np.int64), 1 if nimg is None else int(nimg)
    else:
        img = np.asarray(img)
        if img.shape != (m,) or img.dtype.kind not in "iu" or (m and img.min() < 0):
            raise KGLibraryError(f"{fn}: img must be {m} non-negative integers")
        nimg = (int(img.max()) + 1 if m else 1) if nimg is None else int(nimg)
    if nimg < 1 or (m and img.max() >= nimg):
        raise KGLibraryError(f"{fn}: nimg {nimg} does not hold every image index")
    rows = polys.part_rows()
    return ids.astype(np.int64)[rows], rows, img.astype(np.int64)[rows], nimg


def _sizes(fn, nimg, H, W):
    nimg, H, W = int(nimg), int(H), int(W)
    if nimg < 1 or H < 1 or W < 1 or H > MAX_SIDE or W > MAX_SIDE or nimg * H * W > 2 ** 31 - 1:
        raise KGLibraryError(f"{fn}: nimg {nimg}, H {H}, W {W}: sides of 1 .. {MAX_SIDE} and at most 2^31 - 1 pixels")
    return nimg, H, W


def _top(fn, top):
    if top not in ("first", "last"):
        raise KGLibraryError(f"{fn}: top must be 'first' or 'last'")
    return top == "last"


def tile_lists(ranges, boxes, values, rows, H, W, img=None, nimg=1, top="first"):
    """The binning.  Per part: ranges [P, 2] and boxes [P, 4] of edge_table, values [P], rows [P] (non-decreasing), img [P] (default 0) ->
    (items int32 [n, 4] = {value, edge_first, edge_count, row}, tile_ptr int32 [nimg * tiles + 1]): every part with an edge in every
    TILE_H x TILE_W tile its box, clamped to the map, meets; a tile's items in row order, reversed for top="last"."""
    nimg, H, W = _sizes("tile_lists", nimg, H, W)
    ranges, boxes = np.asarray(ranges, np.int64).reshape(-1, 2), np.asarray(boxes, np.int64).reshape(-1, 4)
    P = len(ranges)
    values, rows = np.asarray(values, np.int64).reshape(-1), np.asarray(rows, np.int64).reshape(-1)
    img = np.zeros(P, np.int64) if img is None else np.asarray(img, np.int64).reshape(-1)
    if not len(boxes) == len(values) == len(rows) == len(img) == P:
        raise KGLibraryError("tile_lists: ranges, boxes, values, rows and img must have one entry per part")
    order = np.arange(P)[::-1] if _top("tile_lists", top) else np.arange(P)
    ty_n, tx_n = _ceil_div(H, TILE_H), _ceil_div(W, TILE_W)
    ntiles = nimg * ty_n * tx_n
    y1, x1 = np.clip(boxes[order, 0], 0, H), np.clip(boxes[order, 1], 0, W)
    y2, x2 = np.clip(boxes[order, 2], 0, H), np.clip(boxes[order, 3], 0, W)
    live = (y2 > y1) & (x2 > x1) & (ranges[order, 1] > 0) & (img[order] >= 0) & (img[order] < nimg)
    order, y1, x1, y2, x2 = order[live], y1[live], x1[live], y2[live], x2[live]
    ty0, tx0 = y1 // TILE_H, x1 // TILE_W
    nty, ntx = (y2 - 1) // TILE_H - ty0 + 1, (x2 - 1) // TILE_W - tx0 + 1
    cnt = nty * ntx
    n = int(cnt.sum())
    if n > 2 ** 31 - 1:
        raise KGLibraryError(f"tile_lists: {n} (tile, part) pairs exceed 2^31 - 1")
    b = np.repeat(np.arange(len(order)), cnt)
    k = np.arange(n, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    tile = (img[order][b] * ty_n + ty0[b] + k // ntx[b]) * tx_n + tx0[b] + k % ntx[b]
    part = order[b[np.argsort(tile, kind="stable")]]
    items = np.stack([values[part], ranges[part, 0], ranges[part, 1], rows[part]], 1).reshape(-1, 4)
    if items.size and (items.min() < -2 ** 31 or items.max() > 2 ** 31 - 1):
        raise KGLibraryError("tile_lists: an item does not fit int32")
    tile_ptr = np.zeros(ntiles + 1, np.int64)
    np.cumsum(np.bincount(tile, minlength=ntiles), out=tile_ptr[1:])
    return items.astype(np.int32), tile_ptr.astype(np.int32)


def tables(polys, H, W, ids=None, top="first", img=None, nimg=None):
    """edge_table and tile_lists in one step -> (edges, items, tile_ptr, nimg)"""
    if not isinstance(polys, Polygons):
        raise KGLibraryError("fill: a Polygons")
    values, rows, pimg, nimg = _per_part("fill", polys, ids, img, nimg)
    edges, ranges, boxes = edge_table(polys)
    items, tile_ptr = tile_lists(ranges, boxes, values, rows, H, W, pimg, nimg, top)
    return edges, items, tile_ptr, nimg


# ---- host statement of the rule ---------------------------------------------------------------------------------------------------------------

def _parity(e, y1, x1, y2, x2):
    """e: int64 [n, 4] edges; the half-open pixel box -> bool [y2 - y1, x2 - x1]: the number of counting edges of every centre is odd"""
    h, w = y2 - y1, x2 - x1
    out = np.zeros((h, w), bool)
    if len(e) == 0 or h <= 0 or w <= 0:
        return out
    cx = (F * np.arange(x1, x2, dtype=np.int64) + F // 2)[None, :, None]
    eb = max(1, min(len(e), 2 ** 20 // w))
    hb = max(1, 2 ** 20 // (w * eb))
    for r0 in range(0, h, hb):
        cy = (F * np.arange(y1 + r0, min(y1 + r0 + hb, y2), dtype=np.int64) + F // 2)[:, None, None]
        for e0 in range(0, len(e), eb):
            x0, y0, xe, ye = (e[e0:e0 + eb, c][None, None, :] for c in range(4))
            hit = (y0 <= cy) & (cy < ye) & ((xe - x0) * (cy - y0) > (cx - x0) * (ye - y0))
            out[r0:r0 + hb] ^= (hit.sum(-1) & 1).astype(bool)
    return out


def fill_host(polys, H, W, ids=None, background=0, top="first", cover=False, img=None, nimg=None):
    """The rule in plain NumPy: per pixel the crossing count over all the edges of a part, no tiles and no bins (a part is evaluated on
    the pixel box of edge_table only: outside it every count is 0 or even) -> int32 [H, W], or [nimg, H, W] when img, the image index of
    every row, is given (nimg: default its largest entry + 1).  ids: the int32 value of every row, default 1 .. m.  cover=True:
    -> (out, cover), cover int32 of the same shape.  The yardstick of fill."""
    if not isinstance(polys, Polygons):
        raise KGLibraryError("fill_host: a Polygons")
    values, rows, pimg, n_img = _per_part("fill_host", polys, ids, img, nimg)
    n_img, H, W = _sizes("fill_host", n_img, H, W)
    background = _int32("fill_host", "background", background)
    edges, ranges, boxes = edge_table(polys)
    e64 = edges.astype(np.int64)
    out = np.full((n_img, H, W), background, np.int32)
    has = np.zeros((n_img, H, W), bool)
    cov = np.zeros((n_img, H, W), np.int32)
    m = len(polys)
    for k in (range(m - 1, -1, -1) if _top("fill_host", top) else range(m)):
        p0, p1 = int(polys.part_ptr[k]), int(polys.part_ptr[k + 1])
        live = [p for p in range(p0, p1) if ranges[p, 1] > 0]
        if not live:
            continue
        b = boxes[live]
        y1, x1, y2, x2 = max(int(b[:, 0].min()), 0), max(int(b[:, 1].min()), 0), min(int(b[:, 2].max()), H), min(int(b[:, 3].max()), W)
        if y2 <= y1 or x2 <= x1:
            continue
        covered = np.zeros((y2 - y1, x2 - x1), bool)
        for p in live:
            py1, px1, py2, px2 = max(int(boxes[p, 0]), y1), max(int(boxes[p, 1]), x1), min(int(boxes[p, 2]), y2), min(int(boxes[p, 3]), x2)
            if py2 > py1 and px2 > px1:
                covered[py1 - y1:py2 - y1, px1 - x1:px2 - x1] |= _parity(e64[ranges[p, 0]:ranges[p, 0] + ranges[p, 1]], py1, px1, py2, px2)
        i = int(pimg[p0])
        o, hs = out[i, y1:y2, x1:x2], has[i, y1:y2, x1:x2]
        o[covered & ~hs] = values[p0]
        hs |= covered
        cov[i, y1:y2, x1:x2] += covered
    if img is None:
        out, cov = out[0], cov[0]
    return (out, cov) if cover else out


def fill_tables_host(edges, items, tile_ptr, nimg, H, W, background=0):
    """kg_polygons_fill stated in NumPy for ANY tables, wrong ones included (the clamped tile range, the predicates that empty an item)
    -> (out, cover) int32 [nimg, H, W].  Edge coordinates must lie in the fixed-point range."""
    nimg, H, W = _sizes("fill_tables_host", nimg, H, W)
    edges, items = np.asarray(edges, np.int64).reshape(-1, 4), np.asarray(items, np.int64).reshape(-1, 4)
    tile_ptr = np.asarray(tile_ptr, np.int64).reshape(-1)
    E, n = len(edges), len(items)
    ty_n, tx_n = _ceil_div(H, TILE_H), _ceil_div(W, TILE_W)
    if len(tile_ptr) != nimg * ty_n * tx_n + 1:
        raise KGLibraryError(f"fill_tables_host: tile_ptr of {len(tile_ptr)} entries for {nimg * ty_n * tx_n} tiles")
    out = np.full((nimg, H, W), _int32("fill_tables_host", "background", background), np.int32)
    cov = np.zeros((nimg, H, W), np.int32)
    for t in range(nimg * ty_n * tx_n):
        i, rest = divmod(t, ty_n * tx_n)
        ty, tx = divmod(rest, tx_n)
        y1, x1, y2, x2 = ty * TILE_H, tx * TILE_W, min((ty + 1) * TILE_H, H), min((tx + 1) * TILE_W, W)
        lo, hi = (min(max(int(v), 0), n) for v in tile_ptr[t:t + 2])
        has = np.zeros((y2 - y1, x2 - x1), bool)
        last = np.zeros((y2 - y1, x2 - x1), np.int64)
        o, c = out[i, y1:y2, x1:x2], cov[i, y1:y2, x1:x2]
        for value, first, count, row in items[lo:max(lo, hi)].tolist():
            if not (0 <= first <= E and 0 <= count <= E - first):
                continue
            odd = _parity(edges[first:first + count], y1, x1, y2, x2)
            o[odd & ~has] = value
            has |= odd
            counts = odd & ((c == 0) | (last != row))
            c += counts
            last[counts] = row
    return out, cov


# ---- device -------------------------------------------------------------------------------------------------------------------------------

def _int32(fn, what, v):
    if isinstance(v, (bool, np.bool_)) or not -2 ** 31 <= int(v) <= 2 ** 31 - 1:
        raise KGLibraryError(f"{fn}: {what} {v!r} must fit int32")
    return int(v)


def _table(fn, what, t, ncol, dev):
    import torch
    ok = torch.is_tensor(t) and t.dtype == torch.int32 and t.is_contiguous() and (dev is None or t.device == dev) and t.device.type == "cuda"
    if not ok or (ncol and (t.dim() != 2 or t.shape[1] != ncol)) or (not ncol and t.dim() != 1):
        raise KGLibraryError(f"{fn}: {what} must be a contiguous device int32 tensor {'[n, %d]' % ncol if ncol else '[nimg * tiles + 1]'} on one device")
    return t


def fill_tables(edges, items, tile_ptr, nimg, H, W, background=0, out=None, cover=None):
    """kg_polygons_fill as it is: edges device int32 [E, 4], items device int32 [n, 4] = {value, edge_first, edge_count, row}, tile_ptr
    device int32 [nimg * tiles + 1] -> out device int32 [nimg, H, W], or (out, cover) when cover is True or a tensor.  out / cover: None
    (tensors are made) or contiguous device int32 [nimg, H, W] tensors written in place.  One launch, no copy back, no
    synchronisation."""
    import torch
    from ._lib import ptr, stream_ptr
    fn = "fill_tables"
    tile_ptr = _table(fn, "tile_ptr", tile_ptr, 0, None)
    dev = tile_ptr.device
    edges, items = _table(fn, "edges", edges, 4, dev), _table(fn, "items", items, 4, dev)
    nimg, H, W = _sizes(fn, nimg, H, W)
    if tile_ptr.numel() != nimg * _ceil_div(H, TILE_H) * _ceil_div(W, TILE_W) + 1:
        raise KGLibraryError(f"{fn}: tile_ptr of {tile_ptr.numel()} entries for {nimg} x {_ceil_div(H, TILE_H)} x {_ceil_div(W, TILE_W)} tiles")
    background = _int32(fn, "background", background)

    def made(t, what):
        if t is None or t is True:
            return torch.empty(nimg, H, W, dtype=torch.int32, device=dev)
        if not is_device(t) or t.dtype != torch.int32 or tuple(t.shape) != (nimg, H, W) or t.device != dev or not t.is_contiguous():
            raise KGLibraryError(f"{fn}: {what} must be a contiguous int32 [{nimg}, {H}, {W}] tensor on the tables' device")
        return t
    out = made(out, "out")
    cov = None if cover is None or cover is False else made(cover, "cover")
    E, n = edges.shape[0], items.shape[0]
    with torch.cuda.device(dev):
        _lib.call("kg_polygons_fill", ptr(edges) if E else None, E, ptr(items) if n else None, n, ptr(tile_ptr), nimg, H, W, background, ptr(out),
                  ptr(cov), stream_ptr())
    return out if cov is None else (out, cov)


def upload_tables(edges, items, tile_ptr, device):
    """The three host tables -> three device int32 views of ONE uploaded buffer (edges first, then items, then tile_ptr: the two tables of
    16-byte rows stay 16-byte aligned)."""
    from . import ops
    E, n = len(edges), len(items)
    buf = np.concatenate([np.ascontiguousarray(edges, np.int32).reshape(-1), np.ascontiguousarray(items, np.int32).reshape(-1),
                          np.ascontiguousarray(tile_ptr, np.int32).reshape(-1)])
    d = ops.h2d(buf, device)
    return d[:4 * E].view(E, 4), d[4 * E:4 * (E + n)].view(n, 4), d[4 * (E + n):]


def fill(polys, H, W, device, ids=None, background=0, top="first", cover=False, img=None, nimg=None):
    """fill_host on the device -> device int32 [H, W] ([nimg, H, W] when img is given), or (out, cover).  The host builds the edge table
    and the tile lists (edge_table, tile_lists); the three tables go up in one buffer, ONE kg_polygons_fill launch, no copy back and no
    synchronisation: polygon ground truth reaches labelmetrics.LabelEvaluator without a host label map."""
    import torch
    dev = torch.device(device)
    if dev.type != "cuda":
        raise KGLibraryError("fill (MI355X build) needs a GPU device; the host route is fill_host")
    background = _int32("fill", "background", background)
    edges, items, tile_ptr, n_img = tables(polys, H, W, ids, top, img, nimg)
    de, di, dp = upload_tables(edges, items, tile_ptr, dev)
    got = fill_tables(de, di, dp, n_img, H, W, background, cover=True if cover else None)
    if img is None:
        got = (got[0][0], got[1][0]) if cover else got[0]
    return got
