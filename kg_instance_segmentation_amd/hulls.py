"""Convex hulls on the device: the hull ring of every instance of a label map, and what morphometry reads from it.

Solidity (area / convex area: the irregularity and "two nuclei merged" flag), the maximum and minimum Feret (caliper) diameter and the
hull perimeter (convexity = hull perimeter / outline perimeter, with measure.py's perimeter) are all functions of the convex hull; the
hull polygon is also the compact ROI that COCO and GeoJSON tools take when the full outline (contours.py) is too heavy.  Here the device
builds the hull of every instance (kg_label_hulls, csrc/hulls.hip), the rows and the rings come back instead of the map, and the host
builds a CSR structure over them.

    hulls_host       the statement below in NumPy / Python integers, never size-limited: the yardstick
    hull_rows        kg_label_hulls as it is: ONE launch, everything stays on the device
    hulls            hulls_host from a device map: one upload, ONE launch, one copy back; large jobs are banded, never traced on the host
    band_jobs        the pieces of the jobs: at most max_job_pixels pixels and at most MAX_ROWS rows each
    merge_bands      the hull of a union is the hull of the hulls: the pieces' rows -> the jobs' rows
    Hulls            host CSR over the jobs: ptr, verts, rows; of(k), solidity(), feret_max(), feret_min(), props(), coco(k), ...
    hulls_instances  hulls for an Instances / TiledInstances (ids 1 .. n, boxes from its table)

Semantics (include/kgnet_hip.h is the normative text)
  job         {img, id, y1, x1, y2, x2}: a half-open box, clamped to the map.  P = the pixels of the box in image img with labels == id.
              Values are compared only: any int32 is an id.  H, W <= 32768.
  lattice     as in contours: pixel (y, x) is the square between vertices (y, x) and (y + 1, x + 1); C(P) = the four corners of every
              pixel of P.
  hull        the convex hull of C(P) as a ring of its STRICT vertices: no vertex lies on the segment between its neighbours.
  ring order  clockwise on the screen, area2 = sum of x_i * y_(i+1) - x_(i+1) * y_i > 0 (the sign of an outer ring of contours), from the
              vertex with the smallest (Y, X) in raster order; the closing vertex is not repeated; absolute (Y, X), int32.
  extent form L(Y) / R(Y) = the smallest / largest X of a corner of C(P) on lattice line Y, defined where box row Y - 1 or Y holds a pixel
              of P.  The ring is (top, L(top)), the vertices of the upper concave envelope of R from top to bottom, the vertices of the
              lower convex envelope of L from bottom to top without the start; (Y_i, F_i) is a strict envelope vertex iff for all defined
              j < i < k: (Y_i - Y_j)(F_k - F_i) - (Y_k - Y_i)(F_i - F_j) > 0 for L, < 0 for R (extent_ring; the device builds this).
  row         int64 [10] = ROW_COLUMNS.  area = |P|; count = ring vertices (>= 4); area2 = twice the hull's area; feret_max2 = the largest
              squared distance between two ring vertices, (fmax_i, fmax_j), i < j, its ring indices, a tie to the lexicographically
              smallest pair.  For edge k (vertex k to k + 1, cyclic) c_k = max over the vertices u of |cross(v_(k+1) - v_k, u - v_k)|,
              d_k = |v_(k+1) - v_k|^2; the squared minimum caliper width is min_k c_k^2 / d_k: minw_num = c_k, minw_den2 = d_k,
              minw_edge = k of the minimum, edges compared exactly by c_a^2 d_b < c_b^2 d_a (up to 2^93: 128 bits on the device, Python
              integers here), a tie to the smallest k.
  status      0 ok; 1 the clamped box is taller than MAX_ROWS (zero row; hulls never produces it); 2 the slab of the table is smaller
              than count (right statistics, only the first cap vertices stored).
  bad jobs    an image index outside [0, nimg), an empty or inverted box, an id the box does not hold: a row of zeros, no vertices.
  bands       a job is cut into pieces of at most max_job_pixels pixels and MAX_ROWS rows (labelmetrics.split_jobs, then by rows); the
              areas add, the ring is the hull (the same monotone chain) of the pieces' ring vertices, the other columns are recomputed
              from the merged ring by the function hulls_host uses (ring_row)."""
import numpy as np

from . import _lib, _labelmaps, labelmetrics
from ._labelmaps import JOB_COLUMNS as _JOB_COLUMNS, MAX_SIDE, device_stack, host_stack, out_tensor  # noqa: F401  (MAX_SIDE: public here)

KGLibraryError = _lib.KGLibraryError
MAX_ROWS = 4095                                                        # rows of a box the device takes: 4096 lattice lines in LDS
ROW_COLUMNS = ("area", "count", "area2", "feret_max2", "fmax_i", "fmax_j", "minw_num", "minw_den2", "minw_edge", "status")
_ROW_JOB_COLUMNS = "(img, id, y1, x1, y2, x2, vert_at, cap)"


class Hulls:
    """Host CSR over the jobs (or the instances): row k owns the ring verts[ptr[k] : ptr[k + 1]] as (y, x), int32, and rows[k], int64
    [10] (ROW_COLUMNS).  An empty job has an empty ring and a row of zeros."""
    __slots__ = ("ptr", "verts", "rows")

    def __init__(self, ptr, verts, rows):
        self.ptr = np.ascontiguousarray(ptr, np.int64).reshape(-1)
        self.verts = np.ascontiguousarray(verts, np.int32).reshape(-1, 2)
        self.rows = np.ascontiguousarray(rows, np.int64).reshape(-1, 10)
        p = self.ptr
        if len(p) != len(self.rows) + 1 or p[0] != 0 or p[-1] != len(self.verts) or not np.array_equal(np.diff(p), self.rows[:, 1]):
            raise KGLibraryError(f"Hulls: ptr of {len(p)} entries for {len(self.rows)} rows and {len(self.verts)} vertices does not follow the counts")

    def __len__(self):
        return len(self.rows)

    def __eq__(self, other):
        return isinstance(other, Hulls) and all(np.array_equal(getattr(self, k), getattr(other, k)) for k in self.__slots__)

    __hash__ = None

    def of(self, k):
        """int32 [count, 2] of (y, x): the ring of row k"""
        return self.verts[int(self.ptr[k]):int(self.ptr[k + 1])]

    def slice(self, r0, r1):
        """The Hulls of rows r0 .. r1 - 1"""
        a, b = int(self.ptr[r0]), int(self.ptr[r1])
        return Hulls(self.ptr[r0:r1 + 1] - a, self.verts[a:b], self.rows[r0:r1])

    def _nan_empty(self, v):
        return np.where(self.rows[:, 0] > 0, v, np.nan)

    def areas(self):
        """int64 [m]: the pixels of every row"""
        return self.rows[:, 0].copy()

    def convex_areas(self):
        """float64 [m]: the area of the hull, area2 / 2"""
        return self.rows[:, 2] / 2.0

    def solidity(self):
        """float64 [m]: area / convex area, in (0, 1]; NaN for an empty row"""
        with np.errstate(invalid="ignore", divide="ignore"):
            return self._nan_empty(2.0 * self.rows[:, 0] / self.rows[:, 2])

    def feret_max(self):
        """float64 [m]: the largest distance between two hull vertices; NaN for an empty row"""
        return self._nan_empty(np.sqrt(self.rows[:, 3].astype(np.float64)))

    def feret_min(self):
        """float64 [m]: the minimum caliper width, minw_num / sqrt(minw_den2); NaN for an empty row"""
        with np.errstate(invalid="ignore", divide="ignore"):
            return self._nan_empty(self.rows[:, 6] / np.sqrt(self.rows[:, 7].astype(np.float64)))

    def feret_max_points(self):
        """int32 [m, 2, 2]: the two vertices (y, x) of the maximum Feret diameter; zeros for an empty row"""
        out = np.zeros((len(self), 2, 2), np.int32)
        k = np.flatnonzero(self.rows[:, 1] > 0)
        out[k, 0] = self.verts[self.ptr[k] + self.rows[k, 4]]
        out[k, 1] = self.verts[self.ptr[k] + self.rows[k, 5]]
        return out

    def perimeters(self):
        """float64 [m]: the length of the hull's boundary, the sum of its edge lengths; 0 for an empty row"""
        out = np.zeros(len(self), np.float64)
        if len(self.verts):
            v = self.verts.astype(np.float64)
            nxt = np.arange(1, len(v) + 1)
            last = self.ptr[1:][self.rows[:, 1] > 0] - 1                 # the last vertex of a ring closes to its first
            nxt[last] = self.ptr[:-1][self.rows[:, 1] > 0]
            np.add.at(out, np.repeat(np.arange(len(self)), self.rows[:, 1]), np.hypot(*(v[nxt] - v).T))
        return out

    def props(self):
        """dict of float64 arrays [m], from the integers only: area, convex_area, solidity, feret_max, feret_min, convex_perimeter,
        vertices.  It stands next to measure.Measurements.props(): convexity is convex_perimeter / that dict's perimeter.  A row with
        area == 0 gets NaN everywhere but area and vertices."""
        return {"area": self.rows[:, 0].astype(np.float64), "convex_area": self._nan_empty(self.convex_areas()), "solidity": self.solidity(),
                "feret_max": self.feret_max(), "feret_min": self.feret_min(), "convex_perimeter": self._nan_empty(self.perimeters()),
                "vertices": self.rows[:, 1].astype(np.float64)}

    def coco(self, k):
        """COCO's `segmentation` polygons of row k: one flat [x0, y0, x1, y1, ...] list, none for an empty row"""
        r = self.of(k)
        return [r[:, ::-1].reshape(-1).tolist()] if len(r) else []

    def geojson(self, k):
        """A GeoJSON Polygon of row k in pixel coordinates [x, y]: one closed ring (its first position repeated) in ring order; no
        coordinates for an empty row"""
        v = self.of(k)[:, ::-1].tolist()
        return {"type": "Polygon", "coordinates": [v + v[:1]] if v else []}

    def to_polygons(self):
        """polygons.Polygons, one row of one part of one ring per row (an empty row has no part): polygons.fill of it paints the convex
        image of every instance"""
        from . import polygons
        return polygons.from_rings([[[self.of(k)[:, ::-1]]] if self.rows[k, 1] else [] for k in range(len(self))])


def _assemble(per_job):
    """per_job: one (row int64 [10], ring [count, 2]) per job -> Hulls"""
    ptr = np.zeros(len(per_job) + 1, np.int64)
    np.cumsum([len(p[1]) for p in per_job], out=ptr[1:])
    rows = np.array([p[0] for p in per_job], np.int64).reshape(-1, 10)
    rings = [np.asarray(p[1], np.int32).reshape(-1, 2) for p in per_job]
    return Hulls(ptr, np.concatenate(rings) if rings else np.zeros((0, 2), np.int32), rows)


# ---- host statement of the semantics ------------------------------------------------------------------------------------------------------

_NONE = (np.zeros(10, np.int64), np.zeros((0, 2), np.int32))


def chain(points):
    """Andrew's monotone chain: lattice points [n, 2] of (Y, X), not all on one line -> the strict hull vertices as a list of (Y, X),
    clockwise on the screen from the smallest (Y, X).  Python integers throughout."""
    pts = sorted(set(map(tuple, np.asarray(points, np.int64).reshape(-1, 2).tolist())))

    def half(seq):
        st = []
        for p in seq:                                                  # keep a strict turn of the ring's sign, drop the rest
            while len(st) >= 2 and (st[-1][1] - st[-2][1]) * (p[0] - st[-2][0]) - (st[-1][0] - st[-2][0]) * (p[1] - st[-2][1]) <= 0:
                st.pop()
            st.append(p)
        return st
    return half(pts)[:-1] + half(pts[::-1])[:-1]                       # the right chain downwards, then the left chain upwards


def _boundary_corners(me, y1, x1):
    """me: bool [h, w] at (y1, x1) -> int64 [n, 2]: the corners of C(P) that 1 to 3 pixels of P touch.  A corner that four pixels of P
    touch lies inside the union of their squares, hence strictly inside the hull: leaving it out changes no vertex."""
    h, w = me.shape
    m = np.zeros((h + 2, w + 2), np.int8)
    m[1:-1, 1:-1] = me
    cnt = m[:-1, :-1] + m[:-1, 1:] + m[1:, :-1] + m[1:, 1:]
    Y, X = np.nonzero((cnt > 0) & (cnt < 4))
    return np.stack([Y + y1, X + x1], 1).astype(np.int64)


def ring_row(ring, area=0):
    """ring: the hull vertices [count, 2] of (Y, X) in ring order -> the row int64 [10] with the given area and status 0: the shoelace
    sum, the farthest pair and the narrowest edge by their definitions, over all pairs; the edges are compared in Python integers."""
    v = np.asarray(ring, np.int64).reshape(-1, 2)
    n = len(v)
    if n == 0:
        return np.zeros(10, np.int64)
    y, x = v[:, 0], v[:, 1]
    yn, xn = np.roll(y, -1), np.roll(x, -1)
    area2 = int((x * yn - xn * y).sum())
    best = (-1, 0, 0)
    cmax = np.zeros(n, np.int64)
    step = max(1, 2 ** 21 // n)
    for i0 in range(0, n, step):
        sl = slice(i0, min(i0 + step, n))
        dy, dx = y[None, :] - y[sl, None], x[None, :] - x[sl, None]
        d2 = dy * dy + dx * dx
        d2[np.arange(n)[None, :] <= np.arange(i0, sl.stop)[:, None]] = -1          # pairs (i, j) with i < j only
        at = int(d2.argmax())                                          # the first in row-major order: the smallest (i, j) of a tie
        if d2.reshape(-1)[at] > best[0]:
            best = (int(d2.reshape(-1)[at]), i0 + at // n, at % n)
        cmax[sl] = np.abs((xn[sl] - x[sl])[:, None] * dy - (yn[sl] - y[sl])[:, None] * dx).max(1)
    dk = ((yn - y) ** 2 + (xn - x) ** 2).tolist()
    ck = cmax.tolist()
    k = 0
    for e in range(1, n):
        if ck[e] * ck[e] * dk[k] < ck[k] * ck[k] * dk[e]:              # Python integers: the products reach 2^93
            k = e
    return np.array([area, n, area2, best[0], best[1], best[2], ck[k], dk[k], k, 0], np.int64)


def _job_hull(lab, H, W, job):
    """One map [H, W], one job (id, y1, x1, y2, x2) -> (row, ring)"""
    v, y1, x1, y2, x2 = job
    y1, x1, y2, x2 = max(y1, 0), max(x1, 0), min(y2, H), min(x2, W)
    if y2 <= y1 or x2 <= x1:
        return _NONE
    me = lab[y1:y2, x1:x2] == v
    area = int(np.count_nonzero(me))
    if area == 0:
        return _NONE
    ring = np.array(chain(_boundary_corners(me, y1, x1)), np.int32)
    return ring_row(ring, area), ring


def extent_ring(me, y1=0, x1=0):
    """The extent form of the semantics for a mask me: bool [h, w] at (y1, x1), by its definition (every triple of defined lines) ->
    int64 [count, 2].  What the device builds; hulls_host does not come this way, so the two check each other."""
    me = np.asarray(me, bool)
    rows = np.flatnonzero(me.any(1))
    if len(rows) == 0:
        return np.zeros((0, 2), np.int64)
    first = me.argmax(1)
    last = me.shape[1] - me[:, ::-1].argmax(1)
    L, R = {}, {}
    for r in rows.tolist():
        for Y in (r, r + 1):
            L[Y] = min(L.get(Y, first[r]), first[r]); R[Y] = max(R.get(Y, last[r]), last[r])
    Ys = sorted(L)

    def strict(F, sign):
        out = []
        for a, Yi in enumerate(Ys):
            if all(sign * ((Yi - Yj) * (F[Yk] - F[Yi]) - (Yk - Yi) * (F[Yi] - F[Yj])) > 0 for Yj in Ys[:a] for Yk in Ys[a + 1:]):
                out.append((Yi + y1, int(F[Yi]) + x1))
        return out
    left, right = strict(L, 1), strict(R, -1)
    return np.array(left[:1] + right + left[:0:-1], np.int64)


def hulls_host(labels, jobs_or_n):
    """labels: integers [H, W] or [nimg, H, W]; jobs_or_n: jobs [m, 6] = (img, id, y1, x1, y2, x2), or the instance count n (one per map
    for a stack): the ids 1 .. n inside their own boxes (labelmetrics.label_stats_host) -> Hulls, one row per job.  The ring is the
    monotone chain over the corners C(P) themselves, not the extent form.  Never size-limited."""
    maps = host_stack("hulls_host", labels)
    nimg, H, W = maps.shape
    j = _labelmaps.host_job_table("hulls_host", maps, jobs_or_n, labelmetrics.label_stats_host)
    return _assemble([_job_hull(maps[i], H, W, rest) if 0 <= i < nimg else _NONE for i, *rest in j.tolist()])


# ---- bands --------------------------------------------------------------------------------------------------------------------------------

def band_jobs(jobs, max_job_pixels=65536, max_rows=MAX_ROWS):
    """Jobs int [m, 6] -> (pieces int32 [m2, 6], owner int64 [m2]): labelmetrics.split_jobs, then any piece taller than max_rows cut by
    rows.  The pieces of a job tile its box and lie together, in the order of the jobs."""
    max_rows = int(max_rows)
    if max_rows < 1:
        raise KGLibraryError(f"band_jobs: max_rows {max_rows}")
    pieces, owner = labelmetrics.split_jobs(jobs, max_job_pixels)
    p = pieces.astype(np.int64)
    parts = np.maximum(-(-(p[:, 4] - p[:, 2]) // max_rows), 1)         # an empty or inverted box stays one piece
    if (parts == 1).all():
        return pieces, owner
    rep = np.repeat(np.arange(len(p)), parts)
    k = np.arange(len(rep)) - np.repeat(np.cumsum(parts) - parts, parts)
    out = p[rep]
    out[:, 2] = p[rep, 2] + k * max_rows
    out[:, 4] = np.where(parts[rep] > 1, np.minimum(out[:, 2] + max_rows, p[rep, 4]), p[rep, 4])
    return np.ascontiguousarray(out.astype(np.int32)), owner[rep]


def merge_bands(pieces, owner, m):
    """pieces: the Hulls of band_jobs' pieces; owner int64, non-decreasing; m jobs -> the Hulls of the jobs: the areas add, the ring is
    the chain of the pieces' ring vertices, the other columns are ring_row's.  A job of one piece keeps its row as it is."""
    owner = np.asarray(owner, np.int64).reshape(-1)
    if len(owner) != len(pieces) or (len(owner) and ((np.diff(owner) < 0).any() or owner[0] < 0 or owner[-1] >= m)):
        raise KGLibraryError(f"merge_bands: {len(owner)} owners for {len(pieces)} pieces of {m} jobs")
    if len(owner) == m and np.array_equal(owner, np.arange(m)):
        return pieces
    start = np.searchsorted(owner, np.arange(m + 1))
    per = []
    for k in range(m):
        a, b = int(start[k]), int(start[k + 1])
        if b - a == 1:
            per.append((pieces.rows[a], pieces.of(a)))
            continue
        area = int(pieces.rows[a:b, 0].sum())
        if area == 0:
            per.append(_NONE)
            continue
        ring = np.array(chain(pieces.verts[int(pieces.ptr[a]):int(pieces.ptr[b])]), np.int32)
        per.append((ring_row(ring, area), ring))
    return _assemble(per)


# ---- device -----------------------------------------------------------------------------------------------------------------------------

def hull_rows(labels, jobs, V, rows=None, verts=None):
    """kg_label_hulls as it is: labels device int32 [H, W] or [nimg, H, W]; jobs host integers [m, 8] = (img, id, y1, x1, y2, x2, vert_at,
    cap) (uploaded once) or a device int32 tensor -> (rows device int64 [m, 10] = ROW_COLUMNS, verts device int32 [V, 2] = (y, x)).
    rows / verts: None (tensors of zeros are made) or contiguous device tensors written in place: every row is written, and only the
    vertex slots the table names change.  One launch, no copy back, no synchronisation."""
    import torch
    from ._lib import ptr, stream_ptr
    lab = device_stack("hull_rows", labels)[0]
    nimg, H, W = lab.shape
    jd = _labelmaps.device_jobs("hull_rows", jobs, 8, _ROW_JOB_COLUMNS, lab.device)
    m = jd.shape[0]
    V = int(V)
    if not 0 <= V <= 2 ** 31 - 1:
        raise KGLibraryError(f"hull_rows: V {V}")
    rows = torch.zeros(m, 10, dtype=torch.int64, device=lab.device) if rows is None else out_tensor("hull_rows", "rows", rows, (m, 10), torch.int64, lab.device)
    verts = torch.zeros(V, 2, dtype=torch.int32, device=lab.device) if verts is None else out_tensor("hull_rows", "verts", verts, (V, 2), torch.int32, lab.device)
    with torch.cuda.device(lab.device):
        _lib.call("kg_label_hulls", ptr(lab), nimg, H, W, ptr(jd) if m else None, m, ptr(rows) if m else None, ptr(verts) if V else None, V,
                  stream_ptr())
    return rows, verts


def _device_hulls(lab, j, max_job_pixels):
    """lab: device int32 [nimg, H, W], j: host jobs [m, 6], clamped -> Hulls.  One upload, one launch, one copy back."""
    import torch
    m = len(j)
    if m == 0:
        return _assemble([])
    pieces, owner = band_jobs(j, max_job_pixels)
    p = pieces.astype(np.int64)
    h, w = p[:, 4] - p[:, 2], p[:, 5] - p[:, 3]
    cap = np.where((h > 0) & (w > 0), 2 * (h + 1), 0)                  # one L and one R per lattice line: a slab cannot overflow
    at = np.cumsum(cap) - cap
    mp, V = len(p), int(cap.sum())
    if V > 2 ** 31 - 1:
        raise KGLibraryError(f"hulls: slabs of {V} vertices exceed 2^31 - 1")
    buf = torch.empty(80 * mp + 8 * V, dtype=torch.uint8, device=lab.device)                 # both outputs in one buffer: one copy back
    hull_rows(lab, np.concatenate([p, at[:, None], cap[:, None]], 1), V, buf[:80 * mp].view(torch.int64).view(mp, 10),
              buf[80 * mp:].view(torch.int32).view(V, 2))
    host = buf.cpu().numpy()
    rows, slabs = host[:80 * mp].view(np.int64).reshape(mp, 10), host[80 * mp:].view(np.int32).reshape(V, 2)
    count = rows[:, 1]
    if (rows[:, :2] < 0).any() or (count > cap).any() or rows[:, 9].any() or ((count > 0) != (rows[:, 0] > 0)).any():
        raise KGLibraryError("hulls: rows that are no rows")
    ptr = np.zeros(mp + 1, np.int64)
    np.cumsum(count, out=ptr[1:])
    take = np.repeat(at - ptr[:-1], count) + np.arange(int(ptr[-1]))   # the filled head of every slab
    return merge_bands(Hulls(ptr, slabs[take], rows), owner, m)


def hulls(labels, n=None, jobs=None, stats=None, max_job_pixels=65536):
    """hulls_host on the device -> Hulls (host).  labels: device int32 [H, W] or [nimg, H, W].  What is taken:
      jobs   host integers [m, 6] = (img, id, y1, x1, y2, x2): one row per job; or
      n      the instance count (one per map for a stack): the ids 1 .. n inside their own boxes.  The boxes come from stats -- host
             integers [n, 5] = (area, y1, x1, y2, x2), one array per map for a stack -- or, without stats, from labelmetrics.label_stats.
    The jobs are cut into pieces (band_jobs), every piece gets a slab of 2 * (h + 1) vertices; one upload, ONE kg_label_hulls launch, one
    copy back of rows and slabs in one buffer; the host compacts the slabs and merges the pieces of a job (merge_bands).  No job is
    traced on the host."""
    lab = device_stack("hulls", labels)[0]
    return _device_hulls(lab, _labelmaps.job_table("hulls", lab, n, jobs, stats, labelmetrics.label_stats), max_job_pixels)


# ---- Instances ----------------------------------------------------------------------------------------------------------------------------

def _instance_hulls(insts, max_job_pixels=65536):
    """-> one Hulls per entry (None for a None entry); the entries themselves are not touched"""
    out = [None] * len(insts)

    def host_one(i, inst, lab):
        out[i] = hulls_host(lab, _labelmaps.instance_jobs(inst, 0, 0, *lab.shape))
    for idx, stack, H, W in _labelmaps.size_batches("hulls_instances", insts, host_one):
        got = _device_hulls(device_stack("hulls_instances", stack)[0], _labelmaps.batch_jobs(insts, idx, 0, H, W), max_job_pixels)
        for i, a, b in _labelmaps.deal(insts, idx):
            out[i] = got.slice(a, b)
    return out


def hulls_instances(inst, max_job_pixels=65536):
    """hulls for an Instances / TiledInstances -> Hulls with len(inst) rows: ids 1 .. n, boxes from table[:, 2:6]; an instance with no
    visible pixel gets an empty row.  A host label map (assemble_host's result) goes through hulls_host."""
    return _instance_hulls([inst], max_job_pixels)[0]


def hulls_instances_batch(insts, max_job_pixels=65536):
    """hulls_instances for predict_instances' list (entries may be None), in place: every entry's `hulls` is set.  ONE launch per
    output size."""
    for v, g in zip(insts, _instance_hulls(insts, max_job_pixels)):
        if v is not None:
            v.hulls = g
    return insts
