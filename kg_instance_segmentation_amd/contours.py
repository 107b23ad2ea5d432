"""Instance outlines on the device: the polygon rings of every instance of a label map.

COCO `segmentation` polygons, GeoJSON / QuPath / napari ROIs and every outline overlay take an instance as polygons.  Here the device
traces the outline of every instance (kg_label_contour_counts, kg_label_contours, csrc/contours.hip), the rings and their vertices come
back instead of the map, and the host builds a CSR structure over them.

    contours_host      the statement below in NumPy / Python, never size-limited: the yardstick
    contour_counts     kg_label_contour_counts as it is: ONE launch, rows stay on the device
    contour_rows       kg_label_contours as it is: ONE launch, rows stay on the device
    contours           contours_host from a device map: one count launch, a host prefix, one write launch; a job too large for the device
                       is traced on the host from its box copied back
    fits               the size rule of the device route
    Contours           host CSR over the jobs: ring_ptr, first, count, perimeter, area2, verts; of(k), coco(k), geojson(k), areas(), ...
    contours_instances contours for an Instances / TiledInstances (ids 1 .. n, boxes from its table)

Semantics (include/kgnet_hip.h is the normative text)
  job         {img, id, y1, x1, y2, x2}: a half-open box, clamped to the map.  P = the pixels of the box in image img with labels == id;
              everything else is non-P, the same id outside the box included.  Values are compared only: any int32 is an id.
  lattice     vertices (Y, X), 0 <= Y <= H, 0 <= X <= W; pixel (y, x) is the square between (y, x) and (y + 1, x + 1).
  cracks      a directed crack leaves a vertex E (x + 1) = 0, S (y + 1) = 1, W (x - 1) = 2 or N (y - 1) = 3 with P on its right and non-P
              on its left.  With m(y, x) = "in P" (false outside the box), at (Y, X):
                  E iff m(Y, X) && !m(Y - 1, X)            S iff m(Y, X - 1) && !m(Y, X)
                  W iff m(Y - 1, X - 1) && !m(Y, X - 1)    N iff m(Y - 1, X) && !m(Y - 1, X - 1)
  successor   of a crack arriving at V with direction d: the first existing crack leaving V among right turn (d + 1) & 3, straight d,
              left turn (d + 3) & 3.  Right first makes P 4-connected: pixels that meet only at a corner get separate rings.
  rings       the cracks fall into disjoint cycles.  The vertices of a ring are where the direction changes.  An outer boundary runs
              clockwise on the screen (positive area2), a hole the other way (negative).  A ring may visit a vertex twice (a pinch).
  start       a candidate is an E crack at (Y, X) with no E crack at (Y, X - 1).  The start of a ring is its candidate with the smallest
              (Y, X) in raster order; the vertex list begins there and follows the traversal; the closing vertex is not repeated.
  order       the rings of a job by start (Y, X) in raster order.
  per ring    count (vertices: even, >= 4), perimeter (cracks), area2 = sum of x_i * y_(i+1) - x_(i+1) * y_i (int64).  Coordinates are
              absolute (Y, X), int32.
  bad jobs    an image index outside [0, nimg), an empty or inverted box, an id the box does not hold: zero rings.
  size        the device traces a job whose clamped h x w box has (h + 2) * 32 * (ceil((w + 2) / 32) | 1) <= 2^18 (fits); polygons
              cannot be banded, so any other job is traced by contours_host on its box copied back.  H, W <= 32768."""
import numpy as np

from . import _lib, _labelmaps, labelmetrics
from ._labelmaps import JOB_COLUMNS as _JOB_COLUMNS, MAX_SIDE, device_stack, host_stack, out_tensor  # noqa: F401  (MAX_SIDE: public here)

KGLibraryError = _lib.KGLibraryError
LDS_BITS = 2 ** 18
_ROW_JOB_COLUMNS = "(img, id, y1, x1, y2, x2, ring_at, vert_at)"


def fits(h, w):
    """True when the device traces a clamped box of h x w pixels: its bitmap with one zero halo on each side and a row pitch of an odd
    number of dwords fits 32 KiB of LDS."""
    h, w = int(h), int(w)
    return h > 0 and w > 0 and (h + 2) * 32 * (((w + 2 + 31) // 32) | 1) <= LDS_BITS


class Contours:
    """Host CSR over the jobs (or the instances): row k owns the rings ring_ptr[k] .. ring_ptr[k + 1]; ring r owns the vertices
    verts[first[r] : first[r] + count[r]] as (y, x).  ring_ptr, first, count, perimeter, area2 are int64, verts is int32 [V, 2]; the
    rings lie in order, so first is the exclusive prefix sum of count."""
    __slots__ = ("ring_ptr", "first", "count", "perimeter", "area2", "verts")

    def __init__(self, ring_ptr, first, count, perimeter, area2, verts):
        self.ring_ptr = np.ascontiguousarray(ring_ptr, np.int64).reshape(-1)
        self.first, self.count, self.perimeter, self.area2 = (np.ascontiguousarray(a, np.int64).reshape(-1)
                                                              for a in (first, count, perimeter, area2))
        self.verts = np.ascontiguousarray(verts, np.int32).reshape(-1, 2)
        R = len(self.count)
        p = self.ring_ptr
        if len(p) < 1 or p[0] != 0 or p[-1] != R or (np.diff(p) < 0).any() or any(len(a) != R for a in (self.first, self.perimeter, self.area2)):
            raise KGLibraryError(f"Contours: ring_ptr of {len(p)} entries ending at {p[-1] if len(p) else None} for {R} rings")
        if (self.count < 0).any() or not np.array_equal(self.first, np.cumsum(self.count) - self.count) or int(self.count.sum()) != len(self.verts):
            raise KGLibraryError(f"Contours: first is not the prefix sum of count, or {len(self.verts)} vertices for counts of {int(self.count.sum())}")

    def __len__(self):
        return len(self.ring_ptr) - 1

    def __eq__(self, other):
        return isinstance(other, Contours) and all(np.array_equal(getattr(self, k), getattr(other, k)) for k in self.__slots__)

    __hash__ = None

    def counts(self):
        """int64 [m]: the number of rings of every row"""
        return np.diff(self.ring_ptr)

    def rows(self):
        """int64 [R]: the row every ring belongs to"""
        return np.repeat(np.arange(len(self), dtype=np.int64), self.counts())

    def _per_row(self, values):
        out = np.zeros(len(self), np.int64)
        np.add.at(out, self.rows(), values)
        return out

    def is_hole(self):
        """bool [R]: the ring runs anticlockwise on the screen (negative area2)"""
        return self.area2 < 0

    def areas(self):
        """int64 [m]: the pixels of every row, the sum of area2 over its rings (holes are negative) / 2"""
        return self._per_row(self.area2) // 2

    def perimeters(self):
        """int64 [m]: the cracks of every row, holes included: the pixel sides that face a pixel outside P"""
        return self._per_row(self.perimeter)

    def slice(self, r0, r1):
        """The Contours of rows r0 .. r1 - 1"""
        a, b = int(self.ring_ptr[r0]), int(self.ring_ptr[r1])
        va = int(self.first[a]) if a < len(self.first) else len(self.verts)
        vb = int(self.first[b]) if b < len(self.first) else len(self.verts)
        return Contours(self.ring_ptr[r0:r1 + 1] - a, self.first[a:b] - va, self.count[a:b], self.perimeter[a:b], self.area2[a:b], self.verts[va:vb])

    def ring(self, r):
        """int32 [count, 2] of (y, x): the vertices of ring r"""
        return self.verts[int(self.first[r]):int(self.first[r] + self.count[r])]

    def of(self, k):
        """The rings of row k: a list of int32 [count, 2] arrays of (y, x), in start order"""
        return [self.ring(r) for r in range(int(self.ring_ptr[k]), int(self.ring_ptr[k + 1]))]

    def coco(self, k):
        """COCO's `segmentation` polygons of row k: one flat [x0, y0, x1, y1, ...] list per OUTER ring.  Holes are dropped: the format has
        no way to say them (run lengths do: runlengths.RunLengths.coco)."""
        return [self.ring(r)[:, ::-1].reshape(-1).tolist() for r in range(int(self.ring_ptr[k]), int(self.ring_ptr[k + 1])) if self.area2[r] > 0]

    def geojson(self, k):
        """A GeoJSON geometry of row k in pixel coordinates [x, y]: a Polygon when the row has one outer ring, else a MultiPolygon (with
        no coordinates for an empty row).  Every ring is closed (its first position repeated) and keeps its traversal order.  A hole goes
        to the smallest-area outer ring that contains, even-odd, the centre of pixel (Y, X) of the hole's start, which is in P."""
        rs = range(int(self.ring_ptr[k]), int(self.ring_ptr[k + 1]))
        outer = sorted((r for r in rs if self.area2[r] > 0), key=lambda r: (int(self.area2[r]), r))
        polys = {r: [self._closed(r)] for r in outer}
        for r in rs:
            if self.area2[r] < 0:
                y, x = self.ring(r)[0]
                home = next((o for o in outer if _inside(self.ring(o), y + 0.5, x + 0.5)), None)
                if home is None:
                    raise KGLibraryError(f"Contours.geojson: the hole ring {r} lies in no outer ring of row {k}")
                polys[home].append(self._closed(r))
        parts = [polys[r] for r in sorted(outer)]
        if len(parts) == 1:
            return {"type": "Polygon", "coordinates": parts[0]}
        return {"type": "MultiPolygon", "coordinates": parts}

    def _closed(self, r):
        v = self.ring(r)[:, ::-1].tolist()
        return v + v[:1]


def _inside(ring, py, px):
    """Even-odd: the point (py, px), off the lattice, against the ring's vertical sides on its right"""
    y0, x0 = ring[:, 0], ring[:, 1]
    y1, x1 = np.roll(y0, -1), np.roll(x0, -1)
    hit = (x0 == x1) & (x0 > px) & (np.minimum(y0, y1) < py) & (py < np.maximum(y0, y1))
    return bool(hit.sum() & 1)


def _assemble(per_job):
    """per_job: one (count, perimeter, area2, verts) per job -> Contours"""
    ptr = np.zeros(len(per_job) + 1, np.int64)
    np.cumsum([len(p[0]) for p in per_job], out=ptr[1:])

    def cat(c, dtype, tail=()):
        parts = [np.asarray(p[c], dtype).reshape((-1,) + tail) for p in per_job]
        return np.concatenate(parts) if parts else np.zeros((0,) + tail, dtype)
    count = cat(0, np.int64)
    return Contours(ptr, np.cumsum(count) - count, count, cat(1, np.int64), cat(2, np.int64), cat(3, np.int32, (2,)))


# ---- host statement of the semantics ------------------------------------------------------------------------------------------------------

_EMPTY = (np.zeros(0, np.int64),) * 3 + (np.zeros((0, 2), np.int32),)


def _trace_mask(me, y1, x1):
    """me: bool [h, w], the membership of a box whose corner is (y1, x1) -> (count, perimeter, area2, verts) of its rings, in order"""
    h, w = me.shape
    m = np.zeros((h + 2, w + 2), bool)
    m[1:-1, 1:-1] = me
    a, b, c, e = m[:-1, :-1], m[:-1, 1:], m[1:, :-1], m[1:, 1:]       # m(Y-1, X-1), m(Y-1, X), m(Y, X-1), m(Y, X) at every vertex (Y, X)
    east = e & ~b
    code = (east.astype(np.uint8) | ((c & ~e) << 1) | ((a & ~c) << 2) | ((b & ~a) << 3)).astype(np.uint8)
    cand = east.copy()
    cand[:, 1:] &= ~east[:, :-1]
    starts = np.flatnonzero(cand.reshape(-1)).tolist()                # raster order
    if not starts:
        return _EMPTY
    ex = code.reshape(-1).tolist()
    is_cand = cand.reshape(-1).tolist()
    seen = set()
    pw = w + 1
    step = (1, pw, -1, -pw)
    counts, perims, areas, verts = [], [], [], []
    for s in starts:
        if s in seen:                                                 # a candidate of a ring that began at a smaller start
            continue
        q, d, per, a2 = s, 0, 0, 0
        ring = [s]
        while True:
            Y, X = divmod(q, pw)
            a2 += (-(y1 + Y), x1 + X, y1 + Y, -(x1 + X))[d]
            q += step[d]
            per += 1
            bitsq = ex[q]
            for nd in ((d + 1) & 3, d, (d + 3) & 3):
                if (bitsq >> nd) & 1:
                    break
            else:
                raise KGLibraryError("contours_host: a crack without a successor")
            if nd == 0 and is_cand[q]:
                if q == s:
                    break
                seen.add(q)
            if nd != d:
                ring.append(q)
            d = nd
        counts.append(len(ring)); perims.append(per); areas.append(a2)
        r = np.array(ring, np.int64)
        verts.append(np.stack([r // pw + y1, r % pw + x1], 1))
    return (np.array(counts, np.int64), np.array(perims, np.int64), np.array(areas, np.int64), np.concatenate(verts).astype(np.int32))


def _job_rings(lab, H, W, job):
    """One map [H, W], one job (id, y1, x1, y2, x2) -> (count, perimeter, area2, verts)"""
    v, y1, x1, y2, x2 = job
    y1, x1, y2, x2 = max(y1, 0), max(x1, 0), min(y2, H), min(x2, W)
    if y2 <= y1 or x2 <= x1:
        return _EMPTY
    me = lab[y1:y2, x1:x2] == v
    if not me.any():
        return _EMPTY
    return _trace_mask(me, y1, x1)


def contours_host(labels, jobs_or_n):
    """labels: integers [H, W] or [nimg, H, W]; jobs_or_n: jobs [m, 6] = (img, id, y1, x1, y2, x2), or the instance count n (one per map
    for a stack): the ids 1 .. n inside their own boxes (labelmetrics.label_stats_host) -> Contours, one row per job.  Never
    size-limited."""
    maps = host_stack("contours_host", labels)
    nimg, H, W = maps.shape
    j = _labelmaps.host_job_table("contours_host", maps, jobs_or_n, labelmetrics.label_stats_host)
    return _assemble([_job_rings(maps[i], H, W, rest) if 0 <= i < nimg else _EMPTY for i, *rest in j.tolist()])


# ---- device -----------------------------------------------------------------------------------------------------------------------------

def contour_counts(labels, jobs):
    """kg_label_contour_counts as it is: labels device int32 [H, W] or [nimg, H, W]; jobs host integers [m, 6] = (img, id, y1, x1, y2, x2)
    (uploaded once) or a device int32 tensor -> device int64 [m, 4] = {rings, vertices, perimeter, status}; status 1: the box does not
    fit the device route (fits) and the counts are 0.  One launch, no copy back, no synchronisation."""
    import torch
    from ._lib import ptr, stream_ptr
    lab = device_stack("contour_counts", labels)[0]
    nimg, H, W = lab.shape
    jd = _labelmaps.device_jobs("contour_counts", jobs, 6, _JOB_COLUMNS, lab.device)
    m = jd.shape[0]
    out = torch.empty(m, 4, dtype=torch.int64, device=lab.device)
    with torch.cuda.device(lab.device):
        _lib.call("kg_label_contour_counts", ptr(lab), nimg, H, W, ptr(jd) if m else None, m, ptr(out) if m else None, stream_ptr())
    return out


def contour_rows(labels, jobs, R, V, rings=None, verts=None):
    """kg_label_contours as it is: jobs host integers [m, 8] = (img, id, y1, x1, y2, x2, ring_at, vert_at) (uploaded once) or a device
    int32 tensor -> (rings device int64 [R, 4] = {first, count, perimeter, area2}, verts device int32 [V, 2] = (y, x)).  rings / verts:
    None (tensors of zeros are made) or contiguous device tensors written in place: only the slots the table names change.  One launch,
    no copy back, no synchronisation."""
    import torch
    from ._lib import ptr, stream_ptr
    lab = device_stack("contour_rows", labels)[0]
    nimg, H, W = lab.shape
    jd = _labelmaps.device_jobs("contour_rows", jobs, 8, _ROW_JOB_COLUMNS, lab.device)
    m = jd.shape[0]
    R, V = int(R), int(V)
    if not 0 <= R <= 2 ** 31 - 1 or not 0 <= V <= 2 ** 31 - 1:
        raise KGLibraryError(f"contour_rows: R {R}, V {V}")
    rings = torch.zeros(R, 4, dtype=torch.int64, device=lab.device) if rings is None else out_tensor("contour_rows", "rings", rings, (R, 4), torch.int64, lab.device)
    verts = torch.zeros(V, 2, dtype=torch.int32, device=lab.device) if verts is None else out_tensor("contour_rows", "verts", verts, (V, 2), torch.int32, lab.device)
    with torch.cuda.device(lab.device):
        _lib.call("kg_label_contours", ptr(lab), nimg, H, W, ptr(jd) if m else None, m, ptr(rings) if R else None, R, ptr(verts) if V else None, V,
                  stream_ptr())
    return rings, verts


def _device_contours(lab, j):
    """lab: device int32 [nimg, H, W], j: host jobs [m, 6], clamped -> Contours.  Two launches, two uploads and two copies back, plus
    one box copied back per job that does not fit."""
    import torch
    nimg, H, W = lab.shape
    m = len(j)
    if m == 0:
        return _assemble([])
    cnt = contour_counts(lab, j).cpu().numpy()
    if (cnt < 0).any() or (cnt[:, 3] > 1).any():
        raise KGLibraryError("contours: counts that are no counts")
    R, V = int(cnt[:, 0].sum()), int(cnt[:, 1].sum())
    if R > 2 ** 31 - 1 or V > 2 ** 31 - 1:
        raise KGLibraryError(f"contours: {R} rings, {V} vertices exceed 2^31 - 1")
    ptr = np.zeros(m + 1, np.int64)
    np.cumsum(cnt[:, 0], out=ptr[1:])
    if R:
        table = np.concatenate([j.astype(np.int64), ptr[:-1, None], (np.cumsum(cnt[:, 1]) - cnt[:, 1])[:, None]], 1)
        buf = torch.empty(32 * R + 8 * V, dtype=torch.uint8, device=lab.device)            # both outputs in one buffer: one copy back
        contour_rows(lab, table, R, V, buf[:32 * R].view(torch.int64).view(R, 4), buf[32 * R:].view(torch.int32).view(V, 2))
        host = buf.cpu().numpy()
        rows, verts = host[:32 * R].view(np.int64).reshape(R, 4), host[32 * R:].view(np.int32).reshape(V, 2)
    else:
        rows, verts = np.zeros((0, 4), np.int64), np.zeros((0, 2), np.int32)
    if not np.array_equal(rows[:, 1], np.diff(np.concatenate([rows[:, 0], [V]]))):
        raise KGLibraryError("contours: ring rows whose vertex ranges do not tile the vertex list")
    got = Contours(ptr, rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], verts)
    if not np.array_equal(got.perimeters(), cnt[:, 2]):
        raise KGLibraryError("contours: the rings' cracks do not add up to the counted perimeter")
    large = np.flatnonzero(cnt[:, 3]).tolist()
    if not large:
        return got
    per = [(s.count, s.perimeter, s.area2, s.verts) for s in (got.slice(k, k + 1) for k in range(m))]
    for k in large:                                                   # polygons cannot be banded: the box comes back and the host traces it
        i, v, y1, x1, y2, x2 = j[k].tolist()
        me = lab[i, y1:y2, x1:x2].cpu().numpy() == v
        per[k] = _trace_mask(me, y1, x1) if me.any() else _EMPTY
    return _assemble(per)


def contours(labels, n=None, jobs=None, stats=None):
    """contours_host on the device -> Contours (host).  labels: device int32 [H, W] or [nimg, H, W].  What is traced:
      jobs   host integers [m, 6] = (img, id, y1, x1, y2, x2): one row per job; or
      n      the instance count (one per map for a stack): the ids 1 .. n inside their own boxes.  The boxes come from stats -- host
             integers [n, 5] = (area, y1, x1, y2, x2), one array per map for a stack -- or, without stats, from labelmetrics.label_stats.
    ONE kg_label_contour_counts launch and one small copy back, a host prefix over rings and vertices, ONE kg_label_contours launch and
    one copy back.  A job whose box does not fit the device route (fits) is traced by the host tracer on its box, sliced from the device
    map and copied back alone."""
    lab = device_stack("contours", labels)[0]
    return _device_contours(lab, _labelmaps.job_table("contours", lab, n, jobs, stats, labelmetrics.label_stats))


# ---- Instances ----------------------------------------------------------------------------------------------------------------------------

def _instance_contours(insts):
    """-> one Contours per entry (None for a None entry); the entries themselves are not touched"""
    out = [None] * len(insts)

    def host_one(i, inst, lab):
        out[i] = contours_host(lab, _labelmaps.instance_jobs(inst, 0, 0, *lab.shape))
    for idx, stack, H, W in _labelmaps.size_batches("contours_instances", insts, host_one):
        got = _device_contours(device_stack("contours_instances", stack)[0], _labelmaps.batch_jobs(insts, idx, 0, H, W))
        for i, a, b in _labelmaps.deal(insts, idx):
            out[i] = got.slice(a, b)
    return out


def contours_instances(inst):
    """contours for an Instances / TiledInstances -> Contours with len(inst) rows: ids 1 .. n, boxes from table[:, 2:6]; an instance with
    no visible pixel gets an empty row.  A host label map (assemble_host's result) goes through contours_host."""
    return _instance_contours([inst])[0]


def contours_instances_batch(insts):
    """contours_instances for predict_instances' list (entries may be None), in place: every entry's `contours` is set.  ONE pair of
    launches per output size."""
    for v, g in zip(insts, _instance_contours(insts)):
        if v is not None:
            v.contours = g
    return insts
