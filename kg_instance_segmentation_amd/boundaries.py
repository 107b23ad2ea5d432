"""Boundary distances between two label maps on the device: Hausdorff, HD95, ASSD and the normalised surface Dice of matched instances.

labelmetrics.py scores a predicted label map against a ground truth by overlap only: every metric there is a function of pixel counts, and
overlap cannot see how far a wrong outline lies from the right one.  Here the device takes the outline pixels of one instance and finds,
for each, the exact squared distance to the nearest outline pixel of an instance of the OTHER map (kg_label_border_counts,
kg_label_border_d2, csrc/boundaries.hip); a few hundred integers per pair come back instead of two maps and one distance transform per
pair, and the metrics are host float64 over those integers.

    border_host        the border pixels of an id in a map, in NumPy
    border_d2_host     both entries in NumPy (the yardstick): the plain minimum over all target pixels by broadcasting
    border_d2_store_host  kg_label_border_d2 in NumPy, `first` and the store predicate included
    border_counts      kg_label_border_counts as it is: ONE launch, rows stay on the device
    border_d2          kg_label_border_d2 as it is: ONE launch, values stay on the device
    pair_jobs          id pairs and the two stats tables -> the jobs of both directions, cut to the size rule, and their PairJobs record
    merge_pieces       the counts and values of those jobs -> PairDistances (shared by both routes)
    pair_distances     the device route: two launches with one host prefix sum between them, two copies back
    pair_distances_host  the host route
    PairDistances      host CSR per pair and direction with int32 d2: of(k, direction), directed_hausdorff(), hausdorff(), hd95(), assd(),
                       nsd(tolerance)

Semantics (include/kgnet_hip.h is the normative text)
  maps        a and b: int32 [nimg, H, W] (pair_distances: one map [H, W] each), one shape, one device.  Values are compared only.
  border      a pixel that holds v and has one of its four side-neighbours outside the map or holding another value -- read from the MAP,
              never from a box: mask & ~scipy.ndimage.binary_erosion(mask).
  job         {img, dir, id_s, sy1, sx1, sy2, sx2, id_t, ty1, tx1, ty2, tx2, first}: dir == 0 takes sources from a and targets from b,
              dir != 0 the other way round; both boxes half-open, clamped to the map.
  mode        bit 0, sources: 0 = the border pixels of id_s in the source box, 1 = all its pixels; bit 1, targets: 0 = border, 2 = region.
  value       d2(s) = the minimum over the border pixels t of id_t in the target box of (ys - yt)^2 + (xs - xt)^2; in region mode 0 when
              s lies in the target box and the target map holds id_t there; -1 when there is no target and the region rule does not apply.
  size rule   a target box of more than MAX_TARGET_PIXELS = 8192 pixels: count {0, 0}, status 1, nothing stored.  pair_jobs cuts target
              boxes into rectangles within the rule (their values merge by the element-wise minimum, -1 as +infinity) and source boxes of
              more than max_job_pixels pixels into bands of whole rows (their values concatenate in raster order).
  bad jobs    an image outside [0, nimg), an empty or inverted box on either side: nothing.
  metrics     host float64 from the integers only, every list sorted first: nothing depends on an order of summation.  A -1 is an
              unreachable pixel: the pair's hausdorff is inf, and the pixel lies outside every tolerance."""
import math

import numpy as np

from . import _lib, _labelmaps, labelmetrics
from ._labelmaps import MAX_SIDE, device_maps, host_stack, is_device, out_tensor  # noqa: F401  (MAX_SIDE: public here)

KGLibraryError = _lib.KGLibraryError
MAX_TARGET_PIXELS = 8192
JOB_COLUMNS = "(img, dir, id_s, sy1, sx1, sy2, sx2, id_t, ty1, tx1, ty2, tx2, first)"
_SOURCES = {"border": 0, "all": 1}
_TARGETS = {"border": 0, "region": 2}


def mode_of(fn, sources="border", targets="border"):
    """sources: 'border' or 'all'; targets: 'border' or 'region' -> the two mode bits"""
    if sources not in _SOURCES or targets not in _TARGETS:
        raise KGLibraryError(f"{fn}: sources {sources!r} ('border' or 'all'), targets {targets!r} ('border' or 'region')")
    return _SOURCES[sources] | _TARGETS[targets]


def _mode(fn, mode):
    if isinstance(mode, (bool, np.bool_)) or int(mode) != mode or not 0 <= int(mode) <= 3:
        raise KGLibraryError(f"{fn}: mode {mode!r} (0 .. 3: bit 0 = all sources, bit 1 = region targets)")
    return int(mode)


# ---- host statements of the semantics ---------------------------------------------------------------------------------------------------

def _members(lab, v, y1, x1, y2, x2):
    """One map [H, W], a non-empty box inside it -> (members, border) bool [h, w]: the pixels of the box that hold v, and those of them with
    a side-neighbour outside the map or of another value; the neighbours come from the map."""
    H, W = lab.shape
    ya, xa, yb, xb = max(y1 - 1, 0), max(x1 - 1, 0), min(y2 + 1, H), min(x2 + 1, W)
    big = np.zeros((y2 - y1 + 2, x2 - x1 + 2), bool)                   # the box with a ring of one pixel: False outside the map
    big[ya - y1 + 1:yb - y1 + 1, xa - x1 + 1:xb - x1 + 1] = lab[ya:yb, xa:xb] == v
    me = big[1:-1, 1:-1]
    return me, me & ~(big[:-2, 1:-1] & big[2:, 1:-1] & big[1:-1, :-2] & big[1:-1, 2:])


def border_host(labels, v):
    """One map [H, W] -> bool [H, W]: the border pixels of id v"""
    lab = _labelmaps.host_maps("border_host", labels, False)
    return _members(lab, int(v), 0, 0, *lab.shape)[1]


def _clamp(box, H, W):
    y1, x1, y2, x2 = box
    return max(y1, 0), max(x1, 0), min(y2, H), min(x2, W)


_NO = np.zeros(0, np.int32)


def _job_d2(src, dst, job, mode):
    """One job on the maps of its image -> ((n_sources, n_targets, status), int32 d2 of its sources in raster order)"""
    H, W = src.shape
    id_s, id_t = job[0], job[5]
    sy1, sx1, sy2, sx2 = _clamp(job[1:5], H, W)
    ty1, tx1, ty2, tx2 = _clamp(job[6:10], H, W)
    if sy2 <= sy1 or sx2 <= sx1 or ty2 <= ty1 or tx2 <= tx1:
        return (0, 0, 0), _NO
    if (ty2 - ty1) * (tx2 - tx1) > MAX_TARGET_PIXELS:
        return (0, 0, 1), _NO
    me, edge = _members(src, id_s, sy1, sx1, sy2, sx2)
    ys, xs = np.nonzero(me if mode & 1 else edge)                      # raster order
    ys, xs = ys.astype(np.int64) + sy1, xs.astype(np.int64) + sx1
    inside, tedge = _members(dst, id_t, ty1, tx1, ty2, tx2)
    yt, xt = np.nonzero(tedge)
    yt, xt = yt.astype(np.int64) + ty1, xt.astype(np.int64) + tx1
    d2 = np.full(len(ys), -1, np.int64)
    if len(yt):
        step = max(int(2 ** 22 // len(yt)), 1)                         # the broadcast in slabs of some four million distances
        for k in range(0, len(ys), step):
            d2[k:k + step] = ((ys[k:k + step, None] - yt[None]) ** 2 + (xs[k:k + step, None] - xt[None]) ** 2).min(1)
    if mode & 2:
        at = (ys >= ty1) & (ys < ty2) & (xs >= tx1) & (xs < tx2)
        at[at] = inside[ys[at] - ty1, xs[at] - tx1]
        d2[at] = 0
    return (len(ys), len(yt), 0), d2.astype(np.int32)


def _host_pieces(fn, a, b, jobs, mode):
    ma, mb = host_stack(fn, a), host_stack(fn, b)
    if ma.shape != mb.shape:
        raise KGLibraryError(f"{fn}: maps of {ma.shape} and {mb.shape} must have one shape")
    j = _labelmaps.host_jobs(fn, jobs, 13, JOB_COLUMNS).astype(np.int64)
    mode = _mode(fn, mode)
    counts, vals = np.zeros((len(j), 3), np.int32), []
    for k, row in enumerate(j.tolist()):
        if not 0 <= row[0] < len(ma):
            vals.append(_NO)
            continue
        src, dst = (mb, ma) if row[1] else (ma, mb)
        counts[k], d2 = _job_d2(src[row[0]], dst[row[0]], row[2:12], mode)
        vals.append(d2)
    return j, counts, vals


def border_d2_host(a, b, jobs, mode=0):
    """Both entries in NumPy: a, b integers [H, W] or [nimg, H, W]; jobs integers [m, 13] = JOB_COLUMNS (`first` is ignored)
    -> (counts int32 [m, 3] = {n_sources, n_targets, status}, a list of m int32 arrays: the d2 of every job's sources in raster order).
    The plain minimum over all target pixels; no distance transform."""
    _, counts, vals = _host_pieces("border_d2_host", a, b, jobs, mode)
    return counts, vals


def border_d2_store_host(a, b, jobs, mode, D, fill=0):
    """kg_label_border_d2 in NumPy -> int32 [D], which starts as `fill` everywhere: the k-th source of job j stores into out[first_j + k]
    only when the slot lies in [0, D)."""
    j, _, vals = _host_pieces("border_d2_store_host", a, b, jobs, mode)
    D = int(D)
    if D < 0:
        raise KGLibraryError(f"border_d2_store_host: D {D}")
    out = np.full(D, fill, np.int32)
    for first, d2 in zip(j[:, 12].tolist(), vals):
        slot = first + np.arange(len(d2), dtype=np.int64)
        keep = (slot >= 0) & (slot < D)
        out[slot[keep]] = d2[keep]
    return out


# ---- device: the raw entries --------------------------------------------------------------------------------------------------------------

def _device_pair(fn, a, b):
    a = device_maps(fn, a, True)
    b = device_maps(fn, b, True, like=a)
    a, b = a.view((-1,) + a.shape[-2:]), b.view((-1,) + b.shape[-2:])
    _labelmaps.side(fn, a)
    return a, b


def border_counts(a, b, jobs, mode=0):
    """kg_label_border_counts as it is: a, b device int32 [H, W] or [nimg, H, W]; jobs host integers [m, 13] = JOB_COLUMNS (uploaded once)
    or a device int32 tensor -> device int32 [m, 3] = {n_sources, n_targets, status}.  One launch, no copy back, no synchronisation."""
    import torch
    from ._lib import ptr, stream_ptr
    a, b = _device_pair("border_counts", a, b)
    nimg, H, W = a.shape
    jd = _labelmaps.device_jobs("border_counts", jobs, 13, JOB_COLUMNS, a.device)
    m = jd.shape[0]
    out = torch.empty(m, 3, dtype=torch.int32, device=a.device)
    with torch.cuda.device(a.device):
        _lib.call("kg_label_border_counts", ptr(a), ptr(b), nimg, H, W, ptr(jd) if m else None, m, _mode("border_counts", mode),
                  ptr(out) if m else None, stream_ptr())
    return out


def border_d2(a, b, jobs, mode, D, out=None):
    """kg_label_border_d2 as it is -> device int32 [D].  out: None (a tensor of zeros is made) or a contiguous device int32 [D] that is
    written in place: only the slots the table names change.  One launch, no copy back, no synchronisation."""
    import torch
    from ._lib import ptr, stream_ptr
    a, b = _device_pair("border_d2", a, b)
    nimg, H, W = a.shape
    jd = _labelmaps.device_jobs("border_d2", jobs, 13, JOB_COLUMNS, a.device)
    m = jd.shape[0]
    D = int(D)
    if not 0 <= D <= 2 ** 31 - 1:
        raise KGLibraryError(f"border_d2: D {D}")
    out = torch.zeros(D, dtype=torch.int32, device=a.device) if out is None else out_tensor("border_d2", "out", out, (D,), torch.int32, a.device)
    with torch.cuda.device(a.device):
        _lib.call("kg_label_border_d2", ptr(a), ptr(b), nimg, H, W, ptr(jd) if m else None, m, _mode("border_d2", mode),
                  ptr(out) if D else None, D, stream_ptr())
    return out


# ---- pairs: jobs of both directions, cut to the size rule ---------------------------------------------------------------------------------

class PairJobs:
    """jobs int32 [m, 13] (first = 0) in the order (owner, direction, order, target rectangle); owner int64 [m]: the pair a job belongs
    to; direction int64 [m]: 0 = from a to b, 1 = from b to a; order int64 [m]: the source band of the job inside its pair and direction,
    ascending in y.  Jobs of one (owner, direction, order) have one source band and the rectangles of the target box: they merge by the
    element-wise minimum; the bands concatenate."""
    __slots__ = ("jobs", "owner", "direction", "order", "npairs")

    def __init__(self, jobs, owner, direction, order, npairs):
        self.jobs = np.ascontiguousarray(jobs, np.int32).reshape(-1, 13)
        self.owner, self.direction, self.order = (np.ascontiguousarray(v, np.int64).reshape(-1) for v in (owner, direction, order))
        self.npairs = int(npairs)

    def __len__(self):
        return len(self.jobs)


def _cuts(lo, hi, step):
    """[lo, hi) in pieces of `step` -> (starts, ends)"""
    s = np.arange(lo, hi, step, dtype=np.int64)
    return s, np.minimum(s + step, hi)


def pair_jobs(pairs, stats_a, stats_b, H, W, max_job_pixels=65536, img=0):
    """pairs: integers [k, 2] = (id in a, id in b), 1-based rows of stats_a / stats_b, integers [n, 5] = (area, y1, x1, y2, x2)
    (labelmetrics.STATS_COLUMNS) -> PairJobs for both directions.  Source boxes of more than max_job_pixels pixels are cut into bands of
    max(max_job_pixels // w, 1) whole rows; target boxes into rectangles of at most MAX_TARGET_PIXELS pixels (full width when the width
    fits, else pieces of 8192 columns of one row).  An id of area 0 as a source gives no job; as a target it gives the box of pixel
    (0, 0), where it has no pixel: every source then gets -1."""
    fn = "pair_jobs"
    cap = _labelmaps.check_cap(fn, max_job_pixels)
    p = np.asarray(pairs)
    if p.size == 0:
        p = np.zeros((0, 2), np.int64)
    sa, sb = labelmetrics._stats(fn, stats_a), labelmetrics._stats(fn, stats_b)
    if p.ndim != 2 or p.shape[1] != 2 or p.dtype.kind not in "iu" or (len(p) and (p.min() < 1 or p[:, 0].max() > len(sa) or p[:, 1].max() > len(sb))):
        raise KGLibraryError(f"{fn}: pairs must be integers [k, 2] of ids in 1 .. {len(sa)} and 1 .. {len(sb)}")
    H, W = int(H), int(W)
    p = p.astype(np.int64)
    K = len(p)

    def clamped(st, ids):
        box = st[ids - 1, 1:].copy()
        box[:, :2] = np.clip(box[:, :2], 0, [H, W]); box[:, 2:] = np.clip(box[:, 2:], 0, [H, W])
        return box, (st[ids - 1, 0] > 0) & (box[:, 2] > box[:, 0]) & (box[:, 3] > box[:, 1])
    (ba, has_a), (bb, has_b) = clamped(sa, p[:, 0]), clamped(sb, p[:, 1])
    # row 2 k + d: direction d of pair k
    ids_s, ids_t = np.stack([p[:, 0], p[:, 1]], 1).reshape(-1), np.stack([p[:, 1], p[:, 0]], 1).reshape(-1)
    sbox, tbox = np.stack([ba, bb], 1).reshape(-1, 4), np.stack([bb, ba], 1).reshape(-1, 4)
    has_s, has_t = np.stack([has_a, has_b], 1).reshape(-1), np.stack([has_b, has_a], 1).reshape(-1)
    tbox[~has_t] = [0, 0, 1, 1]
    own, dirn = np.repeat(np.arange(K, dtype=np.int64), 2), np.tile(np.arange(2, dtype=np.int64), K)
    sh, sw = sbox[:, 2] - sbox[:, 0], sbox[:, 3] - sbox[:, 1]
    whole = has_s & (sh * sw <= cap) & ((tbox[:, 2] - tbox[:, 0]) * (tbox[:, 3] - tbox[:, 1]) <= MAX_TARGET_PIXELS)
    n1 = int(whole.sum())
    rows = [np.concatenate([np.full((n1, 1), int(img)), dirn[whole, None], ids_s[whole, None], sbox[whole], ids_t[whole, None], tbox[whole],
                            np.zeros((n1, 1), np.int64)], 1)]
    key, order = [2 * own[whole] + dirn[whole]], [np.zeros(n1, np.int64)]
    for r in np.flatnonzero(has_s & ~whole).tolist():                  # the few that are cut
        (sy1, sx1, sy2, sx2), (ty1, tx1, ty2, tx2) = sbox[r].tolist(), tbox[r].tolist()
        w = sx2 - sx1
        by1, by2 = _cuts(sy1, sy2, max(cap // w, 1) if (sy2 - sy1) * w > cap else sy2 - sy1)
        cw = min(tx2 - tx1, MAX_TARGET_PIXELS)
        ry1, ry2 = _cuts(ty1, ty2, max(MAX_TARGET_PIXELS // cw, 1))
        rx1, rx2 = _cuts(tx1, tx2, cw)
        nb, nr = len(by1), len(ry1) * len(rx1)
        band = np.repeat(np.arange(nb), nr)
        gy, gx = np.repeat(np.arange(len(ry1)), len(rx1)), np.tile(np.arange(len(rx1)), len(ry1))
        gy, gx = np.tile(gy, nb), np.tile(gx, nb)
        n = nb * nr
        rows.append(np.stack([np.full(n, int(img)), np.full(n, dirn[r]), np.full(n, ids_s[r]), by1[band], np.full(n, sx1), by2[band], np.full(n, sx2),
                              np.full(n, ids_t[r]), ry1[gy], rx1[gx], ry2[gy], rx2[gx], np.zeros(n, np.int64)], 1))
        key.append(np.full(n, r)); order.append(band)
    rows, key, order = np.concatenate(rows).reshape(-1, 13), np.concatenate(key), np.concatenate(order)
    at = np.argsort(key, kind="stable")                                # (owner, direction); bands and rectangles keep their order
    return PairJobs(rows[at], key[at] // 2, key[at] % 2, order[at], K)


class PairDistances:
    """Host CSR per pair and direction: row 2 k + direction owns d2[indptr[2 k + direction] : indptr[2 k + direction + 1]], int32, the
    sources in raster order; direction 0 = from the pair's id in a to its id in b, 1 = the other way.  -1 = unreachable."""
    __slots__ = ("indptr", "d2", "_cache")

    def __init__(self, indptr, d2):
        self._cache = None
        self.indptr = np.ascontiguousarray(indptr, np.int64).reshape(-1)
        self.d2 = np.ascontiguousarray(d2, np.int32).reshape(-1)
        if len(self.indptr) < 1 or len(self.indptr) % 2 != 1 or self.indptr[0] != 0 or self.indptr[-1] != len(self.d2) or (np.diff(self.indptr) < 0).any():
            raise KGLibraryError(f"PairDistances: indptr of {len(self.indptr)} entries for {len(self.d2)} distances")

    def __len__(self):
        return (len(self.indptr) - 1) // 2

    def __eq__(self, other):
        return isinstance(other, PairDistances) and np.array_equal(self.indptr, other.indptr) and np.array_equal(self.d2, other.d2)

    __hash__ = None

    def of(self, k, direction):
        """int32: the d2 of pair k in one direction, the sources in raster order"""
        r = 2 * int(k) + (1 if direction else 0)
        return self.d2[int(self.indptr[r]):int(self.indptr[r + 1])]

    def counts(self):
        """int64 [k, 2]: the sources of every pair and direction"""
        return np.diff(self.indptr).reshape(-1, 2)

    def _pairs(self):
        """-> (the d2 of every pair, both directions together, ascending as unsigned numbers -- so -1 comes last --, where every pair begins)"""
        if self._cache is None:
            start = self.indptr[::2]
            u = self.d2.view(np.uint32)
            self._cache = (u[np.lexsort((u, np.repeat(np.arange(len(self)), np.diff(start))))], start)
        return self._cache

    def directed_hausdorff(self):
        """float64 [k, 2]: sqrt of the largest d2 of every direction; inf with an unreachable source, and for a direction without sources"""
        out = np.full(2 * len(self), np.inf)
        rows = np.flatnonzero(np.diff(self.indptr))
        if len(rows):
            top = np.maximum.reduceat(self.d2.view(np.uint32), self.indptr[rows])     # rows without sources have no width: the next begins there
            out[rows] = np.where(top == 0xFFFFFFFF, np.inf, np.sqrt(top.astype(np.float64)))
        return out.reshape(-1, 2)

    def hausdorff(self):
        """float64 [k]: the maximum of the two directions"""
        return self.directed_hausdorff().max(1)

    def _roots(self):
        u, start = self._pairs()
        return np.where(u == 0xFFFFFFFF, np.inf, np.sqrt(u.astype(np.float64))), start

    def hd95(self, q=95.0):
        """float64 [k]: np.percentile (linear interpolation) of the square roots of both directions together, as medpy's hd95 -- the same
        arithmetic, for all pairs at once --; inf when the interpolation touches an unreachable source; nan for a pair without sources"""
        r, start = self._roots()
        n = np.diff(start)
        out = np.full(len(self), np.nan)
        k = np.flatnonzero(n)
        at = (n[k] - 1) * (float(q) / 100.0)
        lo = np.clip(np.floor(at), 0, n[k] - 1).astype(np.int64)
        t = at - lo
        a, b = r[start[k] + lo], r[start[k] + np.minimum(lo + 1, n[k] - 1)]
        with np.errstate(invalid="ignore"):
            diff = b - a
            v = np.where(t >= 0.5, b - diff * (1 - t), a + diff * t)
        out[k] = np.where(np.isnan(v), np.inf, v)
        return out

    def assd(self):
        """float64 [k]: (the sum of the square roots of both directions, by math.fsum) / (the number of sources of both); inf with an
        unreachable source; nan for a pair without sources"""
        r, start = self._roots()
        r, start = r.tolist(), start.tolist()
        return np.array([math.fsum(r[a:b]) / (b - a) if b > a else math.nan for a, b in zip(start[:-1], start[1:])], np.float64).reshape(-1)

    def nsd(self, tolerance):
        """float64 [k]: the sources of both directions with 0 <= d2 <= floor(tolerance^2), over the sources of both; nan without sources"""
        if not float(tolerance) >= 0:
            raise KGLibraryError(f"nsd: tolerance {tolerance!r}")
        t2 = np.uint32(min(math.floor(float(tolerance) * float(tolerance)), 0xFFFFFFFE))
        u, start = self._pairs()
        within = np.concatenate([[0], np.cumsum(u <= t2)])
        n = np.diff(start)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(n > 0, (within[start[1:]] - within[start[:-1]]) / n, np.nan)


def merge_pieces(pj, counts, d2):
    """pj: a PairJobs; counts: integers [m, 3] of its jobs; d2: the values of the jobs one after another (job j's at the exclusive prefix
    sum of n_sources) -> PairDistances.  The rectangles of one band merge by the element-wise minimum with -1 as +infinity -- as unsigned
    numbers -1 is the largest --; the bands concatenate in raster order."""
    cnt = np.asarray(counts, np.int64).reshape(-1, 3)
    d2 = np.ascontiguousarray(d2, np.int32).reshape(-1)
    m = len(pj)
    if len(cnt) != m or (m and ((cnt[:, 2] != 0).any() or (cnt[:, :2] < 0).any())) or int(cnt[:, 0].sum()) != len(d2):
        raise KGLibraryError(f"merge_pieces: {len(cnt)} count rows and {len(d2)} distances for {m} jobs (or a job that broke the size rule)")
    indptr = np.zeros(2 * pj.npairs + 1, np.int64)
    if m == 0:
        return PairDistances(indptr, _NO)
    key = np.stack([pj.owner, pj.direction, pj.order], 1)
    new = np.ones(m, bool)
    new[1:] = (key[1:] != key[:-1]).any(1)                             # the first job of every (owner, direction, band)
    group = np.cumsum(new) - 1
    ns = cnt[:, 0]
    size = ns[new]
    if (ns != size[group]).any():
        raise KGLibraryError("merge_pieces: the jobs of one source band do not agree on its sources")
    at = np.cumsum(size) - size                                        # where every group begins in the merged list
    first = np.cumsum(ns) - ns
    dest = np.repeat(at[group] - first, ns) + np.arange(len(d2), dtype=np.int64)
    out = np.full(int(size.sum()), 0xFFFFFFFF, np.uint32)
    if new.all():
        out[dest] = d2.view(np.uint32)
    else:
        np.minimum.at(out, dest, d2.view(np.uint32))
    np.add.at(indptr, 2 * pj.owner[new] + pj.direction[new] + 1, size)
    return PairDistances(np.cumsum(indptr), out.view(np.int32))


def _pair_args(fn, shape, pairs, stats_a, stats_b, n_a, n_b, stats_of, a, b, sources, targets, max_job_pixels):
    H, W = shape
    mode = mode_of(fn, sources, targets)
    if stats_a is None:
        if n_a is None:
            raise KGLibraryError(f"{fn}: stats_a or the instance count n_a is needed")
        stats_a = stats_of(a, n_a)
    if stats_b is None:
        if n_b is None:
            raise KGLibraryError(f"{fn}: stats_b or the instance count n_b is needed")
        stats_b = stats_of(b, n_b)
    return pair_jobs(pairs, stats_a, stats_b, H, W, max_job_pixels), mode


def pair_distances_host(a, b, pairs, stats_a=None, stats_b=None, n_a=None, n_b=None, sources="border", targets="border", max_job_pixels=65536):
    """pair_distances in NumPy on host maps [H, W]: the same jobs (pair_jobs), border_d2_host on them, the same merge."""
    fn = "pair_distances_host"
    a, b = _labelmaps.side(fn, _labelmaps.host_maps(fn, a, False)), _labelmaps.host_maps(fn, b, False)
    if a.shape != b.shape:
        raise KGLibraryError(f"{fn}: maps of {a.shape} and {b.shape} must have one shape")
    pj, mode = _pair_args(fn, a.shape, pairs, stats_a, stats_b, n_a, n_b, labelmetrics.label_stats_host, a, b, sources, targets, max_job_pixels)
    counts, vals = border_d2_host(a, b, pj.jobs, mode)
    return merge_pieces(pj, counts, np.concatenate(vals) if vals else _NO)


def pair_distances(a, b, pairs, stats_a=None, stats_b=None, n_a=None, n_b=None, sources="border", targets="border", max_job_pixels=65536):
    """The distances of id pairs between two device label maps -> PairDistances (host).  a, b: device int32 [H, W]; pairs: host integers
    [k, 2] = (id in a, id in b), for instance the pairs of a labelmetrics.Contingency.  The boxes come from stats_a / stats_b -- host
    integers [n, 5] = (area, y1, x1, y2, x2); columns 1:6 of an Instances table are that -- or, without them, from
    labelmetrics.label_stats(map, n_a / n_b) (its launch and one copy per side).  sources: 'border' or 'all'; targets: 'border' (surface to
    surface, the medpy / MONAI convention) or 'region' (a source inside the target object has distance 0, GlaS).
    One upload, ONE kg_label_border_counts launch and one small copy back, a host prefix sum, ONE kg_label_border_d2 launch and one copy
    back: two launches and two copies whatever the maps hold."""
    import torch
    fn = "pair_distances"
    a = _labelmaps.side(fn, device_maps(fn, a, False))
    b = device_maps(fn, b, False, like=a)
    pj, mode = _pair_args(fn, a.shape, pairs, stats_a, stats_b, n_a, n_b, labelmetrics.label_stats, a, b, sources, targets, max_job_pixels)
    if len(pj) == 0:
        return merge_pieces(pj, np.zeros((0, 3), np.int64), _NO)
    table = pj.jobs.astype(np.int64)
    cnt = border_counts(a, b, table, mode).cpu().numpy().astype(np.int64)
    D = int(cnt[:, 0].sum())
    if D > 2 ** 31 - 1:
        raise KGLibraryError(f"{fn}: {D} sources exceed 2^31 - 1")
    if D == 0:
        return merge_pieces(pj, cnt, _NO)
    table[:, 12] = np.cumsum(cnt[:, 0]) - cnt[:, 0]
    d2 = border_d2(a, b, table, mode, D, torch.empty(D, dtype=torch.int32, device=a.device)).cpu().numpy()
    return merge_pieces(pj, cnt, d2)
