"""Linking label maps: which instance of one map is which instance of another, without copying a map back.

Every other label-map module looks at one map at a time; labelmetrics.contingency relates one prediction to one ground truth at the same
position.  This module relates ANY two maps of one size, optionally displaced by a drift vector, for a whole stack in one launch: the
frames of a time-lapse (tracks with births, deaths and divisions), the planes of a z-stack (2-D predictions stitched into a label
volume), two segmentations of one image (nuclei in cells).  The device lists, per instance of one map, the values of the other map under
its pixels in ascending order with their pixel counts (kg_label_overlaps, csrc/linking.hip), a few thousand integers come back, and the
host links.

    overlaps_rows_host  the row semantics in NumPy, resume / after / more included (the yardstick of the raw entry)
    overlaps_rows       kg_label_overlaps as it is: ONE launch, rows stay on the device
    overlaps_host       the lists in NumPy, stated directly: per job the full sorted list, nothing paged, nothing split
    overlaps            the same lists from device maps: bands, one launch per round of paging, merged on the host
    paged               the pager and merger both routes share; it takes the row function as an argument
    Overlaps            host CSR over the jobs: indptr, values, pixels, area, zero, outside; of(k), rows(), pairs(), iou(), fraction_of_b()
    link                greedy one-to-one links by IoU, then the child rule; successors, parents, division flags (host)
    track_host / track  a [T, H, W] stack -> Tracks: the stack relabelled by track id, track_of, the track table, lineage()
    track_instances     the same for equal-sized predict_instances / predict_tiled results
    stitch_planes       track with the child rule off: one id per object through z
    relate_host / relate  per child the parent that holds most of it and the fraction inside; per parent the child count

Semantics (include/kgnet_hip.h is the normative text)
  job         {img_a, id, y1, x1, y2, x2, img_b, dy, dx}: a half-open box, clamped to the map.  P = the pixels of the box in a[img_a] that
              hold id.  The partner of (y, x) is (y + dy, x + dx) in b[img_b].  b may be a itself (img_b = img_a + 1).
  area        |P|;  outside = the pixels of P whose partner is not in the map;  zero = those whose partner holds 0
  pixels[v]   the pixels of P whose partner holds v, v != 0.  area = zero + outside + sum of pixels.  The ids of the two maps are unrelated:
              id itself, INT_MIN, -1 and INT_MAX are ordinary partner values.
  row         int64 [5 + 2 slots] = {count, more, area, zero, outside, (value, pixels) x slots} of a job {..., resume, after}: the values
              in ascending signed order, with resume != 0 only those > after; count = the slots filled; more = 1 exactly when a further
              qualifying value exists; unused slots are zeros; area, zero and outside are over all of P on a resumed row too.
  bad jobs    an image index of either side outside its stack, an empty or inverted box, an id the box does not hold: a row of zeros.
  sizes       H, W <= 32768 as in measure.py; 1 <= slots <= 64.
  bands       a job whose clamped box holds more than max_job_pixels pixels is split as labelmetrics.split_jobs does; every piece is
              paged on its own, and the pieces of a job are merged by value: pixels, area, zero and outside add.
  job tables  [m, 9] as above; or [m, 6] = (pair, id, y1, x1, y2, x2) / an instance count n per map of a, together with
              pairs [k, 2] = (img_a, img_b) (default: image i of a against image i of b) and shift = (dy, dx) or one per pair: the first
              column of a [m, 6] table names the pair, and n lists, pair after pair, the ids 1 .. n[img_a] inside their own boxes.
  iou         pixels / (area + area_b - pixels), fraction_of_b = pixels / area_b, float64 from the integers: both routes give the same floats.
  link        candidate pairs sorted by (-iou, a, b) are accepted greedily one-to-one while iou >= min_iou; then a b without a link takes
              as parent the a it shares the most pixels with (ties: the smallest a) if pixels / area_b >= min_child (None: no child rule).
              An a with two or more children is a division; a sole child is its successor.
  tracks      ids 1 .. K in order of (first frame, id); a sole successor keeps the track; the children of a division start new tracks whose
              parent is the divided track; an id without pixels has no track (0).

Out of scope: gap closing across missed frames, drift estimation (shift comes from the caller), motion models, and any change to
inference.py's signatures -- track_instances takes the results as they are."""
from collections import namedtuple

import numpy as np

from . import _lib, _labelmaps, labelmetrics
from ._labelmaps import MAX_SIDE, device_stack, host_stack  # noqa: F401  (MAX_SIDE: public here)
from .labelmetrics import split_jobs

KGLibraryError = _lib.KGLibraryError
COUNTS_FIT = "the bound that keeps the kernel's 32-bit partial counts exact"     # what the side bound protects here
MAX_SLOTS = 64
_JOB_COLUMNS = "(img_a, id, y1, x1, y2, x2, img_b, dy, dx)"
_ROW_JOB_COLUMNS = "(img_a, id, y1, x1, y2, x2, img_b, dy, dx, resume, after)"


def _slots(fn, slots):
    if isinstance(slots, (bool, np.bool_)) or not isinstance(slots, (int, np.integer)) or not 1 <= int(slots) <= MAX_SLOTS:
        raise KGLibraryError(f"{fn}: slots {slots!r} must be an integer in 1 .. {MAX_SLOTS}")
    return int(slots)


class Overlaps:
    """Host CSR over the jobs: row k owns the entries indptr[k] .. indptr[k + 1] of values (ascending) and pixels; area, zero and outside
    have one entry per row.  All int64."""
    __slots__ = ("indptr", "values", "pixels", "area", "zero", "outside")

    def __init__(self, indptr, values, pixels, area, zero, outside):
        self.indptr = np.ascontiguousarray(indptr, np.int64).reshape(-1)
        self.values, self.pixels = (np.ascontiguousarray(a, np.int64).reshape(-1) for a in (values, pixels))
        self.area, self.zero, self.outside = (np.ascontiguousarray(a, np.int64).reshape(-1) for a in (area, zero, outside))
        k, m = len(self.values), len(self.indptr) - 1
        if m < 0 or self.indptr[0] != 0 or self.indptr[-1] != k or (np.diff(self.indptr) < 0).any() or len(self.pixels) != k \
                or any(len(a) != m for a in (self.area, self.zero, self.outside)):
            raise KGLibraryError(f"Overlaps: indptr of {len(self.indptr)} entries for {k} values, {len(self.pixels)} pixel counts and "
                                 f"{len(self.area)} / {len(self.zero)} / {len(self.outside)} row counts")

    @classmethod
    def from_lists(cls, lists):
        """lists: per row a (values, pixels, area, zero, outside) tuple"""
        indptr = np.zeros(len(lists) + 1, np.int64)
        np.cumsum([len(t[0]) for t in lists], out=indptr[1:])
        cat = [np.concatenate([np.asarray(t[c], np.int64) for t in lists]) if lists else np.zeros(0, np.int64) for c in range(2)]
        return cls(indptr, *cat, *[[t[c] for t in lists] for c in (2, 3, 4)])

    def __len__(self):
        return len(self.indptr) - 1

    def __eq__(self, other):
        return isinstance(other, Overlaps) and all(np.array_equal(getattr(self, k), getattr(other, k)) for k in self.__slots__)

    __hash__ = None

    def of(self, k):
        """(values, pixels) of row k"""
        a, b = int(self.indptr[k]), int(self.indptr[k + 1])
        return self.values[a:b], self.pixels[a:b]

    def rows(self):
        """int64 [len(values)]: the row every entry belongs to"""
        return np.repeat(np.arange(len(self), dtype=np.int64), np.diff(self.indptr))

    def pairs(self, ids=None):
        """int64 [k, 3] = (a, b, pixels), one row per entry in order.  ids: the own id of every row (default 1 .. m)."""
        own = np.arange(1, len(self) + 1, dtype=np.int64) if ids is None else np.asarray(ids, np.int64).reshape(-1)
        if len(own) != len(self):
            raise KGLibraryError(f"pairs: {len(own)} ids for {len(self)} rows")
        return np.stack([own[self.rows()], self.values, self.pixels], 1).reshape(-1, 3)

    def _area_b(self, fn, area_b):
        ab = np.asarray(area_b)
        if ab.ndim != 1 or ab.dtype.kind not in "iu":
            raise KGLibraryError(f"{fn}: area_b must be integers [n_b], the areas of the ids 1 .. n_b of the other map")
        if len(self.values) and (self.values.min() < 1 or self.values.max() > len(ab)):
            raise KGLibraryError(f"{fn}: partner values outside 1 .. {len(ab)}")
        return ab.astype(np.int64)[self.values - 1]

    def iou(self, area_b):
        """float64 [len(values)]: pixels / (area + area_b - pixels) of every entry; area_b: integers [n_b], the areas of the ids 1 .. n_b"""
        ab = self._area_b("iou", area_b)
        return self.pixels.astype(np.float64) / (self.area[self.rows()] + ab - self.pixels).astype(np.float64)

    def fraction_of_b(self, area_b):
        """float64 [len(values)]: pixels / area_b of every entry: how much of the partner lies under this row's pixels"""
        return self.pixels.astype(np.float64) / self._area_b("fraction_of_b", area_b).astype(np.float64)

    def slice(self, r0, r1):
        """The Overlaps of rows r0 .. r1 - 1"""
        a, b = int(self.indptr[r0]), int(self.indptr[r1])
        return Overlaps(self.indptr[r0:r1 + 1] - a, self.values[a:b], self.pixels[a:b], self.area[r0:r1], self.zero[r0:r1], self.outside[r0:r1])


# ---- host statements of the semantics ---------------------------------------------------------------------------------------------------

_NONE = (np.zeros(0, np.int64), np.zeros(0, np.int64), 0, 0, 0)


def _job_list(A, B, H, W, job):
    """Stacks A, B; one job (img_a, id, y1, x1, y2, x2, img_b, dy, dx) -> (values, pixels, area, zero, outside), values ascending"""
    ia, v, y1, x1, y2, x2, ib, dy, dx = job
    y1, x1, y2, x2 = max(y1, 0), max(x1, 0), min(y2, H), min(x2, W)
    if not (0 <= ia < len(A) and 0 <= ib < len(B)) or y2 <= y1 or x2 <= x1:
        return _NONE
    ys, xs = np.nonzero(A[ia, y1:y2, x1:x2] == v)
    if len(ys) == 0:
        return _NONE
    py, px = ys.astype(np.int64) + y1 + dy, xs.astype(np.int64) + x1 + dx
    inside = (py >= 0) & (py < H) & (px >= 0) & (px < W)
    got = B[ib, py[inside], px[inside]].astype(np.int64)
    values, pixels = np.unique(got[got != 0], return_counts=True)
    return values.astype(np.int64), pixels.astype(np.int64), len(ys), int(np.count_nonzero(got == 0)), int(len(ys) - np.count_nonzero(inside))


def _host_pair(fn, a, b):
    A, B = host_stack(fn, a, COUNTS_FIT), host_stack(fn, b, COUNTS_FIT)
    if A.shape[1:] != B.shape[1:]:
        raise KGLibraryError(f"{fn}: maps of {A.shape[1:]} and {B.shape[1:]} must have one size")
    return A, B


def overlaps_rows_host(a, b, jobs, slots):
    """kg_label_overlaps in NumPy: a, b integers [H, W] or [nimg, H, W] of one size; jobs integers [m, 11] = (img_a, id, y1, x1, y2, x2,
    img_b, dy, dx, resume, after) -> int64 [m, 5 + 2 slots] = {count, more, area, zero, outside, (value, pixels) x slots}, nothing split."""
    slots = _slots("overlaps_rows_host", slots)
    A, B = _host_pair("overlaps_rows_host", a, b)
    H, W = A.shape[1:]
    j = _labelmaps.host_jobs("overlaps_rows_host", jobs, 11, _ROW_JOB_COLUMNS).astype(np.int64)
    out = np.zeros((len(j), 5 + 2 * slots), np.int64)
    for k, row in enumerate(j.tolist()):
        values, pixels, area, zero, outside = _job_list(A, B, H, W, row[:9])
        if row[9]:
            keep = values > row[10]
            values, pixels = values[keep], pixels[keep]
        c = min(len(values), slots)
        out[k, :5] = c, len(values) > slots, area, zero, outside
        out[k, 5:5 + 2 * c] = np.stack([values[:c], pixels[:c]], 1).reshape(-1)
    return out


def _pair_table(fn, pairs, shift, nimg_a, nimg_b):
    """pairs / shift arguments -> int64 [k, 4] = (img_a, img_b, dy, dx)"""
    if pairs is None:
        if nimg_a != nimg_b:
            raise KGLibraryError(f"{fn}: stacks of {nimg_a} and {nimg_b} maps need pairs")
        p = np.stack([np.arange(nimg_a)] * 2, 1).astype(np.int64)
    else:
        p = np.asarray(pairs)
        if p.ndim != 2 or p.shape[1] != 2 or p.dtype.kind not in "iu" or (p.size and (p.min() < 0 or (p >= [nimg_a, nimg_b]).any())):
            raise KGLibraryError(f"{fn}: pairs must be integers [k, 2] = (img_a, img_b) inside the stacks of {nimg_a} and {nimg_b} maps")
        p = p.astype(np.int64)
    s = np.zeros((1, 2), np.int64) if shift is None else np.asarray(shift)
    if s.dtype.kind not in "iu" or s.shape not in ((2,), (len(p), 2), (1, 2)) or (s.size and (s.min() < -2 ** 31 or s.max() > 2 ** 31 - 1)):
        raise KGLibraryError(f"{fn}: shift must be integers (dy, dx) that fit int32, or one such pair per pair of maps [{len(p)}, 2]")
    return np.concatenate([p, np.broadcast_to(s.astype(np.int64).reshape(-1, 2), (len(p), 2))], 1).reshape(-1, 4)


def _per_map_stats(fn, maps, n, stats, stats_of):
    """n (one per map of the stack) and stats (None: from stats_of) -> (counts, per map int64 [n, 5])"""
    nimg = len(maps)
    ns = _labelmaps.counts(fn, n, nimg)
    if stats is None:
        per = [np.asarray(stats_of(maps[i], ns[i]), np.int64).reshape(-1, 5) for i in range(nimg)]
    else:
        per = [stats] if nimg == 1 and np.ndim(stats) == 2 else list(stats)
        per = [s.cpu().numpy() if _labelmaps.is_device(s) else np.asarray(s) for s in per]
        if len(per) != nimg or any(s.ndim != 2 or s.shape != (k, 5) or s.dtype.kind not in "iu" for s, k in zip(per, ns)):
            raise KGLibraryError(f"{fn}: stats must be integers [n, 5] per label map ({nimg} map(s), counts {ns})")
        per = [s.astype(np.int64) for s in per]
    return ns, per


def _jobs_of_pairs(per, pt):
    """per map of a its stats, pt [k, 4] -> int64 [m, 6]: pair after pair the ids 1 .. n[img_a] inside their own boxes, column 0 the pair"""
    return np.concatenate([_labelmaps.jobs_from_stats(per[int(ia)], k) for k, ia in enumerate(pt[:, 0])] + [np.zeros((0, 6), np.int32)]).astype(np.int64)


def _full_jobs(fn, j, pt, H, W):
    """[m, 6] with column 0 naming the pair, or [m, 9] -> int64 [m, 9], boxes clamped to the map (so that a band rule sees the pixels a job
    really holds); a job of a pair that does not exist gets image indices of -1, hence its row of zeros"""
    j = np.asarray(j)
    if j.ndim == 2 and j.shape[1] == 9:
        full = _labelmaps.host_jobs(fn, j, 9, _JOB_COLUMNS).astype(np.int64)
    else:
        j6 = _labelmaps.host_jobs(fn, j, 6, "(pair, id, y1, x1, y2, x2), or " + _JOB_COLUMNS).astype(np.int64)
        ok = (j6[:, 0] >= 0) & (j6[:, 0] < len(pt))
        sel = pt[np.where(ok, j6[:, 0], 0)] if len(pt) else np.zeros((len(j6), 4), np.int64)
        sel = np.where(ok[:, None], sel, [-1, -1, 0, 0])
        full = np.concatenate([sel[:, :1], j6[:, 1:], sel[:, 1:]], 1)
    full = full.copy().reshape(-1, 9)
    full[:, 2:4] = np.clip(full[:, 2:4], 0, [H, W]); full[:, 4:6] = np.clip(full[:, 4:6], 0, [H, W])
    return full


def _job_args(fn, maps, nimg_b, n, jobs, stats, pairs, shift, stats_of):
    """The n / jobs / stats / pairs / shift arguments -> int64 [m, 9]"""
    nimg, H, W = maps.shape
    if jobs is not None:
        if n is not None or stats is not None:
            raise KGLibraryError(f"{fn}: jobs cannot be given together with n / stats")
        jobs = jobs.cpu().numpy() if _labelmaps.is_device(jobs) else np.asarray(jobs)
        nine = jobs.ndim == 2 and jobs.shape[1] == 9
        if nine and (pairs is not None or shift is not None):
            raise KGLibraryError(f"{fn}: a job table {_JOB_COLUMNS} carries its own pairs and shifts")
        return _full_jobs(fn, jobs if jobs.size or nine else np.zeros((0, 6), np.int64), None if nine else _pair_table(fn, pairs, shift, nimg, nimg_b), H, W)
    if n is None:
        raise KGLibraryError(f"{fn}: the instance count n or a job table is needed")
    pt = _pair_table(fn, pairs, shift, nimg, nimg_b)
    return _full_jobs(fn, _jobs_of_pairs(_per_map_stats(fn, maps, n, stats, stats_of)[1], pt), pt, H, W)


def overlaps_host(a, b, jobs_or_n, pairs=None, shift=None):
    """a, b: integers [H, W] or [nimg, H, W] of one size (b may be a); jobs_or_n: a job table [m, 9] or [m, 6], or the instance count n
    (one per map of a): the ids 1 .. n inside their own boxes (labelmetrics.label_stats_host), pair after pair; pairs, shift: see the
    module text -> Overlaps, one row per job: the full sorted list, not paged and not banded."""
    A, B = _host_pair("overlaps_host", a, b)
    H, W = A.shape[1:]
    is_table = np.ndim(jobs_or_n) == 2 or (np.ndim(jobs_or_n) == 1 and np.size(jobs_or_n) == 0)
    j = _job_args("overlaps_host", A, len(B), None if is_table else jobs_or_n, jobs_or_n if is_table else None, None, pairs, shift,
                  labelmetrics.label_stats_host)
    return Overlaps.from_lists([_job_list(A, B, H, W, row) for row in j.tolist()])


# ---- the pager and merger ---------------------------------------------------------------------------------------------------------------

def paged(row_fn, jobs, H, W, slots, max_job_pixels=65536):
    """jobs: integers [m, 9], for maps of H x W -> Overlaps with m rows, through rows of `slots` slots.
    row_fn(table): host int64 [k, 11] = (img_a, id, y1, x1, y2, x2, img_b, dy, dx, resume, after) -> the k rows, integers
    [k, 5 + 2 slots] (overlaps_rows_host, or overlaps_rows copied back).  The jobs are clamped and split into bands (split_jobs); all
    pieces go through row_fn once, and that round gives area, zero and outside; the pieces whose `more` is 1 go again with resume = 1 and
    after = their last value, until none is left; the entries of the pieces of a job are merged by value, pixels added.  Columns 9 and 10
    belong to the pager."""
    slots = _slots("overlaps", slots)
    j = np.array(jobs, np.int64).reshape(-1, 9)
    j[:, 2:4] = np.clip(j[:, 2:4], 0, [H, W]); j[:, 4:6] = np.clip(j[:, 4:6], 0, [H, W])
    pieces, owner = split_jobs(j[:, :6], max_job_pixels)
    table = np.zeros((len(pieces), 11), np.int64)
    table[:, :6], table[:, 6:9] = pieces, j[owner, 6:9]
    active = np.arange(len(pieces))
    head = np.zeros((len(j), 3), np.int64)                            # area, zero, outside: the first round's, added over the pieces
    found = []                                                        # per round: owner, value, pixels of the slots filled
    first = True
    while len(active):
        rows = np.asarray(row_fn(table[active])).astype(np.int64).reshape(len(active), 5 + 2 * slots)
        cnt, more = rows[:, 0], rows[:, 1] != 0
        ent = rows[:, 5:].reshape(len(active), slots, 2)
        filled = np.arange(slots)[None] < cnt[:, None]
        last = ent[np.arange(len(active)), np.maximum(cnt, 1) - 1, 0]
        if (cnt < 0).any() or (cnt > slots).any() or (more & (cnt == 0)).any() or (more & (table[active, 9] != 0) & (last <= table[active, 10])).any():
            raise KGLibraryError("overlaps: a row that cannot be paged (count outside 0 .. slots, or `more` without progress)")
        if first:
            np.add.at(head, owner[active], rows[:, 2:5])
            first = False
        found.append(np.concatenate([np.broadcast_to(owner[active][:, None], filled.shape)[filled][:, None], ent[filled]], 1))
        table[active[more], 9], table[active[more], 10] = 1, last[more]
        active = active[more]
    e = np.concatenate(found) if found else np.zeros((0, 3), np.int64)
    e = e[np.lexsort((e[:, 1], e[:, 0]))]
    lead = np.ones(len(e), bool)
    lead[1:] = (e[1:, 0] != e[:-1, 0]) | (e[1:, 1] != e[:-1, 1])
    at = np.flatnonzero(lead)
    sums = np.add.reduceat(e[:, 2], at) if len(at) else np.zeros(0, np.int64)
    indptr = np.zeros(len(j) + 1, np.int64)
    np.cumsum(np.bincount(e[at, 0], minlength=len(j)), out=indptr[1:])
    return Overlaps(indptr, e[at, 1], sums, head[:, 0], head[:, 1], head[:, 2])


# ---- device -----------------------------------------------------------------------------------------------------------------------------

def _device_pair(fn, a, b):
    A = device_stack(fn, a, COUNTS_FIT)[0]
    B = A if b is a else device_stack(fn, b, COUNTS_FIT)[0]
    if A.shape[1:] != B.shape[1:] or A.device != B.device:
        raise KGLibraryError(f"{fn}: maps of {tuple(A.shape[1:])} and {tuple(B.shape[1:])} must have one size and one device")
    return A, B


def overlaps_rows(a, b, jobs, slots):
    """kg_label_overlaps as it is: a, b device int32 [H, W] or [nimg, H, W] of one size (b may be a); jobs host integers [m, 11] =
    (img_a, id, y1, x1, y2, x2, img_b, dy, dx, resume, after) (uploaded once) or a device int32 tensor -> device int64 [m, 5 + 2 slots].
    One launch, no copy back, no synchronisation, nothing split."""
    import torch
    from ._lib import ptr, stream_ptr
    slots = _slots("overlaps", slots)
    A, B = _device_pair("overlaps", a, b)
    jd = _labelmaps.device_jobs("overlaps", jobs, 11, _ROW_JOB_COLUMNS, A.device)
    m = jd.shape[0]
    out = torch.empty(m, 5 + 2 * slots, dtype=torch.int64, device=A.device)
    with torch.cuda.device(A.device):
        _lib.call("kg_label_overlaps", ptr(A), A.shape[0], ptr(B), B.shape[0], A.shape[1], A.shape[2], ptr(jd) if m else None, m, slots,
                  ptr(out) if m else None, stream_ptr())
    return out


def _device_lists(A, B, j, slots, max_job_pixels):
    """A, B: device int32 stacks, j: host jobs [m, 9] -> Overlaps.  One launch, one upload and one copy back per round."""
    return paged(lambda table: overlaps_rows(A, B, table, slots).cpu().numpy(), j, A.shape[1], A.shape[2], slots, max_job_pixels)


def overlaps(a, b, n=None, jobs=None, stats=None, pairs=None, shift=None, slots=8, max_job_pixels=65536):
    """overlaps_host on the device -> Overlaps (host).  a, b: device int32 [H, W] or [nimg, H, W] of one size; b may be a.  What is listed:
      jobs   integers [m, 9] = (img_a, id, y1, x1, y2, x2, img_b, dy, dx), or [m, 6] = (pair, id, y1, x1, y2, x2) with pairs / shift; on
             the host, or a device int32 tensor (copied back once: the bands are cut on the host); or
      n      the instance count (one per map of a): pair after pair the ids 1 .. n[img_a] inside their own boxes.  The boxes come from
             stats -- integers [n, 5] = (area, y1, x1, y2, x2), host or device, one table per map for a stack; columns 1:6 of an
             Instances table are that -- or, without stats, from labelmetrics.label_stats (its launches and one copy per map).
    A job whose box holds more than max_job_pixels pixels is listed in bands.  ONE kg_label_overlaps launch, one upload and one
    device -> host copy for all pieces and all pairs, then one more of each per round for the pieces that have more than `slots` partner
    values left (paged): with the default 8 slots consecutive frames need one round."""
    slots = _slots("overlaps", slots)
    A, B = _device_pair("overlaps", a, b)
    j = _job_args("overlaps", A, B.shape[0], n, jobs, stats, pairs, shift, labelmetrics.label_stats)
    return _device_lists(A, B, j, slots, _labelmaps.check_cap("overlaps", max_job_pixels))


# ---- links ------------------------------------------------------------------------------------------------------------------------------

Links = namedtuple("Links", "successor parent linked divided")
Links.__doc__ = """successor int64 [n_a]: the sole child of every a (0: none, or a division); parent int64 [n_b]: the a every b is linked to or
the child of (0: a birth); linked bool [n_b]: the parent came from the one-to-one IoU step; divided bool [n_a]: two or more children."""


def link(ov, area_b, min_iou=0.3, min_child=0.5):
    """ov: Overlaps whose row k is the id k + 1 of map a against ONE map b with ids 1 .. n_b; area_b: integers [n_b] -> Links (module text:
    `link`).  min_child=None turns the child rule off."""
    if not isinstance(ov, Overlaps):
        raise KGLibraryError("link: an Overlaps")
    n_a, n_b = len(ov), len(np.asarray(area_b).reshape(-1))
    iou = ov.iou(area_b)
    a, b = ov.rows() + 1, ov.values
    parent = np.zeros(n_b, np.int64)
    taken, linked = np.zeros(n_a, bool), np.zeros(n_b, bool)
    for k in np.lexsort((b, a, -iou)):
        if iou[k] < min_iou:
            break
        if not taken[a[k] - 1] and not linked[b[k] - 1]:
            parent[b[k] - 1], taken[a[k] - 1], linked[b[k] - 1] = a[k], True, True
    if min_child is not None:
        frac = ov.fraction_of_b(area_b)
        seen = np.zeros(n_b, bool)
        for k in np.lexsort((a, -ov.pixels, b)):                      # per b the entry with the most pixels first, ties to the smallest a
            if not seen[b[k] - 1]:
                seen[b[k] - 1] = True
                if parent[b[k] - 1] == 0 and frac[k] >= min_child:
                    parent[b[k] - 1] = a[k]
    children = np.bincount(parent[parent > 0] - 1, minlength=n_a)
    successor = np.zeros(n_a, np.int64)
    sole = np.flatnonzero(parent > 0)
    sole = sole[children[parent[sole] - 1] == 1]
    successor[parent[sole] - 1] = sole + 1
    return Links(successor, parent, linked, children >= 2)


# ---- tracks -----------------------------------------------------------------------------------------------------------------------------

TRACK_COLUMNS = ("track", "first", "last", "parent", "frames")


class Tracks:
    """labels: the stack relabelled by track id ([T, H, W], host array or device tensor as the route gave it); track_of: per frame t an
    int64 [n_t + 1] with track_of[t][id] the track of id (0 for id 0 and for an id without pixels); table int64 [K, 5] (TRACK_COLUMNS):
    row k - 1 is track k, its first and last frame, the track it split off from (0: none) and the number of frames it lives in."""
    __slots__ = ("labels", "track_of", "table")

    def __init__(self, labels, track_of, table):
        self.labels, self.track_of = labels, [np.asarray(t, np.int64) for t in track_of]
        self.table = np.ascontiguousarray(table, np.int64).reshape(-1, 5)

    def __len__(self):
        return len(self.table)

    def lineage(self):
        """Per track the chain of its ancestors, oldest first, the track itself last: [[1], [2], [3], [3, 5], ...]"""
        out = []
        for k, p in zip(self.table[:, 0].tolist(), self.table[:, 3].tolist()):
            out.append((out[p - 1] if p else []) + [k])               # a parent's id is smaller than its child's: it starts earlier
        return out


def _assign_tracks(ov, pair_rows, ns, areas, min_iou, min_child):
    """ov: the Overlaps of all T - 1 consecutive pairs (pair_rows[t] .. pair_rows[t + 1] the rows of pair t) -> (track_of, table)"""
    T = len(ns)
    track_of = [np.zeros(k + 1, np.int64) for k in ns]
    table = []

    def start(t, ident, parent):
        table.append([len(table) + 1, t, t, parent, 1])
        track_of[t][ident] = len(table)
    for ident in np.flatnonzero(areas[0] > 0) + 1:
        start(0, int(ident), 0)
    for t in range(T - 1):
        lk = link(ov.slice(int(pair_rows[t]), int(pair_rows[t + 1])), areas[t + 1], min_iou, min_child)
        for ident in (np.flatnonzero(areas[t + 1] > 0) + 1).tolist():
            p = int(lk.parent[ident - 1])
            if p and not lk.divided[p - 1]:
                k = int(track_of[t][p])
                track_of[t + 1][ident] = k
                table[k - 1][2], table[k - 1][4] = t + 1, table[k - 1][4] + 1
            else:
                start(t + 1, ident, int(track_of[t][p]) if p else 0)
    return track_of, np.asarray(table, np.int64).reshape(-1, 5)


def _remap_tables(ns, track_of):
    start = np.zeros(len(ns) + 1, np.int64)
    np.cumsum(ns, out=start[1:])
    return start, np.concatenate([t[1:] for t in track_of] + [np.zeros(0, np.int64)])


def track_host(stack, counts, shift=None, min_iou=0.3, min_child=0.5):
    """stack: integers [T, H, W], frame t with the ids 1 .. counts[t]; shift: None, (dy, dx) or one per consecutive pair [T - 1, 2]: the
    drift from frame t to t + 1 -> Tracks (module text: `tracks`), labels a host int32 array."""
    maps = host_stack("track_host", stack, COUNTS_FIT)
    T = len(maps)
    ns, per = _per_map_stats("track_host", maps, counts, None, labelmetrics.label_stats_host)
    pairs = np.stack([np.arange(T - 1), np.arange(1, T)], 1)
    ov = overlaps_host(maps, maps, ns, pairs, shift) if T > 1 else Overlaps.from_lists([])
    pair_rows = np.concatenate([[0], np.cumsum(ns[:-1])]).astype(np.int64)
    track_of, table = _assign_tracks(ov, pair_rows, ns, [s[:, 0] for s in per], min_iou, min_child)
    out = np.zeros(maps.shape, np.int32)
    for t in range(T):
        ok = (maps[t] >= 1) & (maps[t] <= ns[t])
        out[t][ok] = track_of[t][maps[t][ok]]
    return Tracks(out, track_of, table)


def _device_stats(fn, lab, ns):
    """label_stats_device of every frame, ONE copy back for all of them -> per frame int64 [n, 5]; raises on a pixel outside [0, n]"""
    import torch
    parts = [labelmetrics.label_stats_device(lab[t], ns[t]) for t in range(len(ns))]
    flat = torch.cat([p.reshape(-1) for pair in parts for p in pair]).cpu().numpy().astype(np.int64)
    per, at = [], 0
    for t, k in enumerate(ns):
        per.append(flat[at:at + 5 * k].reshape(-1, 5))
        if flat[at + 5 * k]:
            raise KGLibraryError(f"{fn}: {int(flat[at + 5 * k])} pixel(s) of frame {t} lie outside [0, {k}]")
        at += 5 * k + 1
    return per


def track(stack, counts, shift=None, stats=None, min_iou=0.3, min_child=0.5, slots=8, max_job_pixels=65536):
    """track_host on the device: stack device int32 [T, H, W] -> Tracks with labels a device int32 [T, H, W].  stats: per frame integers
    [n, 5] = (area, y1, x1, y2, x2) (columns 1:6 of an Instances table); without them kg_label_stats runs per frame and ONE copy brings
    all tables back.  ONE kg_label_overlaps launch covers all T - 1 consecutive pairs (one more per round of paging), the host links
    pair by pair, and components.remap relabels the whole stack in one call."""
    from . import components
    slots = _slots("track", slots)
    lab = device_stack("track", stack, COUNTS_FIT)[0]
    T = lab.shape[0]
    ns = _labelmaps.counts("track", counts, T)
    per = _device_stats("track", lab, ns) if stats is None else _per_map_stats("track", lab, ns, stats, None)[1]
    pairs = np.stack([np.arange(T - 1), np.arange(1, T)], 1)
    ov = overlaps(lab, lab, n=ns, stats=per, pairs=pairs, shift=shift, slots=slots, max_job_pixels=max_job_pixels) if T > 1 \
        else Overlaps.from_lists([])
    pair_rows = np.concatenate([[0], np.cumsum(ns[:-1])]).astype(np.int64)
    track_of, table = _assign_tracks(ov, pair_rows, ns, [s[:, 0] for s in per], min_iou, min_child)
    return Tracks(components.remap(lab, *_remap_tables(ns, track_of)), track_of, table)


def track_instances(insts, shift=None, min_iou=0.3, min_child=0.5, slots=8, max_job_pixels=65536):
    """track for a list of equal-sized Instances / TiledInstances (the frames, in order): ids 1 .. len(inst), areas and boxes from the
    tables, so no stats launch.  Label maps that are not on a GPU device go through track_host."""
    import torch
    insts = list(insts)
    if not insts:
        raise KGLibraryError("track_instances: no frames")
    for v in insts:
        _labelmaps.check_instances("track_instances", v)
    if len({tuple(v.labels.shape) for v in insts}) != 1:
        raise KGLibraryError("track_instances: the frames must have one size")
    ns = [len(v) for v in insts]
    if not all(_labelmaps.is_device(v.labels) for v in insts):
        return track_host(np.stack([_labelmaps.host_labels(v) if not _labelmaps.is_device(v.labels) else v.labels.cpu().numpy() for v in insts]),
                          ns, shift, min_iou, min_child)
    stats = [_labelmaps.instance_stats("track_instances", v) for v in insts]
    return track(torch.stack([v.labels for v in insts]), ns, shift, stats, min_iou, min_child, slots, max_job_pixels)


def stitch_planes(stack, counts, min_iou=0.25, slots=8, max_job_pixels=65536):
    """The planes of a z-stack, each segmented on its own (plane z with the ids 1 .. counts[z]), as ONE label volume: an object of plane
    z + 1 takes the id of the object of plane z it is linked to one-to-one at iou >= min_iou -- track with the child rule off, so nothing
    divides and a volume id never forks -> Tracks; its labels is the volume (device int32 [Z, H, W], or a host array for a host stack)."""
    if _labelmaps.is_device(stack):
        return track(stack, counts, None, None, min_iou, None, slots, max_job_pixels)
    return track_host(stack, counts, None, min_iou, None)


# ---- child / parent relations -----------------------------------------------------------------------------------------------------------

Relations = namedtuple("Relations", "parent fraction children")
Relations.__doc__ = """parent int64 [n_children]: the parent id that holds the most pixels of every child (ties: the smallest; 0: none);
fraction float64 [n_children]: the share of the child's pixels inside that parent; children int64 [n_parents]: the child count."""


def _relations(ov, n_parents):
    if len(ov.values) and (ov.values.min() < 1 or ov.values.max() > n_parents):
        raise KGLibraryError(f"relate: parent values outside 1 .. {n_parents}")
    rows = ov.rows()
    parent, fraction = np.zeros(len(ov), np.int64), np.zeros(len(ov), np.float64)
    order = np.lexsort((ov.values, -ov.pixels, rows))                 # per child the most pixels first, ties to the smallest parent
    best = order[np.flatnonzero(np.concatenate([[True], rows[order][1:] != rows[order][:-1]]))] if len(order) else order
    parent[rows[best]] = ov.values[best]
    fraction[rows[best]] = ov.pixels[best].astype(np.float64) / ov.area[rows[best]].astype(np.float64)
    return Relations(parent, fraction, np.bincount(parent[parent > 0] - 1, minlength=n_parents).astype(np.int64))


def relate_host(children, parents, n_children, n_parents):
    """children, parents: integer maps [H, W] of one size with the ids 1 .. n_children / 1 .. n_parents -> Relations"""
    return _relations(overlaps_host(children, parents, int(n_children)), _labelmaps.counts("relate_host", n_parents, 1)[0])


def relate(children, parents, n_children, n_parents, stats=None, slots=8, max_job_pixels=65536):
    """relate_host on the device (CellProfiler's RelateObjects): device int32 maps [H, W]; stats: the children's [n, 5] table when the
    caller has it -> Relations (host)."""
    return _relations(overlaps(children, parents, n=int(n_children), stats=stats, slots=slots, max_job_pixels=max_job_pixels),
                      _labelmaps.counts("relate", n_parents, 1)[0])
