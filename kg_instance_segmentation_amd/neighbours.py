"""The touching-neighbour graph of a label map: which instances touch which, and along how many pixel sides and corners, without copying
the map back.

components.py cleans a label map, labelmetrics.py scores it, measure.py measures every instance on its own and distance.py grows, shrinks
and inscribes it.  This module answers how the instances relate: neighbour counts, who touches whom, the contact length per pair -- and,
on expand_labels' regions, the "touching after expansion" graph, whose contact length is the length of the shared Voronoi border.  The
device lists the neighbours of every instance in ascending order (kg_label_neighbours, csrc/neighbours.hip), a few thousand integers come
back, and the host builds a CSR structure over them.

    neighbours_rows_host  the row semantics in NumPy, resume / after / more included (the yardstick of the raw entry)
    neighbours_rows       kg_label_neighbours as it is: ONE launch, rows stay on the device
    neighbours_host       the graph in NumPy, stated directly: per job the full sorted list, nothing paged, nothing split
    neighbours            the same graph from a device map: bands, one launch per round of paging, merged on the host
    paged                 the pager and merger both routes share; it takes the row function as an argument
    Neighbours            host CSR over the jobs: indptr, values, sides, corners; degree(), of(k), pairs(), contact_length()
    neighbours_instances  neighbours for an Instances / TiledInstances (ids 1 .. n, boxes from its table), optionally after expansion

Semantics (include/kgnet_hip.h is the normative text)
  job         {img, id, y1, x1, y2, x2}: a half-open box, clamped to the map.  P = the pixels of the box in image img with labels == id.
  sides[v]    the (pixel of P, direction up / down / left / right) pairs whose neighbour lies INSIDE THE MAP and holds v, v != id, v != 0
  corners[v]  under connectivity 8 the same over the four diagonal directions; under 4 it is 0 and the diagonals are never read
  neighbours  {v : sides[v] + corners[v] > 0}, listed in ascending signed order.  They are read from the MAP, never from the box: a box
              edge or band edge inside the map is not an object edge, as in measure.py.
  values      are compared only: INT_MIN, -1 and INT_MAX are ordinary neighbour values; id may be any value, 0 included.
  row         int64 [2 + 3 slots] = {count, more, (value, sides, corners) x slots} of a job {..., resume, after}: with resume != 0 only the
              values > after are listed (after is ignored when resume == 0); count = the slots filled; more = 1 exactly when a further
              qualifying value exists beyond the last one written; unused slots are zeros.
  bad jobs    an image index outside [0, nimg), an empty or inverted box, an id the box does not hold: a row of zeros.
  sizes       H, W <= 32768 as in measure.py, so a count stays below 2^33; 1 <= slots <= 64.
  bands       a job whose clamped box holds more than max_job_pixels pixels is split as labelmetrics.split_jobs does; every piece is
              paged on its own, and the pieces of a job are merged by value: sides and corners add."""
import math

import numpy as np

from . import _lib, _labelmaps, distance, labelmetrics
from ._labelmaps import MAX_SIDE, device_stack, host_stack  # noqa: F401  (MAX_SIDE: public here)
from .labelmetrics import split_jobs

KGLibraryError = _lib.KGLibraryError
COUNTS_FIT = "the bound that keeps every count inside int64"       # what the side bound protects here
MAX_SLOTS = 64
_JOB_COLUMNS = "(img, id, y1, x1, y2, x2)"
_ROW_JOB_COLUMNS = "(img, id, y1, x1, y2, x2, resume, after)"
_SIDES = ((-1, 0), (1, 0), (0, -1), (0, 1))
_CORNERS = ((-1, -1), (-1, 1), (1, -1), (1, 1))


def _connectivity(fn, connectivity):
    if isinstance(connectivity, (bool, np.bool_)) or connectivity not in (4, 8):
        raise KGLibraryError(f"{fn}: connectivity {connectivity!r} must be 4 or 8")
    return int(connectivity)


def _slots(fn, slots):
    if isinstance(slots, (bool, np.bool_)) or not isinstance(slots, (int, np.integer)) or not 1 <= int(slots) <= MAX_SLOTS:
        raise KGLibraryError(f"{fn}: slots {slots!r} must be an integer in 1 .. {MAX_SLOTS}")
    return int(slots)


class Neighbours:
    """Host CSR over the jobs (or the instances): row k owns the entries indptr[k] .. indptr[k + 1] of values (ascending), sides and
    corners, all int64."""
    __slots__ = ("indptr", "values", "sides", "corners")

    def __init__(self, indptr, values, sides, corners):
        self.indptr = np.ascontiguousarray(indptr, np.int64).reshape(-1)
        self.values, self.sides, self.corners = (np.ascontiguousarray(a, np.int64).reshape(-1) for a in (values, sides, corners))
        k = len(self.values)
        if len(self.indptr) < 1 or self.indptr[0] != 0 or self.indptr[-1] != k or (np.diff(self.indptr) < 0).any() \
                or len(self.sides) != k or len(self.corners) != k:
            raise KGLibraryError(f"Neighbours: indptr of {len(self.indptr)} entries ending at {self.indptr[-1] if len(self.indptr) else None} "
                                 f"for {k} values, {len(self.sides)} sides and {len(self.corners)} corners")

    @classmethod
    def from_lists(cls, lists):
        """lists: per row a (values, sides, corners) triple"""
        indptr = np.zeros(len(lists) + 1, np.int64)
        np.cumsum([len(t[0]) for t in lists], out=indptr[1:])
        cat = [np.concatenate([np.asarray(t[c], np.int64) for t in lists]) if lists else np.zeros(0, np.int64) for c in range(3)]
        return cls(indptr, *cat)

    def __len__(self):
        return len(self.indptr) - 1

    def __eq__(self, other):
        return isinstance(other, Neighbours) and all(np.array_equal(getattr(self, k), getattr(other, k)) for k in self.__slots__)

    __hash__ = None

    def degree(self):
        """int64 [m]: the number of neighbours of every row"""
        return np.diff(self.indptr)

    def of(self, k):
        """(values, sides, corners) of row k"""
        a, b = int(self.indptr[k]), int(self.indptr[k + 1])
        return self.values[a:b], self.sides[a:b], self.corners[a:b]

    def rows(self):
        """int64 [len(values)]: the row every entry belongs to"""
        return np.repeat(np.arange(len(self), dtype=np.int64), self.degree())

    def contact_length(self):
        """int64 [m]: sides summed per row -- measure's edges_contact of the same job"""
        out = np.zeros(len(self), np.int64)
        np.add.at(out, self.rows(), self.sides)
        return out

    def pairs(self, ids=None):
        """int64 [k, 4] = (a, b, sides, corners) with a < b, every undirected pair once: the entries of the rows whose own id is the smaller
        one.  ids: the own id of every row (default 1 .. m, the usual case of an instance map)."""
        own = np.arange(1, len(self) + 1, dtype=np.int64) if ids is None else np.asarray(ids, np.int64).reshape(-1)
        if len(own) != len(self):
            raise KGLibraryError(f"pairs: {len(own)} ids for {len(self)} rows")
        a = own[self.rows()]
        keep = a < self.values
        return np.stack([a[keep], self.values[keep], self.sides[keep], self.corners[keep]], 1).reshape(-1, 4)

    def slice(self, r0, r1):
        """The Neighbours of rows r0 .. r1 - 1"""
        a, b = int(self.indptr[r0]), int(self.indptr[r1])
        return Neighbours(self.indptr[r0:r1 + 1] - a, self.values[a:b], self.sides[a:b], self.corners[a:b])


# ---- host statements of the semantics ---------------------------------------------------------------------------------------------------

_NONE = (np.zeros(0, np.int64),) * 3


def _job_list(lab, H, W, job, connectivity):
    """One map [H, W], one job (id, y1, x1, y2, x2) -> the full (values, sides, corners), values ascending"""
    v, y1, x1, y2, x2 = job
    y1, x1, y2, x2 = max(y1, 0), max(x1, 0), min(y2, H), min(x2, W)
    if y2 <= y1 or x2 <= x1:
        return _NONE
    ys, xs = np.nonzero(lab[y1:y2, x1:x2] == v)
    if len(ys) == 0:
        return _NONE
    ys, xs = ys.astype(np.int64) + y1, xs.astype(np.int64) + x1

    def tally(directions):
        seen = []
        for dy, dx in directions:
            ny, nx = ys + dy, xs + dx
            inside = (ny >= 0) & (ny < H) & (nx >= 0) & (nx < W)
            nb = lab[ny[inside], nx[inside]].astype(np.int64)
            seen.append(nb[(nb != v) & (nb != 0)])
        return np.unique(np.concatenate(seen), return_counts=True)
    sv, sc = tally(_SIDES)
    cv, cc = tally(_CORNERS) if connectivity == 8 else _NONE[:2]
    values = np.union1d(sv, cv).astype(np.int64)
    sides, corners = np.zeros(len(values), np.int64), np.zeros(len(values), np.int64)
    sides[np.searchsorted(values, sv)] = sc
    corners[np.searchsorted(values, cv)] = cc
    return values, sides, corners


def neighbours_rows_host(labels, jobs, slots, connectivity=4):
    """kg_label_neighbours in NumPy: labels integers [H, W] or [nimg, H, W]; jobs integers [m, 8] = (img, id, y1, x1, y2, x2, resume, after)
    -> int64 [m, 2 + 3 slots] = {count, more, (value, sides, corners) x slots}, nothing split."""
    connectivity, slots = _connectivity("neighbours_rows_host", connectivity), _slots("neighbours_rows_host", slots)
    maps = host_stack("neighbours_rows_host", labels, COUNTS_FIT)
    nimg, H, W = maps.shape
    j = _labelmaps.host_jobs("neighbours_rows_host", jobs, 8, _ROW_JOB_COLUMNS).astype(np.int64)
    out = np.zeros((len(j), 2 + 3 * slots), np.int64)
    for k, (i, v, y1, x1, y2, x2, resume, after) in enumerate(j.tolist()):
        if not 0 <= i < nimg:
            continue
        values, sides, corners = _job_list(maps[i], H, W, (v, y1, x1, y2, x2), connectivity)
        if resume:
            keep = values > after
            values, sides, corners = values[keep], sides[keep], corners[keep]
        c = min(len(values), slots)
        out[k, 0], out[k, 1] = c, len(values) > slots
        out[k, 2:2 + 3 * c] = np.stack([values[:c], sides[:c], corners[:c]], 1).reshape(-1)
    return out


def neighbours_host(labels, jobs_or_n, connectivity=4):
    """labels: integers [H, W] or [nimg, H, W]; jobs_or_n: jobs [m, 6] = (img, id, y1, x1, y2, x2), or the instance count n (one per map
    for a stack): the ids 1 .. n inside their own boxes (labelmetrics.label_stats_host, which raises when a pixel lies outside [0, n])
    -> Neighbours, one row per job: the full sorted list, not paged and not banded."""
    connectivity = _connectivity("neighbours_host", connectivity)
    maps = host_stack("neighbours_host", labels, COUNTS_FIT)
    nimg, H, W = maps.shape
    j = _labelmaps.host_job_table("neighbours_host", maps, jobs_or_n, labelmetrics.label_stats_host)
    return Neighbours.from_lists([_job_list(maps[i], H, W, rest, connectivity) if 0 <= i < nimg else _NONE for i, *rest in j.tolist()])


# ---- the pager and merger ---------------------------------------------------------------------------------------------------------------

def paged(row_fn, jobs, H, W, slots, max_job_pixels=65536):
    """jobs: integers [m, 6], for maps of H x W -> Neighbours with m rows, through rows of `slots` slots.
    row_fn(table): host int64 [k, 8] = (img, id, y1, x1, y2, x2, resume, after) -> the k rows, integers [k, 2 + 3 slots]
    (neighbours_rows_host, or neighbours_rows copied back).  The jobs are clamped and split into bands (split_jobs); all pieces go
    through row_fn once; the pieces whose `more` is 1 go again with resume = 1 and after = their last value, until none is left; the
    entries of the pieces of a job are merged by value, sides and corners added.  Columns 6 and 7 belong to the pager."""
    slots = _slots("neighbours", slots)
    j = np.array(jobs, np.int64).reshape(-1, 6)
    j[:, 2:4] = np.clip(j[:, 2:4], 0, [H, W]); j[:, 4:6] = np.clip(j[:, 4:6], 0, [H, W])
    pieces, owner = split_jobs(j, max_job_pixels)
    table = np.zeros((len(pieces), 8), np.int64)
    table[:, :6] = pieces
    active = np.arange(len(pieces))
    found = []                                                        # per round: owner, value, sides, corners of the slots filled
    while len(active):
        rows = np.asarray(row_fn(table[active])).astype(np.int64).reshape(len(active), 2 + 3 * slots)
        cnt, more = rows[:, 0], rows[:, 1] != 0
        ent = rows[:, 2:].reshape(len(active), slots, 3)
        filled = np.arange(slots)[None] < cnt[:, None]
        last = ent[np.arange(len(active)), np.maximum(cnt, 1) - 1, 0]
        if (cnt < 0).any() or (cnt > slots).any() or (more & (cnt == 0)).any() or (more & (table[active, 6] != 0) & (last <= table[active, 7])).any():
            raise KGLibraryError("neighbours: a row that cannot be paged (count outside 0 .. slots, or `more` without progress)")
        found.append(np.concatenate([np.broadcast_to(owner[active][:, None], filled.shape)[filled][:, None], ent[filled]], 1))
        table[active[more], 6], table[active[more], 7] = 1, last[more]
        active = active[more]
    e = np.concatenate(found) if found else np.zeros((0, 4), np.int64)
    e = e[np.lexsort((e[:, 1], e[:, 0]))]
    head = np.ones(len(e), bool)
    head[1:] = (e[1:, 0] != e[:-1, 0]) | (e[1:, 1] != e[:-1, 1])
    at = np.flatnonzero(head)
    sums = np.add.reduceat(e[:, 2:], at, 0) if len(at) else np.zeros((0, 2), np.int64)
    indptr = np.zeros(len(j) + 1, np.int64)
    np.cumsum(np.bincount(e[at, 0], minlength=len(j)), out=indptr[1:])
    return Neighbours(indptr, e[at, 1], sums[:, 0], sums[:, 1])


# ---- device -----------------------------------------------------------------------------------------------------------------------------

def neighbours_rows(labels, jobs, slots, connectivity=4):
    """kg_label_neighbours as it is: labels device int32 [H, W] or [nimg, H, W]; jobs host integers [m, 8] = (img, id, y1, x1, y2, x2,
    resume, after) (uploaded once) or a device int32 tensor -> device int64 [m, 2 + 3 slots].  One launch, no copy back, no
    synchronisation, nothing split."""
    import torch
    from ._lib import ptr, stream_ptr
    connectivity, slots = _connectivity("neighbours", connectivity), _slots("neighbours", slots)
    lab = device_stack("neighbours", labels, COUNTS_FIT)[0]
    nimg, H, W = lab.shape
    jd = _labelmaps.device_jobs("neighbours", jobs, 8, _ROW_JOB_COLUMNS, lab.device)
    m = jd.shape[0]
    out = torch.empty(m, 2 + 3 * slots, dtype=torch.int64, device=lab.device)
    with torch.cuda.device(lab.device):
        _lib.call("kg_label_neighbours", ptr(lab), nimg, H, W, connectivity, ptr(jd) if m else None, m, slots, ptr(out) if m else None,
                  stream_ptr())
    return out


def _device_graph(lab, j, connectivity, slots, max_job_pixels):
    """lab: device int32 [nimg, H, W], j: host jobs [m, 6] -> Neighbours.  One launch, one upload and one copy back per round."""
    return paged(lambda table: neighbours_rows(lab, table, slots, connectivity).cpu().numpy(), j, lab.shape[1], lab.shape[2], slots, max_job_pixels)


def neighbours(labels, n=None, jobs=None, stats=None, connectivity=4, slots=16, max_job_pixels=65536):
    """neighbours_host on the device -> Neighbours (host).  labels: device int32 [H, W] or [nimg, H, W].  What is listed:
      jobs   host integers [m, 6] = (img, id, y1, x1, y2, x2): one row per job; or
      n      the instance count (one per map for a stack): the ids 1 .. n inside their own boxes.  The boxes come from stats -- host
             integers [n, 5] = (area, y1, x1, y2, x2), one array per map for a stack; columns 1:6 of an Instances table are that -- or,
             without stats, from labelmetrics.label_stats (its launches and one copy per map).
    A job whose box holds more than max_job_pixels pixels is listed in bands.  ONE kg_label_neighbours launch, one upload and one
    device -> host copy for all pieces, then one more of each per round for the pieces that have more than `slots` neighbours left
    (paged): with the default 16 slots an instance map needs one round."""
    connectivity, slots = _connectivity("neighbours", connectivity), _slots("neighbours", slots)
    lab = device_stack("neighbours", labels, COUNTS_FIT)[0]
    return _device_graph(lab, _labelmaps.job_table("neighbours", lab, n, jobs, stats, labelmetrics.label_stats), connectivity, slots, max_job_pixels)


# ---- Instances ----------------------------------------------------------------------------------------------------------------------------

def _instance_graphs(insts, connectivity, expand, slots, max_job_pixels):
    """-> one Neighbours per entry (None for a None entry); the entries themselves are not touched"""
    connectivity, slots = _connectivity("neighbours_instances", connectivity), _slots("neighbours_instances", slots)
    grow = 0
    if expand is not None:
        distance.square("neighbours_instances", expand)
        grow = int(math.ceil(expand))
    out = [None] * len(insts)

    def host_one(i, inst, lab):
        if expand is not None:
            lab = distance.expand_labels_host(lab, expand)
        out[i] = neighbours_host(lab, _labelmaps.instance_jobs(inst, 0, grow, *lab.shape), connectivity)
    for idx, stack, H, W in _labelmaps.size_batches("neighbours_instances", insts, host_one):
        if expand is not None:
            stack = distance.expand_labels(stack, expand)
        got = _device_graph(device_stack("neighbours_instances", stack, COUNTS_FIT)[0], _labelmaps.batch_jobs(insts, idx, grow, H, W), connectivity, slots,
                            max_job_pixels)
        for i, a, b in _labelmaps.deal(insts, idx):
            out[i] = got.slice(a, b)
    return out


def neighbours_instances(inst, connectivity=4, expand=None, slots=16, max_job_pixels=65536):
    """neighbours for an Instances / TiledInstances -> Neighbours with len(inst) rows: ids 1 .. n, boxes from table[:, 2:6]; an instance
    with no visible pixel gets an empty row.  expand: None, or a distance in pixels (a number, at most 64): the graph is then taken on
    distance.expand_labels(inst.labels, expand), with the boxes grown by ceil(expand) and clamped -- the "touching after expansion"
    graph, whose `sides` is the length of the shared Voronoi border; inst itself is not changed.  A host label map (assemble_host's
    result) goes through neighbours_host."""
    return _instance_graphs([inst], connectivity, expand, slots, max_job_pixels)[0]


def neighbours_instances_batch(insts, connectivity=4, expand=None, slots=16, max_job_pixels=65536):
    """neighbours_instances for predict_instances' list (entries may be None), in place: every entry's `neighbours` is set.  ONE launch
    per output size and round of paging."""
    for v, g in zip(insts, _instance_graphs(insts, connectivity, expand, slots, max_job_pixels)):
        if v is not None:
            v.neighbours = g
    return insts
