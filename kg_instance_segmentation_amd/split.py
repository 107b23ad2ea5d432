"""Merged instances split on the device: two touching nuclei under one id become two ids again.

Every other label-map module takes the network's instances as given.  The most common defect of a nucleus segmentation is a merged pair
under one id; hulls.py can flag it (solidity) and distance.py can shrink it to cores, and this module turns the cores back into
instances without copying the map to the host:

    seeds            the rank map of the core seeds and S, the seed count of every id   (kg_label_regrow op 2, kg_label_components,
                                                                                          kg_component_stats, kg_component_remap)
    regrow           the seeded geodesic regrow inside every job's instance, ANY seed map  (kg_label_split, csrc/split.hip)
    split            seeds + the host decision + regrow + the refreshed table              (+ kg_label_table)
    split_batch      split for a stack of maps of one size
    split_instances  split for an Instances / TiledInstances; predict_instances, predict_tiled and assemble take split=

The *_host functions state the same semantics in NumPy (the CPU route, and the yardstick of the GPU tests) as per-seed breadth-first
distance maps followed by a lexicographic minimum -- NOT the level-synchronous flood the kernel runs, so the two check each other.  Every
number is an exact integer.

Semantics (include/kgnet_hip.h is the normative text)
  core      shrink_labels(labels, distance, frame) of distance.py, unchanged.
  seeds     the components of core (components.py, connectivity c, bg_connectivity 0).  A seed of id k is a component of value k with
            area >= min_seed_area; the seeds of k get ranks 1 .. S_k in ascending component number (raster order of the first pixel).
  which     an id with S_k <= 1, or not in `only`, is untouched.
  regrow    P = the pixels of the id's box with labels == k.  g(p, s) = the steps of the shortest c-connected path inside P from p to seed
            s.  p goes to the seed of smallest rank among those with the smallest finite g(p, s); a pixel no seed reaches (a piece of k
            without a seed) goes to rank 1.
  ids       rank 1 keeps k; rank r >= 2 becomes first_new_k + r - 2; new ids are n + 1, n + 2, ... per image in ascending (k, r).
  results   parent int32 [n_new]: a row's own index for an original, k - 1 for a new id; the refreshed table (kg_label_table over the
            parents' boxes), a new row's area_full is its parent's.
  size      a job is regrown on the device when fits(h, w) of its clamped box: (h + 2) * (w + 2) <= 16384, the 32 KiB of LDS of one
            workgroup at 16 bits per pixel with a one-pixel halo.  A flood cannot be banded: a larger box is copied back, regrown by the
            host statement and written in (contours.py does the same for its large boxes).

Splitting only the suspicious instances: a merged pair is concave, so with hulls.py
    only = np.flatnonzero(inst.hulls.solidity() < t) + 1
    inst = split_instances(inst, distance, only=only)"""
import numpy as np

from . import _lib, _labelmaps, components, distance as _distance, labelmetrics, tiling

KGLibraryError = _lib.KGLibraryError
MAX_CELLS = 16384                       # KG_SP_CELLS of csrc/split.hip
MAX_RANK = 16382                        # KG_SP_MAX_RANK: a seeds value above it is no seed
ROW_COLUMNS = ("members", "unreached", "levels", "status")
_JOB_COLUMNS = "(img, id, y1, x1, y2, x2, nseeds, first_new)"


def fits(h, w):
    """True when a clamped box of h x w pixels is regrown on the device: (h + 2) * (w + 2) <= 16384."""
    return (int(h) + 2) * (int(w) + 2) <= MAX_CELLS


def _args(fn, connectivity, min_seed_area):
    if connectivity not in (4, 8):
        raise KGLibraryError(f"{fn}: connectivity {connectivity!r} (4 or 8)")
    if isinstance(min_seed_area, (bool, np.bool_)) or not isinstance(min_seed_area, (int, np.integer)) or min_seed_area < 1:
        raise KGLibraryError(f"{fn}: min_seed_area {min_seed_area!r} must be an integer >= 1")
    return int(connectivity), int(min_seed_area)


def _wrap32(v):
    return ((np.asarray(v, np.int64) + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)


# ---- host statements of the semantics ---------------------------------------------------------------------------------------------------

def _bfs(P, seed_masks, conn):
    """P bool [h, w], seed_masks bool [S, h, w] (inside P) -> int32 [S, h, w]: g(p, s), INT32_MAX where no path inside P exists.  One
    breadth-first search per seed, all of them stepped together."""
    S, h, w = seed_masks.shape
    dist = np.full((S, h, w), np.iinfo(np.int32).max, np.int32)
    reach = seed_masks.copy()
    dist[reach] = 0
    front, level = reach, 0
    pad = np.zeros((S, h + 2, w + 2), bool)
    while front.any():
        level += 1
        pad[:, 1:-1, 1:-1] = front
        nb = pad[:, :-2, 1:-1] | pad[:, 2:, 1:-1] | pad[:, 1:-1, :-2] | pad[:, 1:-1, 2:]
        if conn == 8:
            nb |= pad[:, :-2, :-2] | pad[:, :-2, 2:] | pad[:, 2:, :-2] | pad[:, 2:, 2:]
        front = nb & P & ~reach
        dist[front] = level
        reach |= front
    return dist


def regrow_box_host(P, rank, connectivity=4):
    """The regrow rule on one box: P bool [h, w]; rank int [h, w], > 0 on the seed pixels (used inside P only) -> (assign int64 [h, w]: the
    rank every pixel of P goes to, 0 for a pixel no seed reaches and outside P; levels: the largest finite distance).  Per seed a
    breadth-first distance map, then per pixel the lexicographic minimum of (g, rank)."""
    P = np.asarray(P, bool)
    rank = np.where(P, np.asarray(rank, np.int64), 0)
    big = np.iinfo(np.int32).max
    best_d = np.full(P.shape, big, np.int64)
    best_r = np.zeros(P.shape, np.int64)
    u = np.unique(rank[rank > 0])
    chunk = max(1, 4_000_000 // max(P.size, 1))
    for a in range(0, len(u), chunk):
        ranks = u[a:a + chunk]                                           # ascending: argmin's first minimum is the smallest rank
        dist = _bfs(P, rank[None] == ranks[:, None, None], connectivity)
        d, k = dist.min(0), dist.argmin(0)
        take = d < best_d
        best_d[take], best_r[take] = d[take], ranks[k][take]
    got = best_d < big
    return np.where(got, best_r, 0), int(best_d[got].max()) if got.any() else 0


def _split_jobs_table(fn, jobs):
    return _labelmaps.host_jobs(fn, jobs, 8, _JOB_COLUMNS).astype(np.int64).reshape(-1, 8)


def regrow_host(labels, seeds, jobs, connectivity=4):
    """kg_label_split in NumPy: labels, seeds integers [H, W] or [nimg, H, W] (ANY values), jobs integers [m, 8] = (img, id, y1, x1, y2,
    x2, nseeds, first_new) -> (out int32 of the labels' shape, rows int64 [m, 4] = ROW_COLUMNS).  Never size-limited: status is 0."""
    conn, _ = _args("regrow_host", connectivity, 1)
    maps, single = _labelmaps.host_maps("regrow_host", labels, True)
    sd, _ = _labelmaps.host_maps("regrow_host", seeds, True)
    if sd.shape != maps.shape:
        raise KGLibraryError(f"regrow_host: seeds of {sd.shape} for label maps of {maps.shape}")
    nimg, H, W = maps.shape
    j = _split_jobs_table("regrow_host", jobs)
    out = maps.astype(np.int32)
    rows = np.zeros((len(j), 4), np.int64)
    for k, (i, v, y1, x1, y2, x2, ns, first) in enumerate(j.tolist()):
        y1, x1, y2, x2 = max(y1, 0), max(x1, 0), min(y2, H), min(x2, W)
        if not 0 <= i < nimg or y2 <= y1 or x2 <= x1:
            continue
        P = maps[i, y1:y2, x1:x2] == v
        s = sd[i, y1:y2, x1:x2].astype(np.int64)
        rank = np.where(P & (s >= 1) & (s <= min(ns, MAX_RANK)), s, 0)
        assign, levels = regrow_box_host(P, rank, conn)
        rows[k, :3] = P.sum(), (P & (assign == 0)).sum(), levels
        box = out[i, y1:y2, x1:x2]                                       # a view: the assignment writes out
        box[assign >= 2] = _wrap32(first + assign[assign >= 2] - 2)
    return (out[0] if single else out), rows


def rank_components(stats, n, min_seed_area=1):
    """ONE image's component stats int64 [m, 9] of the core -> (rankval int32 [m]: the rank of every component that is a seed, else 0;
    S int64 [n]: the seeds of every id).  Shared by split and split_host: the host decision."""
    s = np.asarray(stats, np.int64).reshape(-1, 9)
    n = int(n)
    value, area = s[:, 0], s[:, 1]
    idx = np.flatnonzero((value >= 1) & (value <= n) & (area >= int(min_seed_area)))
    idx = idx[np.lexsort((idx, value[idx]))]                             # by id, then by component number
    v = value[idx]
    first = np.searchsorted(v, v, side="left")                           # the position of the id's first seed
    rankval = np.zeros(len(s), np.int32)
    rankval[idx] = np.arange(len(idx)) - first + 1
    return rankval, np.bincount(v - 1, minlength=n).astype(np.int64)[:n]


def _only(fn, only, n):
    if only is None:
        return np.ones(n, bool)
    o = np.asarray(only)
    if o.ndim != 1 or (o.size and o.dtype.kind not in "iu"):
        raise KGLibraryError(f"{fn}: only must be None or a list of ids")
    o = o.astype(np.int64)
    if o.size and (o.min() < 1 or o.max() > n):
        raise KGLibraryError(f"{fn}: only names an id outside 1 .. {n}")
    keep = np.zeros(n, bool)
    keep[o - 1] = True
    return keep


def plan_jobs(S, boxes, only, img=0, fn="split"):
    """The ids that split, as kg_label_split's jobs.  S int [n]; boxes int [n, 5] = (area, y1, x1, y2, x2) of the ids (an area of 0: no
    visible pixel, never split); only: None or ids -> (jobs int64 [k, 8], parent int32 [n_new])."""
    S = np.asarray(S, np.int64).reshape(-1)
    n = len(S)
    b = np.asarray(boxes, np.int64).reshape(n, 5)
    ids = np.flatnonzero((S >= 2) & _only(fn, only, n) & (b[:, 0] > 0))
    extra = S[ids] - 1
    first = n + 1 + np.cumsum(extra) - extra
    jobs = np.concatenate([np.full((len(ids), 1), int(img)), ids[:, None] + 1, b[ids, 1:], S[ids, None], first[:, None]], 1).astype(np.int64)
    parent = np.concatenate([np.arange(n), np.repeat(ids, extra)]).astype(np.int32)
    if len(parent) > 2 ** 31 - 1:
        raise KGLibraryError(f"{fn}: {len(parent)} ids exceed 2^31 - 1")
    return jobs.reshape(-1, 8), parent


def _boxes(fn, table, n, stats_of):
    """(area, y1, x1, y2, x2) of the ids 1 .. n: columns 1:6 of the old table, or the map's own stats"""
    if table is None:
        return np.asarray(stats_of(), np.int64).reshape(n, 5)
    t = np.asarray(table)
    if t.shape != (n, 8):
        raise KGLibraryError(f"{fn}: the old table must be [{n}, 8]")
    return t[:, 1:6].astype(np.int64)


def _table_jobs(boxes, parent):
    """kg_label_table's jobs of the new map: every id with a visible parent inside its parent's box -> (jobs int32 [k, 5], rows)"""
    b = np.asarray(boxes, np.int64)[parent]
    rows = np.flatnonzero(b[:, 0] > 0)
    return np.ascontiguousarray(np.concatenate([rows[:, None] + 1, b[rows, 1:]], 1).astype(np.int32)).reshape(-1, 5), rows


def _new_table(table, parent, rows, new_rows):
    out = np.zeros((len(parent), 8), np.int64)
    if table is not None:
        out[:, 0] = np.asarray(table, np.int64).reshape(-1, 8)[parent, 0]
    out[rows, 1:] = np.asarray(new_rows, np.int64).reshape(-1, 8)[:, 1:]
    return out


def seeds_host(labels, n, distance, connectivity=4, min_seed_area=1, frame=False):
    """One label map [H, W] with ids 1 .. n -> (rank map int32 [H, W]: the rank of every seed pixel, 0 elsewhere; S int64 [n])."""
    conn, msa = _args("seeds_host", connectivity, min_seed_area)
    lab = _labelmaps.host_maps("seeds_host", labels, False)
    core = _distance.shrink_labels_host(lab, distance, frame)
    comp, m = components.components_host(core, conn, 0)
    rankval, S = rank_components(components.component_stats_host(core, comp, m), n, msa)
    return np.concatenate([[0], rankval])[comp].astype(np.int32), S


def split_host(labels, n, distance, connectivity=4, min_seed_area=1, frame=False, only=None, table=None):
    """One label map [H, W] with ids 1 .. n -> (new int32 map, table int64 [n_new, 8] (instances.TABLE_COLUMNS), parent int32 [n_new]).
    table: the map's old table: its boxes are the jobs' boxes and its area_full is carried over (a new row gets its parent's); without it
    the boxes come from labelmetrics.label_stats_host and area_full is 0.  A box is never size-limited here."""
    lab = _labelmaps.host_maps("split_host", labels, False)
    n = int(n)
    rank, S = seeds_host(lab, n, distance, connectivity, min_seed_area, frame)
    boxes = _boxes("split_host", table, n, lambda: labelmetrics.label_stats_host(lab, n))
    jobs, parent = plan_jobs(S, boxes, only, 0, "split_host")
    out, _ = regrow_host(lab, rank, jobs, connectivity)
    tj, rows = _table_jobs(boxes, parent)
    return out, _new_table(table, parent, rows, tiling.table_from_labels_host(out, tj)), parent


# ---- device -----------------------------------------------------------------------------------------------------------------------------

def regrow_rows(labels, seeds, jobs, connectivity=4):
    """kg_label_split as it is: labels, seeds device int32 [H, W] or [nimg, H, W]; jobs host integers [m, 8] = (img, id, y1, x1, y2, x2,
    nseeds, first_new) (uploaded once) or a device int32 tensor -> (out device int32 of the labels' shape, rows device int32 [m, 4] =
    ROW_COLUMNS).  A job that does not fit has status 1 and is left as copied.  One copy and one launch, no copy back, no
    synchronisation."""
    import torch
    from ._lib import ptr, stream_ptr
    conn, _ = _args("regrow", connectivity, 1)
    lab, shape = _labelmaps.device_stack("regrow", labels)
    sd = _labelmaps.device_maps("regrow", seeds, True)
    if sd.shape != shape or sd.device != lab.device:
        raise KGLibraryError(f"regrow: seeds of {tuple(sd.shape)} for label maps of {tuple(shape)}: one shape and one device")
    nimg, H, W = lab.shape
    jd = _labelmaps.device_jobs("regrow", jobs, 8, _JOB_COLUMNS, lab.device)
    m = jd.shape[0]
    out = torch.empty_like(lab)
    rows = torch.empty(m, 4, dtype=torch.int32, device=lab.device)
    with torch.cuda.device(lab.device):
        _lib.call("kg_label_split", ptr(lab), ptr(sd), nimg, H, W, conn, ptr(jd) if m else None, m, ptr(out), ptr(rows) if m else None,
                  stream_ptr())
    return out.view(shape), rows


def regrow(labels, seeds, jobs, connectivity=4):
    """regrow_host on the device, for ANY seed map: labels, seeds device int32 [H, W] or [nimg, H, W]; jobs HOST integers [m, 8] ->
    (out device int32 of the labels' shape, rows host int64 [m, 4] = ROW_COLUMNS).  One copy, one launch, one upload (the jobs) and one
    device -> host copy (the rows).  A job whose clamped box does not fit (status 1 in its row) is regrown by the host statement from its
    box copied back and written in; its row then holds the host's counts and keeps status 1."""
    from . import ops
    j = _split_jobs_table("regrow", jobs)
    out, rows = regrow_rows(labels, seeds, j, connectivity)
    rows = rows.cpu().numpy().astype(np.int64) if len(j) else np.zeros((0, 4), np.int64)
    if (rows[:, 3] < 0).any() or (rows[:, 3] > 1).any():
        raise KGLibraryError("regrow: rows that are no rows")
    large = np.flatnonzero(rows[:, 3]).tolist()
    if large:
        lab, _ = _labelmaps.device_stack("regrow", labels)
        sd = seeds.contiguous().view(lab.shape)
        o3 = out.view(lab.shape)
        _, H, W = lab.shape
        for k in large:                                                   # a flood cannot be banded: the box comes back
            i, v, y1, x1, y2, x2, ns, first = j[k].tolist()
            y1, x1, y2, x2 = max(y1, 0), max(x1, 0), min(y2, H), min(x2, W)
            P = lab[i, y1:y2, x1:x2].cpu().numpy() == v
            s = sd[i, y1:y2, x1:x2].cpu().numpy().astype(np.int64)
            assign, levels = regrow_box_host(P, np.where((s >= 1) & (s <= min(ns, MAX_RANK)), s, 0), connectivity)
            rows[k, :3] = P.sum(), (P & (assign == 0)).sum(), levels
            if (assign >= 2).any():
                box = o3[i, y1:y2, x1:x2].cpu().numpy()
                box[assign >= 2] = _wrap32(first + assign[assign >= 2] - 2)
                o3[i, y1:y2, x1:x2].copy_(ops.h2d(np.ascontiguousarray(box), lab.device))
    return out, rows


def _seeds_stack(fn, lab, ns, distance, conn, msa, frame):
    """lab device int32 [nimg, H, W] -> (rank map device int32 [nimg, H, W], per image S)"""
    core = _distance.shrink_labels(lab, distance, frame)
    comp, ncomp = components.components(core, conn, 0)
    stats, cs = components.component_stats(core, comp, ncomp)
    dec = [rank_components(stats[cs[i]:cs[i + 1]], ns[i], msa) for i in range(len(ns))]
    return components.remap(comp, cs, np.concatenate([d[0] for d in dec])), [d[1] for d in dec]


def seeds(labels, n, distance, connectivity=4, min_seed_area=1, frame=False):
    """seeds_host on the device: labels device int32 [H, W] with ids 1 .. n (or a stack [nimg, H, W] with one count per image) -> (the
    rank map, device int32 of the labels' shape; S host int64 [n], one array per image for a stack).  shrink_labels' launch, components 6,
    stats 3 (two copies back), remap 1."""
    conn, msa = _args("seeds", connectivity, min_seed_area)
    lab, shape = _labelmaps.device_stack("seeds", labels)
    rank, S = _seeds_stack("seeds", lab, _labelmaps.counts("seeds", n, lab.shape[0]), distance, conn, msa, frame)
    return rank.view(shape), (S[0] if len(shape) == 2 else S)


def split_batch(labels, ns, distance, connectivity=4, min_seed_area=1, frame=False, only=None, tables=None):
    """split for a stack of maps of one size: labels device int32 [nimg, H, W], ns = the instance count of every image; only = None, or
    per image None or the ids that may be split; tables = None, or per image the old table (or None) -> (new maps device int32
    [nimg, H, W], per image the table, per image parent).  ONE seeds pass, ONE kg_label_split launch for all images, one kg_label_table
    launch per image and one copy back of all tables; an image without a table costs labelmetrics.label_stats on top."""
    import torch
    conn, msa = _args("split", connectivity, min_seed_area)
    lab = _labelmaps.device_maps("split", labels, True)
    if lab.dim() != 3:
        raise KGLibraryError("split: a stack [nimg, H, W] and one instance count per image")
    lab, _ = _labelmaps.device_stack("split", lab)
    nimg = lab.shape[0]
    ns = _labelmaps.counts("split", ns, nimg)
    for what, v in (("only", only), ("tables", tables)):
        if v is not None and len(v) != nimg:
            raise KGLibraryError(f"split: {what} must be None or one entry per image")
    rank, S = _seeds_stack("split", lab, ns, distance, conn, msa, frame)
    boxes = [_boxes("split", None if tables is None else tables[i], ns[i], lambda i=i: labelmetrics.label_stats(lab[i], ns[i])) for i in range(nimg)]
    plans = [plan_jobs(S[i], boxes[i], None if only is None else only[i], i) for i in range(nimg)]
    out, _ = regrow(lab, rank, np.concatenate([p[0] for p in plans]), conn)
    tj = [_table_jobs(boxes[i], plans[i][1]) for i in range(nimg)]
    got = [tiling.table_from_labels(out[i], tj[i][0]) for i in range(nimg)]
    host = (torch.cat(got) if nimg > 1 else got[0]).cpu().numpy()
    tabs, r = [], 0
    for i in range(nimg):
        rows = tj[i][1]
        tabs.append(_new_table(None if tables is None else tables[i], plans[i][1], rows, host[r:r + len(rows)]))
        r += len(rows)
    return out, tabs, [p[1] for p in plans]


def split(labels, n, distance, connectivity=4, min_seed_area=1, frame=False, only=None, table=None):
    """split_host on the device: labels = device int32 [H, W] with ids 1 .. n -> (new device int32 map, host int64 table [n_new, 8],
    parent int32 [n_new]).  A fixed number of launches whatever the map holds: shrink_labels 1, components 6, stats 3 (two copies back),
    the host decision over a few thousand integers, remap 1 (the rank map), kg_label_split 1 and its copy (one upload of the jobs, one
    copy back of the rows), kg_label_table 1 and one copy of the table.  table: the map's old table (boxes and area_full); without it the
    boxes cost labelmetrics.label_stats.  Only a job whose box does not fit (fits) costs more: its box is regrown on the host."""
    lab = _labelmaps.device_maps("split", labels, True)
    if lab.dim() != 2:
        raise KGLibraryError("split: one label map [H, W] (split_batch takes a stack)")
    out, tabs, parents = split_batch(lab[None], [n], distance, connectivity, min_seed_area, frame, None if only is None else [only],
                                     None if table is None else [table])
    return out[0], tabs[0], parents[0]


# ---- Instances ----------------------------------------------------------------------------------------------------------------------------

def _grown(inst, labels, table, parent):
    """A new object of inst's type: labels and table replaced, dets (tile, origin) extended by a copy of the parent's row per new id,
    masks / tile_masks kept (the rows of the parents), parent set when a split ran."""
    from .instances import Instances
    from .tiling import TiledInstances
    n = len(inst)
    if len(parent) == n:                                                  # nothing split: parent stays as it was
        return components.like(inst, labels, table)
    old = np.arange(n, dtype=np.int32) if inst.parent is None else np.asarray(inst.parent, np.int32)
    dets = np.asarray(inst.dets)[parent]
    if isinstance(inst, TiledInstances):
        new = TiledInstances(labels, dets, table, np.asarray(inst.tile)[parent], np.asarray(inst.origin)[parent], inst.tile_masks)
    else:
        new = Instances(labels, dets, table, inst.masks)
    new.parent = old[parent]                                              # through an earlier split: always a row of masks
    return new


def split_instances(inst, distance, connectivity=4, min_seed_area=1, frame=False, only=None):
    """split for an Instances / TiledInstances: a new object of the same type.  labels and table are replaced; dets is extended by a copy
    of the parent's row per new id (likewise tile and origin of a TiledInstances), so len() and the table stay consistent and the ids
    still mean rows of dets; masks / tile_masks are kept as they are, the rows of the parents; `parent` (int32 [len]) is set when a split
    ran and stays None otherwise: masks[parent[i]] is the mask instance i + 1 came from.  Everything later (expand, measure, quantiles,
    neighbours, runs, contours, hulls) works from labels and table alone.  A host label map (assemble_host's result) goes through
    split_host.  only: None, or the ids that may be split, for example np.flatnonzero(inst.hulls.solidity() < t) + 1."""
    return split_instances_batch([inst], distance, connectivity, min_seed_area, frame, None if only is None else [only])[0]


def split_instances_batch(insts, distance, connectivity=4, min_seed_area=1, frame=False, only=None):
    """split_instances for predict_instances' list (entries may be None): the seeds and kg_label_split run ONCE over all images of one
    output size.  only: None, or per entry None or the ids that may be split."""
    _args("split_instances", connectivity, min_seed_area)
    _distance.square("split_instances", distance)
    if only is not None and len(only) != len(insts):
        raise KGLibraryError("split_instances: only must be None or one entry per instance list entry")
    only = [None] * len(insts) if only is None else list(only)
    out = list(insts)

    def host_one(i, inst, lab):
        new, table, parent = split_host(lab, len(inst), distance, connectivity, min_seed_area, frame, only[i], inst.table)
        out[i] = _grown(inst, new, table, parent)
    for idx, stack, _, _ in _labelmaps.size_batches("split_instances", insts, host_one):
        new, tabs, parents = split_batch(stack, [len(insts[i]) for i in idx], distance, connectivity, min_seed_area, frame,
                                         [only[i] for i in idx], [insts[i].table for i in idx])
        for k, i in enumerate(idx):
            out[i] = _grown(insts[i], new[k], tabs[k], parents[k])
    return out
