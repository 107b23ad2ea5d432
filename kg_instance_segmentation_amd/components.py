"""Label-map clean-up: connected components of an instance label map, and the usual policy on top of them -- keep the largest piece of
every instance, drop specks, fill holes -- without copying the map back.

predict_instances and predict_tiled end in ONE int32 label map per image, and nothing so far looked at its connectivity: an overlap that
goes to the more confident instance leaves the other one in two or three pieces under one id, the mask threshold leaves pin-holes and
specks at a box edge, and a tile edge can cut a sliver off a large object.

    components       comp (the component number of every pixel) and ncomp per image      (kg_label_components, csrc/components.hip)
    component_stats  per component {value, area, box, border, nb_min, nb_max}              (kg_component_stats), copied to the host
    clean            the policy, decided on the host over the stats (a few thousand integers), written back by kg_component_remap;
                     the refreshed per-instance table comes from kg_label_table
    clean_instances  clean for an Instances / TiledInstances; predict_instances, predict_tiled and assemble take clean={...}

The *_host functions state the same semantics in NumPy and plain Python (the CPU route, and the yardstick of the GPU tests); every
number is an exact integer.

Semantics (include/kgnet_hip.h is the normative text)
  joining     two pixels of one image belong together if they hold the same value and are adjacent under the rule for that value:
              `connectivity` (4 or 8) for non-zero values, `bg_connectivity` (0, 4 or 8) for the value 0.  With bg_connectivity == 0 zero
              pixels belong to no component.  Values are compared only: any int32 is a value.
  comp        0 for a pixel outside every component, else the number of its component: 1 .. m per image, in raster order of each
              component's first pixel (smallest y * W + x).  Ids and background components share one numbering.
  stats       int64 [m, 9] (STATS_COLUMNS), row c - 1: the label value of the component, its pixel count, its half-open box, border = 1
              if a pixel lies on the first or last row or column, and nb_min / nb_max = the smallest / largest comp value over all
              4-adjacent pixels whose comp differs from c (pixels with comp == 0 count as 0; both -1 if there is none).
  policy      see clean_host."""
import numpy as np

from . import _lib
from ._labelmaps import device_maps, host_maps, size_batches
from .instances import Instances, TABLE_COLUMNS  # noqa: F401  (TABLE_COLUMNS: the columns of the tables returned here)

KGLibraryError = _lib.KGLibraryError
STATS_COLUMNS = ("value", "area", "y1", "x1", "y2", "x2", "border", "nb_min", "nb_max")
POLICY = {"keep": "largest", "min_area": 0, "fill_holes": True, "max_hole_area": None, "connectivity": 8, "relabel": False}


def _conn(fn, connectivity, bg_connectivity):
    if connectivity not in (4, 8) or bg_connectivity not in (0, 4, 8):
        raise KGLibraryError(f"{fn}: connectivity {connectivity} (4 or 8), bg_connectivity {bg_connectivity} (0, 4 or 8)")
    return int(connectivity), int(bg_connectivity)


def _host_maps(fn, labels):
    """-> (int64 [nimg, H, W], was_2d)"""
    maps, single = host_maps(fn, labels, True)
    return maps.astype(np.int64), single


# ---- host statements of the semantics ---------------------------------------------------------------------------------------------------

def _components_one(lab, conn, bg):
    """One image.  Rows are cut into runs (a pixel whose value has connectivity 0 is a run of its own), runs of consecutive rows are
    united where they touch, and a component is numbered by its first run: runs are numbered in raster order of their first pixel."""
    H, W = lab.shape
    c = np.where(lab != 0, conn, bg)
    start = np.ones((H, W), bool)
    start[:, 1:] = (lab[:, 1:] != lab[:, :-1]) | (c[:, 1:] == 0)
    run = (np.cumsum(start.reshape(-1)) - 1).reshape(H, W)
    nrun = int(run[-1, -1]) + 1
    live = np.zeros(nrun, bool)
    live[run.reshape(-1)] = c.reshape(-1) != 0
    edges = []
    if H > 1:
        def touch(a, b, sel):                          # a: pixels of rows 1 .., b: the pixels of the row above them, shifted
            edges.append(np.stack([run[1:][a][sel], run[:-1][b][sel]], 1))
        full = (slice(None), slice(None))
        touch(full, full, (lab[1:] == lab[:-1]) & (c[1:] != 0))
        if W > 1:
            a, b = (slice(None), slice(1, None)), (slice(None), slice(None, -1))           # (y, x) with (y - 1, x - 1)
            touch(a, b, (lab[1:][a] == lab[:-1][b]) & (c[1:][a] == 8))
            touch(b, a, (lab[1:][b] == lab[:-1][a]) & (c[1:][b] == 8))                      # (y, x) with (y - 1, x + 1)
    parent = list(range(nrun))
    if edges:
        e = np.concatenate(edges)
        e = np.unique(e[:, 0].astype(np.int64) * nrun + e[:, 1]) if len(e) else e
        for key in e.tolist() if len(e) else ():
            a, b = divmod(key, nrun)
            while parent[a] != a:
                parent[a] = a = parent[parent[a]]
            while parent[b] != b:
                parent[b] = b = parent[parent[b]]
            if a < b:
                parent[b] = a
            elif b < a:
                parent[a] = b
    for i in range(nrun):                              # a parent is never above its run: one ascending pass flattens everything
        parent[i] = parent[parent[i]]
    root = np.asarray(parent, np.int64)
    first = live & (root == np.arange(nrun))
    number = np.where(live, np.cumsum(first)[root], 0)
    return number[run].astype(np.int32), int(first.sum())


def components_host(labels, connectivity=8, bg_connectivity=0):
    """Integer label map(s) [H, W] or [nimg, H, W] -> (comp int32 of the same shape, ncomp: an int, or int64 [nimg] for a stack)."""
    conn, bg = _conn("components_host", connectivity, bg_connectivity)
    maps, single = _host_maps("components_host", labels)
    out = [_components_one(m, conn, bg) for m in maps]
    comp, ncomp = np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int64)
    return (comp[0], int(ncomp[0])) if single else (comp, ncomp)


def _stats_one(lab, comp, m):
    H, W = lab.shape
    out = np.zeros((m, 9), np.int64)
    out[:, 7:] = -1
    ys, xs = np.nonzero((comp >= 1) & (comp <= m))
    if m == 0 or len(ys) == 0:
        return out
    k = comp[ys, xs] - 1
    big = np.iinfo(np.int64).max
    val, y1, x1 = np.full(m, -big), np.full(m, big), np.full(m, big)
    np.maximum.at(val, k, lab[ys, xs])
    out[:, 1] = np.bincount(k, minlength=m)
    np.minimum.at(y1, k, ys); np.minimum.at(x1, k, xs)
    np.maximum.at(out[:, 4], k, ys + 1); np.maximum.at(out[:, 5], k, xs + 1)
    np.maximum.at(out[:, 6], k, ((ys == 0) | (ys == H - 1) | (xs == 0) | (xs == W - 1)).astype(np.int64))
    have = out[:, 1] > 0
    out[have, 0], out[have, 2], out[have, 3] = val[have], y1[have], x1[have]
    lo, hi = np.full(m, big), np.full(m, -big)
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        ny, nx = ys + dy, xs + dx
        ok = (ny >= 0) & (ny < H) & (nx >= 0) & (nx < W)
        nb = comp[ny[ok], nx[ok]]
        differs = nb != k[ok] + 1
        np.minimum.at(lo, k[ok][differs], nb[differs]); np.maximum.at(hi, k[ok][differs], nb[differs])
    met = lo != big
    out[met, 7], out[met, 8] = lo[met], hi[met]
    return out


def component_stats_host(labels, comp, ncomp):
    """labels, comp [H, W] (or stacks [nimg, H, W] with ncomp [nimg]) -> int64 [m, 9] (STATS_COLUMNS); for a stack the rows of the images
    follow each other.  A comp value outside [1, m] names no row."""
    maps, _ = _host_maps("component_stats_host", labels)
    comps, _ = _host_maps("component_stats_host", comp)
    ms = np.asarray(ncomp, np.int64).reshape(-1)
    if maps.shape != comps.shape or len(ms) != len(maps) or np.any(ms < 0):
        raise KGLibraryError(f"component_stats_host: labels {maps.shape}, comp {comps.shape}, {len(ms)} counts")
    return np.concatenate([_stats_one(a, b, int(m)) for a, b, m in zip(maps, comps, ms)])


def _policy(fn, policy):
    bad = set(policy) - set(POLICY)
    if bad:
        raise KGLibraryError(f"{fn}: unknown policy argument(s) {sorted(bad)}; known: {sorted(POLICY)}")
    p = dict(POLICY, **policy)
    if p["keep"] not in ("largest", "all"):
        raise KGLibraryError(f"{fn}: keep must be 'largest' or 'all', not {p['keep']!r}")
    if p["connectivity"] not in (4, 8):
        raise KGLibraryError(f"{fn}: connectivity {p['connectivity']} is not 4 or 8")
    if int(p["min_area"]) != p["min_area"] or p["min_area"] < 0 or (p["max_hole_area"] is not None and p["max_hole_area"] < 0):
        raise KGLibraryError(f"{fn}: min_area {p['min_area']}, max_hole_area {p['max_hole_area']}")
    p["bg_connectivity"] = (4 if p["connectivity"] == 8 else 8) if p["fill_holes"] else 0
    return p


def decide(stats, n, policy, fn="clean"):
    """The policy over ONE image's component stats int64 [m, 9] -> (newval int32 [m], the new label value of every component; jobs int32
    [k, 5] = (id, y1, x1, y2, x2), the box of every id that survives; old_ids int32 [k], the ids that survive, ascending).  With relabel
    newval and the jobs carry the compacted ids 1 .. k, otherwise the old ones.  Shared by clean and clean_host."""
    s = np.asarray(stats, np.int64).reshape(-1, 9)
    m, n = len(s), int(n)
    value, area = s[:, 0], s[:, 1]
    outside = (value < 0) | (value > n)
    if outside.any():
        raise KGLibraryError(f"{fn}: {int(area[outside].sum())} pixel(s) of the label map lie outside [0, {n}]")
    fg = value > 0
    kept = fg.copy()
    if policy["keep"] == "largest":
        cand = np.flatnonzero(fg)
        order = cand[np.lexsort((cand, -area[cand], value[cand]))]     # per id: the largest area first, a tie by the lowest number
        best = order[np.flatnonzero(np.diff(value[order], prepend=0))] if len(order) else order
        kept[:] = False
        kept[best] = True
    kept &= area >= int(policy["min_area"])
    newval = np.where(kept, value, 0)
    hole = np.zeros(m, bool)
    if policy["fill_holes"]:
        hole = (value == 0) & (area > 0) & (s[:, 6] == 0) & (s[:, 7] == s[:, 8]) & (s[:, 7] > 0) & (s[:, 7] <= m)
        if policy["max_hole_area"] is not None:
            hole &= area <= int(policy["max_hole_area"])
        filled = newval[s[hole, 7] - 1]                                  # what the one enclosing component became (an id's component)
        newval = newval.copy()
        newval[hole] = filled
    old_ids = np.unique(newval[newval > 0]).astype(np.int32)
    if policy["relabel"]:
        lut = np.zeros(n + 1, np.int64)
        lut[old_ids] = np.arange(1, len(old_ids) + 1)
        newval = lut[newval]
    ids = np.arange(1, len(old_ids) + 1) if policy["relabel"] else old_ids.astype(np.int64)
    big = np.iinfo(np.int64).max
    box = np.stack([np.full(n + 1, big), np.full(n + 1, big), np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)], 1)
    live = np.flatnonzero(newval > 0)
    np.minimum.at(box[:, 0], newval[live], s[live, 2]); np.minimum.at(box[:, 1], newval[live], s[live, 3])
    np.maximum.at(box[:, 2], newval[live], s[live, 4]); np.maximum.at(box[:, 3], newval[live], s[live, 5])
    jobs = np.concatenate([ids[:, None], box[ids]], 1).astype(np.int32).reshape(-1, 5)
    return newval.astype(np.int32), jobs, old_ids


def _finish_table(rows, jobs, old_ids, n, relabel, table, fn):
    """Rows int64 [k, 8] of the surviving ids (kg_label_table's, area_full still 0) -> the returned table: [k, 8] with relabel, else [n, 8]
    with zero rows for the ids that vanished; area_full from the caller's old table."""
    rows = np.asarray(rows, np.int64).reshape(-1, 8).copy()
    if table is not None:
        old = np.asarray(table)
        if old.shape != (n, 8):
            raise KGLibraryError(f"{fn}: the old table must be [{n}, 8]")
        rows[:, 0] = old[old_ids.astype(np.int64) - 1, 0]
    if relabel:
        return rows
    out = np.zeros((n, 8), np.int64)
    out[jobs[:, 0].astype(np.int64) - 1] = rows
    return out


def clean_host(labels, n, keep="largest", min_area=0, fill_holes=True, max_hole_area=None, connectivity=8, relabel=False, table=None):
    """Label map [H, W] with ids 1 .. n -> (new int32 map, int64 [n, 8] table (TABLE_COLUMNS)[, old_ids]).

      1. Components are taken with `connectivity` for ids; with fill_holes, background components are taken too, with the complementary
         connectivity (4 for 8, 8 for 4).
      2. keep="largest": every id keeps its component of largest area (a tie: the lowest component number), its other components become
         0; keep="all" keeps every piece.
      3. A kept component with area < min_area becomes 0.
      4. A background component is a hole when border == 0, nb_min == nb_max == k > 0 (exactly one component encloses it) and area <=
         max_hole_area when that is given.  A hole takes whatever component k became: k's id if k was kept, 0 otherwise.
      5. A value outside [0, n] raises, naming the pixel count.
      6. relabel=True compacts the surviving ids to 1 .. k in ascending order of old id and also returns old_ids int32 [k]; the table
         then has k rows.
    ALL decisions are taken on the components of the INPUT map, in one pass: the hole a dropped fragment leaves behind is not a component
    of the input and is not filled; a caller who wants it filled calls clean twice.
    table: the map's old table; its area_full column is carried over (0 without it).  An id that vanished has a zero row."""
    p = _policy("clean_host", dict(keep=keep, min_area=min_area, fill_holes=fill_holes, max_hole_area=max_hole_area, connectivity=connectivity,
                                   relabel=relabel))
    lab, single = _host_maps("clean_host", labels)
    if not single:
        raise KGLibraryError("clean_host: one label map [H, W]")
    comp, m = components_host(lab[0], p["connectivity"], p["bg_connectivity"])
    newval, jobs, old_ids = decide(component_stats_host(lab[0], comp, m), n, p, "clean_host")
    out = np.concatenate([[0], newval])[comp].astype(np.int32)
    from .tiling import table_from_labels_host
    tab = _finish_table(table_from_labels_host(out, jobs), jobs, old_ids, int(n), p["relabel"], table, "clean_host")
    return (out, tab, old_ids) if p["relabel"] else (out, tab)


# ---- device -----------------------------------------------------------------------------------------------------------------------------

def components(labels, connectivity=8, bg_connectivity=0):
    """labels: device int32 [H, W] or [nimg, H, W], any values -> (comp device int32 of the same shape, ncomp device int32 [nimg]).
    Six launches, no copy, no synchronisation (kg_label_components)."""
    import torch
    from ._lib import ptr, stream_ptr, c_long
    conn, bg = _conn("components", connectivity, bg_connectivity)
    lab = device_maps("components", labels, True)
    H, W = lab.shape[-2:]
    nimg = lab.numel() // (H * W)
    need = _lib.load().kg_label_components_workspace_bytes(nimg, H, W)
    if need < 0:
        raise KGLibraryError(f"components: no workspace size for {nimg} x {H} x {W}")
    comp = torch.empty_like(lab)
    ncomp = torch.empty(nimg, dtype=torch.int32, device=lab.device)
    work = torch.empty(need // 4, dtype=torch.int32, device=lab.device)
    with torch.cuda.device(lab.device):
        _lib.call("kg_label_components", ptr(lab), nimg, H, W, conn, bg, ptr(comp), ptr(ncomp), ptr(work), c_long(need), stream_ptr())
    return comp, ncomp


def component_stats(labels, comp, ncomp):
    """labels, comp: device int32 of one shape; ncomp: device int32 [nimg] (components' outputs) -> (host int64 [total, 9]
    (STATS_COLUMNS), comp_start host int32 [nimg + 1]).  Two device -> host copies: ncomp, then the stats."""
    import torch
    from ._lib import ptr, stream_ptr
    lab = device_maps("component_stats", labels, True)
    cmp_ = device_maps("component_stats", comp, True, lab)
    H, W = lab.shape[-2:]
    nimg = lab.numel() // (H * W)
    if not torch.is_tensor(ncomp) or ncomp.dtype != torch.int32 or tuple(ncomp.shape) != (nimg,):
        raise KGLibraryError(f"component_stats: ncomp must be an int32 tensor [{nimg}]")
    counts = ncomp.cpu().numpy().astype(np.int64)
    if np.any(counts < 0) or counts.sum() * 9 > 2 ** 31 - 1:
        raise KGLibraryError("component_stats: bad component counts")
    comp_start = np.ascontiguousarray(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))
    total = int(comp_start[-1])
    stats = torch.empty(total, 9, dtype=torch.int32, device=lab.device)
    with torch.cuda.device(lab.device):
        _lib.call("kg_component_stats", ptr(lab), ptr(cmp_), nimg, H, W, comp_start.ctypes.data, total, ptr(stats) if total else None, stream_ptr())
    return stats.cpu().numpy().astype(np.int64), comp_start


def remap(comp, comp_start, newval):
    """comp: device int32 [H, W] or [nimg, H, W]; comp_start: host ints [nimg + 1]; newval: host ints [total] (uploaded once) or a device
    int32 tensor -> device int32 of comp's shape (kg_component_remap)."""
    import torch
    from . import ops
    from ._lib import ptr, stream_ptr
    cmp_ = device_maps("remap", comp, True)
    H, W = cmp_.shape[-2:]
    nimg = cmp_.numel() // (H * W)
    cs = np.ascontiguousarray(np.asarray(comp_start, np.int64).reshape(-1).astype(np.int32))
    if len(cs) != nimg + 1:
        raise KGLibraryError(f"remap: comp_start has {len(cs)} entries for {nimg} image(s)")
    total = int(cs[-1])
    if torch.is_tensor(newval):
        if newval.dtype != torch.int32 or newval.device != cmp_.device or tuple(newval.shape) != (total,):
            raise KGLibraryError(f"remap: device newval must be int32 [{total}] on comp's device")
        nv = newval.contiguous()
    else:
        v = np.asarray(newval).reshape(-1)
        if len(v) != total or v.dtype.kind not in "iu":
            raise KGLibraryError(f"remap: newval must be {total} integers")
        nv = ops.h2d(np.ascontiguousarray(v.astype(np.int32)), cmp_.device) if total else None
    out = torch.empty_like(cmp_)
    with torch.cuda.device(cmp_.device):
        _lib.call("kg_component_remap", ptr(cmp_), nimg, H, W, cs.ctypes.data, total, ptr(nv) if total else None, ptr(out), stream_ptr())
    return out


def clean_batch(labels, ns, tables=None, **policy):
    """clean for a stack of maps of one size: labels device int32 [nimg, H, W], ns = the instance count of every image, tables = None or
    per image the old table (or None).  ONE components / stats / remap pass over the whole stack; returns (new maps device int32
    [nimg, H, W], per image the table, per image old_ids)."""
    import torch
    from . import tiling
    p = _policy("clean", policy)
    lab = device_maps("clean", labels, True)
    if lab.dim() != 3 or len(ns) != lab.shape[0]:
        raise KGLibraryError("clean: a stack [nimg, H, W] and one instance count per image")
    nimg = lab.shape[0]
    comp, ncomp = components(lab, p["connectivity"], p["bg_connectivity"])
    stats, cs = component_stats(lab, comp, ncomp)
    dec = [decide(stats[cs[i]:cs[i + 1]], ns[i], p) for i in range(nimg)]
    out = remap(comp, cs, np.concatenate([d[0] for d in dec]))
    rows = [tiling.table_from_labels(out[i], dec[i][1]) for i in range(nimg)]
    host = (torch.cat(rows) if nimg > 1 else rows[0]).cpu().numpy()
    tabs, r = [], 0
    for i, (_, jobs, old_ids) in enumerate(dec):
        tabs.append(_finish_table(host[r:r + len(jobs)], jobs, old_ids, int(ns[i]), p["relabel"], None if tables is None else tables[i], "clean"))
        r += len(jobs)
    return out, tabs, [d[2] for d in dec]


def clean(labels, n, keep="largest", min_area=0, fill_holes=True, max_hole_area=None, connectivity=8, relabel=False, table=None):
    """clean_host on the device: labels = device int32 [H, W] with ids 1 .. n -> (new device int32 map, host int64 table[, old_ids]).
    A fixed number of launches (components 6, stats 3, remap 1, kg_label_table 1); the decision is made on the host over the stats, which
    cost two device -> host copies (ncomp, then the stats); the refreshed table, which holds coordinate sums the stats do not, is one
    more.  ALL decisions are taken on the components of the INPUT map, in one pass (clean_host): call clean twice to fill the hole a
    dropped fragment leaves behind."""
    lab = device_maps("clean", labels, True)
    if lab.dim() != 2:
        raise KGLibraryError("clean: one label map [H, W] (clean_batch takes a stack)")
    out, tabs, old = clean_batch(lab[None], [n], None if table is None else [table], keep=keep, min_area=min_area, fill_holes=fill_holes,
                                 max_hole_area=max_hole_area, connectivity=connectivity, relabel=relabel)
    return (out[0], tabs[0], old[0]) if relabel else (out[0], tabs[0])


def like(inst, labels, table):
    """A new object of inst's type with labels and table replaced; dets, the masks and parent (split.py) are kept."""
    from .tiling import TiledInstances
    if isinstance(inst, TiledInstances):
        new = TiledInstances(labels, inst.dets, table, inst.tile, inst.origin, inst.tile_masks)
    else:
        new = Instances(labels, inst.dets, table, inst.masks)
    new.parent = inst.parent
    return new


def _instance_policy(fn, policy):
    if policy.get("relabel", False):
        raise KGLibraryError(f"{fn}: relabel is not available for an Instances: its ids mean rows of dets (relabel the map with clean)")
    return policy


def clean_instances(inst, **policy):
    """clean for an Instances / TiledInstances: a new object of the same type with labels and table replaced; dets, masks and tile /
    origin / tile_masks are kept, so the ids still mean rows of dets (relabel is therefore refused) and an instance that vanished has a
    zero table row.  area_full is carried over.  A host label map (assemble_host's result) goes through clean_host."""
    import torch
    if not isinstance(inst, Instances):
        raise KGLibraryError("clean_instances: an Instances or a TiledInstances")
    _instance_policy("clean_instances", policy)
    if torch.is_tensor(inst.labels) and inst.labels.device.type == "cuda":
        labels, table = clean(inst.labels, len(inst), table=inst.table, **policy)
    else:
        lab = inst.labels.numpy() if torch.is_tensor(inst.labels) else inst.labels
        labels, table = clean_host(lab, len(inst), table=inst.table, **policy)
    return like(inst, labels, table)


def clean_instances_batch(insts, **policy):
    """clean_instances for predict_instances' list (entries may be None): components run ONCE over all images of one output size."""
    _instance_policy("clean", policy)
    out = list(insts)
    for idx, stack, _, _ in size_batches("clean", insts):
        labels, tabs, _ = clean_batch(stack, [len(insts[i]) for i in idx], [insts[i].table for i in idx], **policy)
        for k, i in enumerate(idx):
            out[i] = like(insts[i], labels[k], tabs[k])
    return out
