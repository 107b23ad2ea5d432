"""Nearest-other-label distance maps: how far every pixel of a label map is from a pixel that carries another value, and which value --
and the four products of that one transform: expanded labels (cell regions from nuclei), rings (a cytoplasm proxy), shrunk labels (seeds,
margins) and the inscribed circle of every instance (its thickness, and a centre that lies inside a non-convex object).

    distance         (d2, nearest) per pixel                                               (kg_label_distance, csrc/distance.hip)
    expand_labels    every id grown by `distance` pixels, two ids never merge             (kg_label_regrow, op 0)
    ring_labels      the part of the expansion between `inner` and `outer`                 (op 1)
    shrink_labels    the pixels farther than `distance` from everything else               (op 2)
    inscribed        per instance the largest inner d2, where it is attained, the count    (kg_label_distance + kg_label_inscribed)
    expand_instances expand_labels for an Instances / TiledInstances, the table refreshed; predict_instances and predict_tiled take expand=

The *_host functions state the same semantics in NumPy (the CPU route, and the yardstick of the GPU tests), as a plain minimum over the
offsets (dy, dx) with dy^2 + dx^2 <= max_d2 -- NOT the separable form the kernel uses.  Every number is an exact integer.

Semantics (include/kgnet_hip.h is the normative text)
  labels     integers [H, W] or [nimg, H, W]; the values may be ANY int32 and are only compared.
  max_d2     an integer in 1 .. 4096: the search radius is floor(sqrt(max_d2)) <= 64 pixels.
  C(p)       for a pixel p with value v: the pixels q of the same image with labels[q] != v and |p - q|^2 <= max_d2.
  d2[p]      the smallest |p - q|^2 over C(p); max_d2 + 1 ("saturated") when C(p) is empty.
  nearest[p] the smallest value (signed compare) among the q of C(p) at that distance; v when C(p) is empty.
  frame      with frame the four sides of the image count as another value for d2 only: f = min(y + 1, x + 1, H - y, W - x), and where
             f^2 <= max_d2, d2[p] = min(d2[p], f^2).  nearest is not affected.
  distances  a float or an int; a pixel lies within `distance` when d2 <= floor(distance^2).  At most 64.
  images     a stacked image never sees its neighbours in the stack."""
import math

import numpy as np

from . import _lib, _labelmaps, components, labelmetrics, tiling

KGLibraryError = _lib.KGLibraryError
TILE_H, TILE_W = 32, 64                 # the tile of one workgroup (KG_DT_TH, KG_DT_TW of csrc/distance.hip): the tests need the seams
MAX_D2 = 4096
EXPAND, RING, SHRINK = 0, 1, 2
INSCRIBED_DTYPE = np.dtype([("d2max", np.int64), ("radius", np.float64), ("y", np.int64), ("x", np.int64), ("count", np.int64),
                            ("saturated", np.bool_)])


def _max_d2(fn, max_d2):
    if isinstance(max_d2, (bool, np.bool_)) or not isinstance(max_d2, (int, np.integer)) or not 1 <= int(max_d2) <= MAX_D2:
        raise KGLibraryError(f"{fn}: max_d2 {max_d2!r} must be an integer in 1 .. {MAX_D2}")
    return int(max_d2)


def square(fn, distance, least=1):
    """floor(distance^2) of a float or an int distance; refused above 64 and where the square is below `least`"""
    if isinstance(distance, (bool, np.bool_)) or not isinstance(distance, (int, float, np.integer, np.floating)) or not math.isfinite(distance) \
            or distance < 0:
        raise KGLibraryError(f"{fn}: distance {distance!r} must be a non-negative number")
    sq = int(distance) ** 2 if isinstance(distance, (int, np.integer)) else int(math.floor(float(distance) ** 2))
    if sq > MAX_D2:
        raise KGLibraryError(f"{fn}: distance {distance} exceeds 64 (the search radius of max_d2 <= {MAX_D2})")
    if sq < least:
        raise KGLibraryError(f"{fn}: distance {distance} must be at least 1")
    return sq


def _ring(fn, inner, outer):
    if not (isinstance(inner, (int, float, np.integer, np.floating)) and isinstance(outer, (int, float, np.integer, np.floating))) \
            or not 0 <= inner < outer:
        raise KGLibraryError(f"{fn}: need 0 <= inner < outer (inner {inner!r}, outer {outer!r})")
    return square(fn, inner, 0), square(fn, outer)


def _want(fn, want):
    w = (want,) if isinstance(want, str) else tuple(want)
    if not w or any(k not in ("d2", "nearest") for k in w):
        raise KGLibraryError(f"{fn}: want {want!r} must name 'd2', 'nearest' or both")
    return "d2" in w, "nearest" in w


# ---- host statements of the semantics ---------------------------------------------------------------------------------------------------

def _offsets(max_d2):
    R = math.isqrt(max_d2)
    return [(dy, dx, dy * dy + dx * dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1) if 0 < dy * dy + dx * dx <= max_d2]


def _transform_host(fn, labels, max_d2, frame):
    """-> (d2 int64 [nimg, H, W], nearest int64 [nimg, H, W], maps int64, was_2d)"""
    max_d2 = _max_d2(fn, max_d2)
    maps, single = _labelmaps.host_maps(fn, labels, True)
    maps = maps.astype(np.int64)
    _, H, W = maps.shape
    d2 = np.full(maps.shape, max_d2 + 1, np.int64)
    near = maps.copy()
    for dy, dx, dd in _offsets(max_d2):                               # q = p + (dy, dx), over the p for which q lies in the image
        ya, yb, xa, xb = max(0, -dy), H - max(0, dy), max(0, -dx), W - max(0, dx)
        if ya >= yb or xa >= xb:
            continue
        P = (slice(None), slice(ya, yb), slice(xa, xb))
        u = maps[:, ya + dy:yb + dy, xa + dx:xb + dx]
        bd, bn = d2[P], near[P]                                       # views: the assignments below write d2 and near
        take = (u != maps[P]) & ((dd < bd) | ((dd == bd) & (u < bn)))
        bd[take] = dd
        bn[take] = u[take]
    if frame:
        yy, xx = np.mgrid[0:H, 0:W]
        f = np.minimum(np.minimum(yy + 1, xx + 1), np.minimum(H - yy, W - xx)).astype(np.int64)
        d2 = np.where(f * f <= max_d2, np.minimum(d2, f * f), d2)
    return d2, near, maps, single


def _shaped(a, single):
    a = a.astype(np.int32)
    return a[0] if single else a


def distance_host(labels, max_d2, frame=False):
    """Integer label map(s) [H, W] or [nimg, H, W] -> (d2, nearest), int32 of the same shape."""
    d2, near, _, single = _transform_host("distance_host", labels, max_d2, frame)
    return _shaped(d2, single), _shaped(near, single)


def _regrow_host(fn, labels, op, lo2, hi2, frame=False):
    d2, near, maps, single = _transform_host(fn, labels, hi2, frame)
    if op == EXPAND:
        out = np.where((maps == 0) & (d2 <= hi2), near, maps)
    elif op == RING:
        out = np.where((maps == 0) & (d2 > lo2) & (d2 <= hi2), near, 0)
    else:
        out = np.where((maps != 0) & (d2 > hi2), maps, 0)
    return _shaped(out, single)


def expand_labels_host(labels, distance):
    """Every background (0) pixel within `distance` of a non-zero pixel takes the value of the nearest one; everything else is kept.  This is
    skimage.segmentation.expand_labels with THIS project's tie rule: among equally near values the smallest (signed) wins, whatever the
    order of the pixels -- skimage takes whichever scipy's distance transform happened to index."""
    return _regrow_host("expand_labels_host", labels, EXPAND, 0, square("expand_labels_host", distance))


def ring_labels_host(labels, inner, outer):
    """The part of expand_labels(labels, outer) that lies farther than `inner` from its object, on background pixels; 0 elsewhere."""
    lo2, hi2 = _ring("ring_labels_host", inner, outer)
    return _regrow_host("ring_labels_host", labels, RING, lo2, hi2)


def shrink_labels_host(labels, distance, frame=False):
    """A non-zero pixel survives iff it lies farther than `distance` from every pixel with another value (and from the frame, if asked)."""
    return _regrow_host("shrink_labels_host", labels, SHRINK, 0, square("shrink_labels_host", distance), bool(frame))


def _result(rows, max_d2):
    """int64 [m, 4] = (d2max, y, x, count) -> the structured result"""
    rows = np.asarray(rows, np.int64).reshape(-1, 4)
    out = np.zeros(len(rows), INSCRIBED_DTYPE)
    out["d2max"], out["y"], out["x"], out["count"] = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
    out["radius"] = np.sqrt(rows[:, 0].astype(np.float64))
    out["saturated"] = rows[:, 0] > max_d2
    return out


def inscribed_rows_host(labels, d2, jobs):
    """kg_label_inscribed in NumPy: maps and d2 [nimg, H, W], jobs [m, 6] -> int64 [m, 4] = (d2max, y, x, count), nothing split."""
    maps, dd = np.asarray(labels), np.asarray(d2)
    nimg, H, W = maps.shape
    out = np.zeros((len(jobs), 4), np.int64)
    out[:, 1:3] = -1
    for k, (i, v, y1, x1, y2, x2) in enumerate(np.asarray(jobs, np.int64).tolist()):
        y1, x1, y2, x2 = max(y1, 0), max(x1, 0), min(y2, H), min(x2, W)
        if not 0 <= i < nimg or y2 <= y1 or x2 <= x1:
            continue
        ys, xs = np.nonzero(maps[i, y1:y2, x1:x2] == v)
        if len(ys) == 0:
            continue
        ys, xs = ys + y1, xs + x1
        val = dd[i, ys, xs].astype(np.int64)
        top = np.flatnonzero(val == val.max())                        # np.nonzero is row-major: the first is the smallest y * W + x
        out[k] = val.max(), ys[top[0]], xs[top[0]], len(ys)
    return out


def inscribed_host(labels, n=None, jobs=None, stats=None, max_d2=MAX_D2, frame=True):
    """The inscribed circle of every instance -> a structured array (INSCRIBED_DTYPE), one element per instance (or per job):
      d2max      the largest d2 over the instance's pixels (inside its box): the squared radius of the largest circle around a pixel centre
                 that meets no other value (nor, with frame, the outside of the image)
      radius     sqrt(d2max), float64
      y, x       the pixel with the smallest y * W + x among those that attain d2max: it lies inside the instance; -1 without a pixel
      count      the pixels of the id inside its box
      saturated  d2max > max_d2: the object is thicker than the search radius, and radius is only a lower bound
    n / jobs / stats: what is measured, as measure.measure_host / measure.measure take them."""
    d2, _, maps, _ = _transform_host("inscribed_host", labels, max_d2, frame)
    j = _labelmaps.job_table("inscribed_host", maps, n, jobs, stats, labelmetrics.label_stats_host)
    return _result(inscribed_rows_host(maps, d2, j), int(max_d2))


def combine_bands(rows, owner, n_jobs, W):
    """rows int64 [m2, 4] of the pieces split_jobs made, owner int [m2] -> int64 [n_jobs, 4].  The rows are NOT additive: the largest d2max
    wins, then the smallest y * W + x; the counts are added; a job whose pieces hold no pixel is {0, -1, -1, 0}."""
    rows = np.asarray(rows, np.int64).reshape(-1, 4)
    owner = np.asarray(owner, np.int64).reshape(-1)
    if len(rows) != len(owner) or (len(owner) and (owner.min() < 0 or owner.max() >= n_jobs)):
        raise KGLibraryError(f"combine_bands: rows {rows.shape}, {len(owner)} owners, {n_jobs} jobs")
    out = np.zeros((int(n_jobs), 4), np.int64)
    out[:, 1:3] = -1
    np.add.at(out[:, 3], owner, rows[:, 3])
    live = rows[:, 3] > 0
    key = np.full(int(n_jobs), -1, np.int64)
    big = 2 ** 31 - 1
    np.maximum.at(key, owner[live], rows[live, 0] * 2 ** 31 + (big - (rows[live, 1] * int(W) + rows[live, 2])))
    have = key >= 0
    idx = big - key[have] % 2 ** 31
    out[have, 0], out[have, 1], out[have, 2] = key[have] // 2 ** 31, idx // int(W), idx % int(W)
    return out


# ---- device -----------------------------------------------------------------------------------------------------------------------------

def _stack(fn, labels):
    """-> (device int32 [nimg, H, W], the caller's shape); the transform has no side bound"""
    return _labelmaps.device_stack(fn, labels, bound=False)


def distance(labels, max_d2, frame=False, want=("d2", "nearest")):
    """distance_host on the device: labels = device int32 [H, W] or [nimg, H, W] -> (d2, nearest), device int32 of the same shape; an output
    that `want` does not name is None and is never written.  ONE launch for the whole stack, no copy, no synchronisation."""
    import torch
    from ._lib import ptr, stream_ptr
    max_d2 = _max_d2("distance", max_d2)
    w_d2, w_near = _want("distance", want)
    lab, shape = _stack("distance", labels)
    nimg, H, W = lab.shape
    d2 = torch.empty_like(lab) if w_d2 else None
    near = torch.empty_like(lab) if w_near else None
    with torch.cuda.device(lab.device):
        _lib.call("kg_label_distance", ptr(lab), nimg, H, W, max_d2, int(bool(frame)), ptr(d2), ptr(near), stream_ptr())
    return (None if d2 is None else d2.view(shape)), (None if near is None else near.view(shape))


def _regrow(fn, labels, op, lo2, hi2, frame=False):
    import torch
    from ._lib import ptr, stream_ptr
    lab, shape = _stack(fn, labels)
    nimg, H, W = lab.shape
    out = torch.empty_like(lab)
    with torch.cuda.device(lab.device):
        _lib.call("kg_label_regrow", ptr(lab), nimg, H, W, hi2, int(bool(frame)), op, lo2, hi2, ptr(out), stream_ptr())
    return out.view(shape)


def expand_labels(labels, distance):
    """expand_labels_host on the device (skimage.segmentation.expand_labels with this project's tie rule: among equally near values the
    smallest wins): device int32 [H, W] or [nimg, H, W] -> a new device int32 map.  One launch; d2 and nearest never reach memory."""
    return _regrow("expand_labels", labels, EXPAND, 0, square("expand_labels", distance))


def ring_labels(labels, inner, outer):
    """ring_labels_host on the device.  One launch."""
    lo2, hi2 = _ring("ring_labels", inner, outer)
    return _regrow("ring_labels", labels, RING, lo2, hi2)


def shrink_labels(labels, distance, frame=False):
    """shrink_labels_host on the device.  One launch."""
    return _regrow("shrink_labels", labels, SHRINK, 0, square("shrink_labels", distance), frame)


def inscribed_rows(labels, d2, jobs):
    """kg_label_inscribed as it is: labels, d2 device int32 [H, W] or [nimg, H, W]; jobs host int [m, 6] (uploaded once) or a device int32
    tensor -> device int32 [m, 4].  One launch, no copy back, nothing split."""
    import torch
    from ._lib import ptr, stream_ptr
    lab, _ = _stack("inscribed", labels)
    dd, _ = _stack("inscribed", d2)
    if dd.shape != lab.shape or dd.device != lab.device:
        raise KGLibraryError(f"inscribed: d2 of {tuple(dd.shape)} for label maps of {tuple(lab.shape)}: one shape and one device")
    nimg, H, W = lab.shape
    jd = _labelmaps.device_jobs("inscribed", jobs, 6, "(img, id, y1, x1, y2, x2)", lab.device)
    m = jd.shape[0]
    out = torch.empty(m, 4, dtype=torch.int32, device=lab.device)
    with torch.cuda.device(lab.device):
        _lib.call("kg_label_inscribed", ptr(lab), ptr(dd), nimg, H, W, ptr(jd) if m else None, m, ptr(out) if m else None, stream_ptr())
    return out


def inscribed(labels, n=None, jobs=None, stats=None, max_d2=MAX_D2, frame=True, max_job_pixels=65536):
    """inscribed_host on the device -> the same structured array (host).  labels: device int32 [H, W] or [nimg, H, W]; n / jobs / stats as
    measure.measure takes them (without stats the boxes come from labelmetrics.label_stats, its launches and one copy per map).  A job
    whose box holds more than max_job_pixels pixels is walked in bands (split_jobs, combine_bands).  One kg_label_distance launch (d2
    only), one kg_label_inscribed launch, one upload (the jobs) and one device -> host copy (the rows)."""
    max_d2 = _max_d2("inscribed", max_d2)
    lab, _ = _stack("inscribed", labels)
    j = _labelmaps.job_table("inscribed", lab, n, jobs, stats, labelmetrics.label_stats)
    pieces, owner = labelmetrics.split_jobs(j, max_job_pixels)
    d2, _ = distance(lab, max_d2, frame, want=("d2",))
    rows = inscribed_rows(lab, d2, pieces).cpu().numpy()
    return _result(combine_bands(rows, owner, len(j), lab.shape[2]), max_d2)


# ---- Instances ----------------------------------------------------------------------------------------------------------------------------

def _grown_jobs(table, distance, H, W):
    """The table's boxes grown by ceil(distance) and clamped -> (jobs int32 [k, 5] = (id, y1, x1, y2, x2) of the ids with a visible pixel,
    their rows)."""
    t = np.asarray(table, np.int64).reshape(-1, 8)
    grow = int(math.ceil(distance))
    rows = np.flatnonzero(t[:, 1] > 0)
    box = t[rows, 2:6] + [-grow, -grow, grow, grow]
    box[:, :2] = np.clip(box[:, :2], 0, [H, W]); box[:, 2:] = np.clip(box[:, 2:], 0, [H, W])
    return np.ascontiguousarray(np.concatenate([rows[:, None] + 1, box], 1).astype(np.int32)).reshape(-1, 5), rows


def _grown_table(old, rows, new_rows):
    """The refreshed table: the rows of the ids with a visible pixel replaced, area_full kept; an instance without one keeps its zero row."""
    out = np.zeros((len(old), 8), np.int64)
    out[:, 0] = np.asarray(old, np.int64).reshape(-1, 8)[:, 0]
    out[rows, 1:] = np.asarray(new_rows, np.int64).reshape(-1, 8)[:, 1:]
    return out


def expand_instances(inst, distance):
    """expand_labels for an Instances / TiledInstances: a new object of the same type with labels replaced and the table refreshed
    (tiling.table_from_labels over the old boxes grown by ceil(distance) and clamped); area_full, dets and masks are kept, so the ids still
    mean rows of dets, and an instance with no visible pixel keeps its zero row.  A host label map goes through expand_labels_host."""
    return expand_instances_batch([inst], distance)[0]


def expand_instances_batch(insts, distance):
    """expand_instances for predict_instances' list (entries may be None): ONE kg_label_regrow launch for all images of one output size,
    one kg_label_table launch per image and one device -> host copy of the tables per size."""
    import torch
    square("expand_instances", distance)
    out = list(insts)

    def host_one(i, inst, lab):
        new = expand_labels_host(lab, distance)
        jobs, rows = _grown_jobs(inst.table, distance, *lab.shape)
        out[i] = components.like(inst, new, _grown_table(inst.table, rows, tiling.table_from_labels_host(new, jobs)))
    for idx, stack, H, W in _labelmaps.size_batches("expand_instances", insts, host_one):
        new = expand_labels(stack, distance)
        jr = [_grown_jobs(insts[i].table, distance, H, W) for i in idx]
        tabs = [tiling.table_from_labels(new[k], jr[k][0]) for k in range(len(idx))]
        got = (torch.cat(tabs) if len(tabs) > 1 else tabs[0]).cpu().numpy()
        for k, (i, a, b) in enumerate(_labelmaps.deal(insts, idx, [len(r[1]) for r in jr])):
            out[i] = components.like(insts[i], new[k], _grown_table(insts[i].table, jr[k][1], got[a:b]))
    return out
