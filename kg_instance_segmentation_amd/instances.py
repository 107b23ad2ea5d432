"""Instance results from bit-packed masks: one label map per image, a table of exact per-instance integers, the reference's mask
overlay, and Kaggle run-length lists.

predict() ends where the reference's post_processing ends: n full-size binary masks per image, which may overlap.  What users read from
them -- counts, areas, centroids, boxes, a non-overlapping submission -- comes from ONE label map per image: every pixel holds the id
of the instance it belongs to, overlaps resolved.  label_map / overlay run on the device from the words (csrc/instances.hip); the *_host
functions state the same semantics in NumPy over dense [n, H, W] arrays (the CPU route, and the yardstick of the GPU tests); run-length
encoding here is host NumPy over a label map copied back (runlengths.py lists the runs on the device, with these functions as its
yardstick).

Semantics (include/kgnet_hip.h, kg_instance_labels / kg_instance_overlay):
  label map   0 where no mask of the image covers the pixel, else the id of the first covering row in priority order.  Priority order is
              row order unless `priority` is given; predict's rows are sorted by descending confidence, so by default the more confident
              instance wins an overlap.  The id of a row is its index within its image + 1: ids always mean "row of dets".
  table       int64 [n, 8], one line per row: area_full, area_visible, y1, x1, y2, x2 (half-open box of the visible pixels, zeros if
              none), sum_y, sum_x over the visible pixels.  The centroid is (sum_y, sum_x) / area_visible, in the caller's float64.
  overlay     test.py:29-37 (apply_mask) for every row in ascending row order, as test.py:171-185 loops: every covered channel becomes
              (uint8)(v * (1 - alpha) + alpha * color[c] * 255) in float64, truncated; the blend compounds where masks overlap.
  run lengths pixels numbered down the columns first, then left to right, from 1; a list is (start, length) pairs in ascending order."""
import numpy as np

from . import _lib
from .bitmasks import BitMasks

TABLE_COLUMNS = ("area_full", "area_visible", "y1", "x1", "y2", "x2", "sum_y", "sum_x")


class Instances:
    """One image's result of inference.predict_instances: labels = device int32 [h, w]; dets = float32 [n, 5], predict's; table = host
    int64 [n, 8] (TABLE_COLUMNS); masks = the BitMasks; measurements = None unless asked for (measure=, measure.py: a Measurements);
    neighbours = None unless asked for (neighbours=, neighbours.py: a Neighbours); runs = None unless asked for (runs=, runlengths.py: a
    RunLengths); contours = None unless asked for (contours=, contours.py: a Contours); hulls = None unless asked for (hulls=, hulls.py: a
    Hulls); quantiles = None unless asked for (quantiles=, intensity.py: a Quantiles); texture = None unless asked for (texture=, texture.py:
    a CoMatrices); midlines = None unless asked for (thin=, thinning.py: a Midlines, which keeps the midline map `skel`); crops = None unless asked for (crops=, crops.py: a Crops, patches and masks on the device); parent = None unless a split ran (split=, split.py): then int32 [n], and dets holds a copy of the parent's row for every new id while masks keeps the rows of the parents only:
    masks[parent[i]] is the mask instance i + 1 came from (parent[i] == i for an instance that was there before the split)."""
    __slots__ = ("labels", "dets", "table", "masks", "measurements", "neighbours", "runs", "contours", "hulls", "quantiles", "texture", "midlines", "crops", "parent")

    def __init__(self, labels, dets, table, masks):
        self.labels, self.dets, self.table, self.masks = labels, dets, table, masks
        self.measurements = None
        self.neighbours = None
        self.runs = None
        self.contours = None
        self.hulls = None
        self.quantiles = None
        self.texture = None
        self.midlines = None
        self.crops = None
        self.parent = None

    def __len__(self):
        return len(self.dets)

    def centroids(self):
        """float64 [n, 2] (y, x) of the visible pixels; NaN for a hidden instance."""
        t = self.table.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return t[:, 6:8] / t[:, 1:2]


# ---- host statements of the semantics ------------------------------------------------------------------------------------------------

def _order(n, priority):
    if priority is None:
        return np.arange(n)
    p = np.asarray(priority, np.int64).reshape(-1)
    if len(p) != n or not np.array_equal(np.sort(p), np.arange(n)):
        raise ValueError("priority must be a permutation of the rows")
    return p


def _winner(dense_masks, priority):
    """int64 [H, W]: the row that wins every pixel, -1 where none does."""
    m = np.asarray(dense_masks)
    if m.ndim != 3:
        raise ValueError("dense masks must be [n, H, W]")
    win = np.full(m.shape[1:], -1, np.int64)
    for k in _order(len(m), priority)[::-1]:          # painted from the lowest priority up: the first in priority order stays on top
        win[m[k] != 0] = k
    return win


def label_map_host(dense_masks, priority=None, ids=None):
    """[n, H, W] masks of ONE image (any non-zero value is foreground) -> int32 [H, W].  priority: a permutation of the rows, highest
    priority first (default: row order).  ids: the value written for every row (default: row + 1)."""
    win = _winner(dense_masks, priority)
    n = len(dense_masks)
    val = np.arange(1, n + 1, dtype=np.int32) if ids is None else np.asarray(ids, np.int32).reshape(n)
    return np.where(win >= 0, np.concatenate([val, np.zeros(1, np.int32)])[win], 0).astype(np.int32)


def table_host(dense_masks, priority=None):
    """int64 [n, 8] (TABLE_COLUMNS) of ONE image, one line per row of dense_masks whatever the priority."""
    m = np.asarray(dense_masks)
    win = _winner(m, priority)
    out = np.zeros((len(m), 8), np.int64)
    for k in range(len(m)):
        out[k, 0] = np.count_nonzero(m[k])
        ys, xs = np.nonzero(win == k)
        if len(ys):
            out[k, 1:] = len(ys), ys.min(), xs.min(), ys.max() + 1, xs.max() + 1, ys.sum(dtype=np.int64), xs.sum(dtype=np.int64)
    return out


def overlay_host(image, dense_masks, colors, alpha=0.8):
    """uint8 [H, W, 3] image blended with every mask in ascending row order (a copy is returned).  colors: float64 [n, 3] in [0, 1]."""
    out = np.array(image, dtype=np.uint8, copy=True)
    col = np.asarray(colors, np.float64).reshape(-1, 3)
    m = np.asarray(dense_masks)
    if out.ndim != 3 or out.shape[2] != 3 or m.shape[1:] != out.shape[:2] or len(col) != len(m):
        raise ValueError("overlay_host: image [H, W, 3], masks [n, H, W], colors [n, 3]")
    alpha = float(alpha)
    for k in range(len(m)):
        sel = m[k] != 0
        for c in range(3):
            out[sel, c] = out[sel, c] * (1 - alpha) + alpha * col[k, c] * 255      # float64; the store into uint8 truncates
    return out


# ---- run-length lists (host) ---------------------------------------------------------------------------------------------------------

def rle_encode(labels, ids=None):
    """Label map [H, W] -> {id: int64 [runs, 2] of (start, length)}: one pass over the transposed map yields the runs of every id.
    ids: ids to report (an id absent from the map gets an empty list); default: the ids present."""
    lab = np.asarray(labels)
    if lab.ndim != 2:
        raise ValueError("rle_encode: labels must be [H, W]")
    flat = np.ascontiguousarray(lab.T).reshape(-1)
    starts = np.concatenate([[0], np.flatnonzero(flat[1:] != flat[:-1]) + 1]) if flat.size else np.zeros(0, np.int64)
    lengths = np.diff(np.concatenate([starts, [flat.size]]))
    vals = flat[starts]
    fg = vals != 0
    starts, lengths, vals = starts[fg], lengths[fg], vals[fg]
    order = np.argsort(vals, kind="stable")                # runs of one id stay in ascending order
    uniq, first = np.unique(vals[order], return_index=True)
    runs = np.stack([starts[order] + 1, lengths[order]], 1).astype(np.int64)
    out = {int(u): r for u, r in zip(uniq, np.split(runs, first[1:]))}
    if ids is not None:
        out = {int(i): out.get(int(i), np.zeros((0, 2), np.int64)) for i in ids}
    return out


def rle_decode(runs, H, W):
    """int64 [runs, 2] -> uint8 [H, W] mask; a dict {id: runs} (rle_encode's output) -> int32 [H, W] label map."""
    if isinstance(runs, dict):
        lab = np.zeros((H, W), np.int32)
        for i, r in runs.items():
            lab[rle_decode(r, H, W) != 0] = i
        return lab
    flat = np.zeros(H * W, np.uint8)
    for s, l in np.asarray(runs, np.int64).reshape(-1, 2):
        if s < 1 or l < 1 or s - 1 + l > H * W:
            raise ValueError(f"rle_decode: run ({s}, {l}) outside a {H} x {W} image")
        flat[s - 1:s - 1 + l] = 1
    return np.ascontiguousarray(flat.reshape(W, H).T)


def rle_string(runs):
    """'start length start length ...' (the EncodedPixels column of a Kaggle nuclei submission)."""
    return " ".join(str(int(v)) for v in np.asarray(runs, np.int64).reshape(-1))


# ---- device -----------------------------------------------------------------------------------------------------------------------------

def _ranges(row_start, n):
    rs = np.array([0, n], np.int32) if row_start is None else np.ascontiguousarray(np.asarray(row_start, np.int64).reshape(-1))
    if len(rs) < 2 or rs[0] != 0 or rs[-1] != n or np.any(np.diff(rs) < 0):
        raise _lib.KGLibraryError(f"row_start must run from 0 to n = {n} without decreasing")
    return np.ascontiguousarray(rs.astype(np.int32))


def _device_masks(fn, masks):
    import torch
    if not isinstance(masks, BitMasks):
        raise _lib.KGLibraryError(f"{fn}: masks must be a bitmasks.BitMasks")
    if not torch.is_tensor(masks.words) or masks.words.device.type != "cuda":
        raise _lib.KGLibraryError(f"{fn} (MI355X build) needs masks on a GPU device; the host route is {fn}_host")
    return masks


def label_map(masks, row_start=None, priority=None, with_table=True, ids=None):
    """BitMasks of one or more images of one size -> (labels device int32 [nimg, H, W], table device int64 [n, 8] or None).
    row_start: host ints [nimg + 1], image i owns rows [row_start[i], row_start[i + 1]) (default: one image holding all rows).
    priority: host int array over all rows, within every image a permutation of that image's rows, highest priority first (default:
    row order).  Ids and table lines always refer to the rows of `masks` as given.
    ids: host int32 [n] (or a device int32 tensor [n]), the value written for every row instead of its index within its image + 1
    (tiling.py: the ids of a whole image's instances in the label map of one tile); it cannot be given together with priority."""
    import torch
    from ._lib import ptr, stream_ptr, c_long
    masks = _device_masks("label_map", masks)
    n, h, w = masks.shape
    rs = _ranges(row_start, n)
    nimg = len(rs) - 1
    prio = None
    if ids is not None:
        if priority is not None:
            raise _lib.KGLibraryError("label_map: ids cannot be given together with priority")
        if torch.is_tensor(ids):
            if ids.dtype != torch.int32 or ids.device != masks.device or tuple(ids.shape) != (n,):
                raise _lib.KGLibraryError(f"label_map: device ids must be int32 [{n}] on the masks' device")
            ids = ids.contiguous() if n else None
        else:
            v = np.asarray(ids)
            if v.shape != (n,) or v.dtype.kind not in "iu" or (n and (v.min() < -2 ** 31 or v.max() > 2 ** 31 - 1)):
                raise _lib.KGLibraryError(f"label_map: ids must be {n} integers that fit int32")
            from . import ops
            ids = ops.h2d(np.ascontiguousarray(v.astype(np.int32)), masks.device) if n else None
    if priority is not None:
        p = np.asarray(priority, np.int64).reshape(-1)
        if len(p) != n:
            raise _lib.KGLibraryError(f"label_map: priority has {len(p)} entries for {n} rows")
        for i in range(nimg):
            if not np.array_equal(np.sort(p[rs[i]:rs[i + 1]]), np.arange(rs[i], rs[i + 1])):
                raise _lib.KGLibraryError(f"label_map: priority is not a permutation of the rows of image {i}")
        from . import ops
        dev = masks.device
        local = (p - np.repeat(rs[:-1].astype(np.int64), np.diff(rs)) + 1).astype(np.int32)
        prio = ops.h2d(p, dev) if n else torch.empty(0, dtype=torch.int64, device=dev)
        ids = ops.h2d(local, dev) if n else None
        masks = masks[prio]
    wd = masks.words.contiguous()
    dev = wd.device
    labels = torch.empty(nimg, h, w, dtype=torch.int32, device=dev)
    table = torch.empty(n, 8, dtype=torch.int64, device=dev) if with_table else None
    with torch.cuda.device(dev):
        _lib.call("kg_instance_labels", ptr(wd), c_long(wd.shape[1]), n, rs.ctypes.data, nimg, h, w, ptr(ids), ptr(labels),
                  ptr(table) if n else None, stream_ptr())
    if table is not None and prio is not None and n:
        back = torch.empty_like(table)
        back[prio] = table
        table = back
    return labels, table


def overlay(images, masks, colors, alpha=0.8, row_start=None, out=None):
    """images: device uint8 [nimg, H, W, 3] (or [H, W, 3]) tensor, or a host array that is uploaded once; colors: float64 [n, 3] in [0, 1]
    (host array or device tensor), the caller's; alpha in [0, 1].  Returns a device uint8 tensor of the images' shape: a new one, or
    `out` (which may be `images` itself)."""
    import torch
    from . import ops
    from ._lib import ptr, stream_ptr, c_long, c_double
    masks = _device_masks("overlay", masks)
    n, h, w = masks.shape
    dev = masks.device
    rs = _ranges(row_start, n)
    nimg = len(rs) - 1
    if not torch.is_tensor(images):
        a = np.asarray(images)
        if a.dtype != np.uint8:
            raise _lib.KGLibraryError("overlay: images must be uint8")
        images = ops.h2d(a, dev)
    if images.dtype != torch.uint8 or images.device != dev:
        raise _lib.KGLibraryError("overlay: images must be uint8 on the masks' device")
    shape = tuple(images.shape)
    if shape not in ((nimg, h, w, 3),) + (((h, w, 3),) if nimg == 1 else ()):
        raise _lib.KGLibraryError(f"overlay: images {shape} for {nimg} image(s) of {h} x {w} x 3")
    img = images if images.is_contiguous() else images.contiguous()
    if torch.is_tensor(colors):
        col = colors.to(device=dev, dtype=torch.float64).contiguous()
    else:
        c = np.ascontiguousarray(np.asarray(colors, np.float64).reshape(-1, 3))
        col = ops.h2d(c, dev) if c.size else torch.empty(0, 3, dtype=torch.float64, device=dev)
    if tuple(col.shape) != (n, 3):
        raise _lib.KGLibraryError(f"overlay: colors {tuple(col.shape)} for {n} masks")
    if out is None:
        out = torch.empty_like(img)
    elif out.dtype != torch.uint8 or out.device != dev or tuple(out.shape) != shape or not out.is_contiguous():
        raise _lib.KGLibraryError("overlay: out must be a contiguous uint8 tensor of the images' shape on their device")
    wd = masks.words.contiguous()
    with torch.cuda.device(dev):
        _lib.call("kg_instance_overlay", ptr(img), ptr(wd), c_long(wd.shape[1]), n, rs.ctypes.data, nimg, h, w, ptr(col), c_double(float(alpha)),
                  ptr(out), stream_ptr())
    return out


def join_masks(parts):
    """BitMasks.cat without the copy when the parts are consecutive slices of one buffer (predict's per-image masks of one size are)."""
    import torch
    w0 = parts[0].words
    ld, total = w0.shape[1], sum(len(p) for p in parts)
    nxt = w0.data_ptr()
    for p in parts:
        if (p.h, p.w) != (parts[0].h, parts[0].w):
            raise ValueError("join_masks: masks of different sizes")
        pw = p.words
        if not (pw.is_contiguous() and pw.untyped_storage().data_ptr() == w0.untyped_storage().data_ptr() and (len(p) == 0 or pw.data_ptr() == nxt)):
            return BitMasks.cat(parts)
        nxt += len(p) * ld * 8
    return BitMasks(torch.as_strided(w0, (total, ld), (ld, 1), w0.storage_offset()), parts[0].h, parts[0].w)
