"""Tiled whole-image inference: an image of any size is cut into overlapping tiles of the network's input size, every tile goes through
predict(packed=True) at native resolution, and the per-tile results are joined into ONE instance label map and ONE per-instance table.

    predict_tiled = cut_tiles -> predict(packed=True) per chunk of tiles -> assemble

The *_host functions state the semantics in NumPy (the CPU route, and the yardstick of the GPU tests); cut_tiles, stitch and
table_from_labels run on the device (csrc/tiling.hip), as does the per-tile label map (kg_instance_labels with global ids).

Semantics
  plan        plan_axis(L, t, overlap): one tile at 0 if L <= t (the image is padded), else n = 1 + ceil((L - t) / (t - overlap)) tiles at
              origin_k = k (L - t) // (n - 1): consecutive origins differ by at most t - overlap and the last tile ends at L.  The grid of an
              image is ys x xs, tile t = r * len(xs) + c.
  cores       along an axis the boundary between consecutive tiles a < b is (a + t + b) // 2, the middle of their overlap; tile k owns
              [bound_{k-1}, bound_k), the first core starts at -inf, the last ends at +inf: every point of the plane has exactly one owner.
  tile input  float32 [3, th, tw] = float32(u8) / 255 - 0.5 (two float32 operations), channels in the image's order; a pixel outside the
              image is -0.5, the value of pixel 0.
  per tile    predict's dets are the rounded, clamped boxes in tile pixels, rows in descending confidence.  The bits of the masks of a
              tile that reaches past the image (an image smaller than the tile) are cleared outside the image.
  ownership   a detection is kept by its tile iff its box centre ((y1 + y2) / 2 + y0, (x1 + x2) / 2 + x0), float64, lies in the tile's core.
  order, ids  the kept detections of all tiles sorted by (-conf, tile, row in tile): that is the priority order.
  duplicates  walking that order, a detection is dropped iff an earlier kept detection from a DIFFERENT tile has box IoU > nms_thresh with it
              (the float64 expression of the reference's nms.py on the global, unclipped boxes); pairs from one tile are never compared.
              Position r of what is left has id r + 1.
  label map   labels[y, x] = the smallest id among the instances whose mask covers the pixel, 0 if none: label_map_host on the global dense
              masks in id order.  No global mask is ever built: each tile's kept rows, in ascending id, give a label map of the tile with
              the global ids as values, and the stitched map is, per pixel, the smallest non-zero value over the tiles covering it.
  table       int64 [n, 8] (instances.TABLE_COLUMNS): area_full = the set bits of the instance's tile mask (inside the image); the other
              columns = the pixels with labels == id inside the instance's global det box.  A mask never leaves its det box when the
              tile size is the network input size (the second resize of the paste-back is then the identity).

An object larger than the overlap is cut at the edge of the tile that owns its centre: choose an overlap of at least the largest object."""
import numpy as np

from . import _lib, instances
from ._labelmaps import device_jobs, is_device, upload_jobs
from .bitmasks import BitMasks
from .instances import Instances

KGLibraryError = _lib.KGLibraryError


# ---- plan ---------------------------------------------------------------------------------------------------------------------------------

def plan_axis(L, t, overlap):
    """Origins of the tiles of size t along an axis of length L: int64 [n], ascending."""
    L, t, overlap = int(L), int(t), int(overlap)
    if L < 1 or t < 1 or not 0 <= overlap < t:
        raise KGLibraryError(f"plan_axis: length {L}, tile {t}, overlap {overlap}")
    if L <= t:
        return np.zeros(1, np.int64)
    n = 1 + -(-(L - t) // (t - overlap))
    return np.arange(n, dtype=np.int64) * (L - t) // (n - 1)


def axis_bounds(origins, t):
    """int64 [n - 1]: the boundary between the cores of consecutive tiles."""
    o = np.asarray(origins, np.int64)
    return (o[:-1] + int(t) + o[1:]) // 2


class TilePlan:
    """The tile grid of an H x W image.  ys, xs: int32 origins along the axes; th, tw; origins: int32 [T, 2] (y0, x0) of tile
    t = r * len(xs) + c; cores: float64 [T, 4] (y_lo, y_hi, x_lo, x_hi), half-open, the outer ones infinite."""
    __slots__ = ("ys", "xs", "th", "tw", "H", "W", "origins", "cores", "ybounds", "xbounds")

    def __init__(self, ys, xs, th, tw, H, W):
        self.ys, self.xs = np.ascontiguousarray(ys, np.int32), np.ascontiguousarray(xs, np.int32)
        self.th, self.tw, self.H, self.W = int(th), int(tw), int(H), int(W)
        self.ybounds, self.xbounds = axis_bounds(self.ys, th), axis_bounds(self.xs, tw)
        gy, gx = np.meshgrid(self.ys, self.xs, indexing="ij")
        self.origins = np.ascontiguousarray(np.stack([gy.reshape(-1), gx.reshape(-1)], 1).astype(np.int32))
        cy = np.concatenate([[-np.inf], self.ybounds, [np.inf]])
        cx = np.concatenate([[-np.inf], self.xbounds, [np.inf]])
        r, c = np.divmod(np.arange(len(self)), len(self.xs))
        self.cores = np.stack([cy[r], cy[r + 1], cx[c], cx[c + 1]], 1)

    def __len__(self):
        return len(self.ys) * len(self.xs)

    @property
    def shape(self):
        return len(self.ys), len(self.xs)

    def valid(self, t):
        """(vh, vw): the part of tile t that lies inside the image."""
        y0, x0 = self.origins[t]
        return min(self.th, self.H - int(y0)), min(self.tw, self.W - int(x0))


def plan(H, W, tile=(512, 512), overlap=128):
    """TilePlan of an H x W image.  tile: (th, tw) or one int, multiples of 32 (the network's stride); 0 <= overlap < min(tile)."""
    th, tw = (tile, tile) if np.isscalar(tile) else tile
    th, tw, H, W, ov = int(th), int(tw), int(H), int(W), int(overlap)
    if th < 32 or tw < 32 or th % 32 or tw % 32:
        raise KGLibraryError(f"plan: tile {th} x {tw} must be multiples of 32")
    if not 0 <= ov < min(th, tw) or ov != overlap:
        raise KGLibraryError(f"plan: overlap {overlap} must be an integer in [0, {min(th, tw)})")
    if H < 1 or W < 1:
        raise KGLibraryError(f"plan: image {H} x {W}")
    return TilePlan(plan_axis(H, th, ov), plan_axis(W, tw, ov), th, tw, H, W)


def owner(plan, cy, cx):
    """Tile that owns every point (cy, cx) (float64 arrays): the one whose core holds it."""
    r = np.searchsorted(plan.ybounds, np.asarray(cy, np.float64), side="right")
    c = np.searchsorted(plan.xbounds, np.asarray(cx, np.float64), side="right")
    return r * len(plan.xs) + c


def owner_keep(plan, t, dets):
    """bool [n]: the detections of tile t (predict's dets, tile pixels) whose box centre lies in the tile's core."""
    d = np.asarray(dets, np.float32).reshape(-1, 5).astype(np.float64)
    y0, x0 = plan.origins[t]
    return owner(plan, (d[:, 0] + d[:, 2]) / 2 + float(y0), (d[:, 1] + d[:, 3]) / 2 + float(x0)) == t


# ---- duplicates across tiles (host) -------------------------------------------------------------------------------------------------------

def _iou(boxes, area, kept, later):
    """IoU of the kept box(es) with the later one(s) (indices, broadcast against each other): the float64 expression of the reference's
    nms.py, whose union is (area_later - inter) + area_kept, in that order."""
    yy1 = np.maximum(boxes[later, 0], boxes[kept, 0]); xx1 = np.maximum(boxes[later, 1], boxes[kept, 1])
    yy2 = np.minimum(boxes[later, 2], boxes[kept, 2]); xx2 = np.minimum(boxes[later, 3], boxes[kept, 3])
    inter = np.maximum(0., xx2 - xx1) * np.maximum(0., yy2 - yy1)
    union = (area[later] - inter) + area[kept]
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / union


def suppress_across_tiles_plain(boxes, tile, nms_thresh=0.5):
    """The rule as stated, O(n^2): boxes float64 [n, 4] (global y1, x1, y2, x2) in priority order, tile int [n] -> bool [n] kept."""
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    tile = np.asarray(tile, np.int64).reshape(-1)
    area = (b[:, 3] - b[:, 1]) * (b[:, 2] - b[:, 0])
    keep = np.ones(len(b), bool)
    for i in range(1, len(b)):
        earlier = np.flatnonzero(keep[:i] & (tile[:i] != tile[i]))               # kept, from a different tile
        keep[i] = not np.any(_iou(b, area, earlier, i) > nms_thresh)
    return keep


def touches_other_tile(plan, boxes, tile):
    """bool [n]: the box has an intersection of positive area with the rectangle of a tile other than its own."""
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    tile = np.asarray(tile, np.int64).reshape(-1)
    ys, xs = plan.ys.astype(np.float64), plan.xs.astype(np.float64)
    ry = np.minimum(b[:, None, 2], ys[None] + plan.th) - np.maximum(b[:, None, 0], ys[None]) > 0          # [n, ny]
    cx = np.minimum(b[:, None, 3], xs[None] + plan.tw) - np.maximum(b[:, None, 1], xs[None]) > 0          # [n, nx]
    r, c = np.divmod(tile, len(xs))
    k = np.arange(len(b))
    own = (ry[k, r] & cx[k, c]).astype(np.int64) if len(b) else np.zeros(0, np.int64)
    return ry.sum(1) * cx.sum(1) - own > 0


def suppress_across_tiles(boxes, tile, nms_thresh=0.5, plan=None):
    """bool [n] kept, equal to suppress_across_tiles_plain.  With a plan (and nms_thresh >= 0) only the detections whose box touches an
    overlap band are compared.  The rule: every det box lies inside its tile's rectangle, so a box that has no intersection of positive
    area with the rectangle of any OTHER tile has intersection 0, hence IoU 0 (or 0 / 0) <= nms_thresh, with every box of every other
    tile: it is never dropped and never drops anything, and leaving it out changes nothing."""
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    tile = np.asarray(tile, np.int64).reshape(-1)
    keep = np.ones(len(b), bool)
    cand = np.arange(len(b))
    if plan is not None and nms_thresh >= 0:
        cand = np.flatnonzero(touches_other_tile(plan, b, tile))
    area = (b[:, 3] - b[:, 1]) * (b[:, 2] - b[:, 0])
    alive = np.ones(len(cand), bool)
    for a in range(len(cand)):                       # greedy in priority order: a kept box drops the later boxes of other tiles it overlaps
        if not alive[a]:
            continue
        later = cand[a + 1:]
        hit = (_iou(b, area, cand[a], later) > nms_thresh) & (tile[later] != tile[cand[a]])
        alive[a + 1:] &= ~hit
    keep[cand[~alive]] = False
    return keep


# ---- selection shared by assemble and assemble_host ---------------------------------------------------------------------------------------

class Selection:
    """What the host decides from the dets of all tiles: in id order, tile int32 [n], row int64 [n] (row within the tile), origin int32
    [n, 2], dets float32 [n, 5] (global, clipped to the image), boxes int32 [n, 4] (the same as integers, y1 <= y2 and x1 <= x2)."""
    __slots__ = ("tile", "row", "origin", "dets", "boxes")


def select(plan, tile_dets, nms_thresh=0.5):
    """tile_dets: per tile None or predict's dets float32 [n, 5] -> Selection (ownership, order, duplicates across tiles, ids)."""
    if len(tile_dets) != len(plan):
        raise KGLibraryError(f"tiling: {len(tile_dets)} entries for {len(plan)} tiles")
    tiles, rows, dd = [], [], []
    for t, d in enumerate(tile_dets):
        if d is None or len(d) == 0:
            continue
        d = np.asarray(d, np.float32).reshape(-1, 5)
        k = np.flatnonzero(owner_keep(plan, t, d))
        tiles.append(np.full(len(k), t, np.int64)); rows.append(k); dd.append(d[k])
    tile = np.concatenate(tiles) if tiles else np.zeros(0, np.int64)
    row = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    det = np.concatenate(dd) if dd else np.zeros((0, 5), np.float32)
    order = np.lexsort((row, tile, -det[:, 4].astype(np.float64)))
    tile, row, det = tile[order], row[order], det[order]
    org = plan.origins[tile].reshape(-1, 2)
    glob = det[:, :4].astype(np.float64) + np.concatenate([org, org], 1)
    keep = suppress_across_tiles(glob, tile, nms_thresh, plan)
    tile, row, det, org, glob = tile[keep], row[keep], det[keep], org[keep], glob[keep]
    clip = np.clip(glob, 0, [plan.H, plan.W, plan.H, plan.W])
    s = Selection()
    s.tile, s.row, s.origin = tile.astype(np.int32), row, np.ascontiguousarray(org, np.int32)
    s.dets = np.concatenate([clip, det[:, 4:5].astype(np.float64)], 1).astype(np.float32)
    b = np.rint(clip).astype(np.int32)
    b[:, 2:] = np.maximum(b[:, 2:], b[:, :2])
    s.boxes = b
    return s


class TiledInstances(Instances):
    """predict_tiled's result: labels = device int32 [H, W] (assemble_host: a NumPy array); dets = float32 [n, 5] (y1, x1, y2, x2, conf) in
    global pixels, clipped to the image, in id order; table = host int64 [n, 8]; masks = None; tile int32 [n]; origin int32 [n, 2];
    tile_masks = the tile-local mask rows in id order (BitMasks; assemble_host: uint8 [n, th, tw]): tile_masks[i] placed at origin[i]
    is the full mask of instance i + 1.  measurements, neighbours, runs, contours, hulls, quantiles, texture, midlines and crops are Instances': None unless
    asked for (measure=, neighbours=, runs=, contours=, hulls=, quantiles=, texture=, thin= of predict_tiled).  parent is Instances' too: None unless a split ran
    (split=, split.py); then dets, tile and origin hold a copy of the parent's row for every new id and tile_masks keeps the rows of the
    parents only: tile_masks[parent[i]] placed at origin[i] is the mask instance i + 1 came from."""
    __slots__ = ("tile", "origin", "tile_masks")

    def __init__(self, labels, dets, table, tile, origin, tile_masks):
        super().__init__(labels, dets, table, None)
        self.tile, self.origin, self.tile_masks = tile, origin, tile_masks


# ---- host statements ----------------------------------------------------------------------------------------------------------------------

def _host_image(image):
    a = np.asarray(image)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise KGLibraryError("tiling: image must be uint8 [H, W, 3]")
    return a


def cut_tiles_host(image, plan):
    """uint8 [H, W, 3] -> float32 [T, 3, th, tw]."""
    a = _host_image(image)
    if a.shape[:2] != (plan.H, plan.W):
        raise KGLibraryError(f"cut_tiles: image {a.shape[:2]} for a plan of {plan.H} x {plan.W}")
    out = np.full((len(plan), 3, plan.th, plan.tw), np.float32(0) / np.float32(255) - np.float32(0.5), np.float32)
    for t, (y0, x0) in enumerate(plan.origins):
        vh, vw = plan.valid(t)
        v = a[y0:y0 + vh, x0:x0 + vw].astype(np.float32) / np.float32(255) - np.float32(0.5)
        out[t, :, :vh, :vw] = v.transpose(2, 0, 1)
    return out


def clip_words_host(words, h, w, vh, vw):
    """uint64 words [n, >= h * ceil(w / 64)] of h x w masks -> a copy with every bit at y >= vh or x >= vw cleared; the words behind the
    mask (the padding word) are left as they are, and the full window (vh, vw) == (h, w) changes nothing at all."""
    out = np.array(np.asarray(words).astype(np.uint64, copy=False), copy=True)
    wpr = (int(w) + 63) // 64
    if not (0 <= vh <= h and 0 <= vw <= w) or out.ndim != 2 or out.shape[1] < h * wpr:
        raise KGLibraryError(f"clip_words: window {vh} x {vw} of {h} x {w} masks, words {out.shape}")
    if (vh, vw) == (h, w):
        return out
    keep = np.zeros((h, wpr), np.uint64)
    for k in range(wpr):
        bits = min(max(int(vw) - 64 * k, 0), 64)
        keep[:vh, k] = np.uint64((1 << bits) - 1)
    out[:, :h * wpr] &= keep.reshape(-1)
    return out


def stitch_host(tile_labels, plan):
    """int [T, th, tw] per-tile label maps (values >= 0) -> int32 [H, W]: per pixel the smallest non-zero value over the covering tiles."""
    tl = np.asarray(tile_labels)
    if tl.shape != (len(plan), plan.th, plan.tw):
        raise KGLibraryError(f"stitch: tile labels {tl.shape} for {len(plan)} tiles of {plan.th} x {plan.tw}")
    out = np.zeros((plan.H, plan.W), np.int32)
    for t, (y0, x0) in enumerate(plan.origins):
        vh, vw = plan.valid(t)
        a, g = tl[t, :vh, :vw], out[y0:y0 + vh, x0:x0 + vw]
        g[...] = np.where((a != 0) & ((g == 0) | (a < g)), a, g)
    return out


def _jobs(jobs, H, W):
    j = np.asarray(jobs)
    if j.ndim != 2 or j.shape[1] != 5 or j.dtype.kind not in "iu":
        raise KGLibraryError("table_from_labels: jobs must be integers [n, 5] = (id, y1, x1, y2, x2)")
    j = j.astype(np.int64)
    if len(j) and not (np.all(j[:, 0] > 0) and np.all(j[:, 0] < 2 ** 31) and np.all(j[:, 1:3] >= 0) and np.all(j[:, 1:3] <= j[:, 3:5])
                       and np.all(j[:, 3] <= H) and np.all(j[:, 4] <= W)):
        raise KGLibraryError(f"table_from_labels: a job has id <= 0 or a box that is not 0 <= y1 <= y2 <= {H}, 0 <= x1 <= x2 <= {W}")
    return np.ascontiguousarray(j.astype(np.int32))


def table_from_labels_host(labels, jobs, area_full=None):
    """int64 [n, 8] (TABLE_COLUMNS): column 0 = area_full (zeros without it), columns 1-7 from the pixels with labels == id inside the
    job's box."""
    lab = np.asarray(labels)
    j = _jobs(jobs, *lab.shape)
    out = np.zeros((len(j), 8), np.int64)
    if area_full is not None:
        out[:, 0] = np.asarray(area_full, np.int64).reshape(len(j))
    for k, (i, y1, x1, y2, x2) in enumerate(j):
        ys, xs = np.nonzero(lab[y1:y2, x1:x2] == i)
        if len(ys):
            ys, xs = ys + y1, xs + x1
            out[k, 1:] = len(ys), ys.min(), xs.min(), ys.max() + 1, xs.max() + 1, ys.sum(dtype=np.int64), xs.sum(dtype=np.int64)
    return out


def _ids_jobs(sel):
    n = len(sel.tile)
    return np.concatenate([np.arange(1, n + 1, dtype=np.int32)[:, None], sel.boxes], 1)


def assemble_host(plan, per_tile_preds, nms_thresh=0.5):
    """assemble on dense host masks: per tile None or [masks [n, th, tw] (any non-zero value is foreground), dets float32 [n, 5]]."""
    sel = select(plan, [None if p is None else p[1] for p in per_tile_preds], nms_thresh)
    n, T = len(sel.tile), len(plan)
    tile_labels = np.zeros((T, plan.th, plan.tw), np.int32)
    tile_masks = np.zeros((n, plan.th, plan.tw), np.uint8)
    for t in np.unique(sel.tile):
        k = np.flatnonzero(sel.tile == t)                                   # ascending id
        vh, vw = plan.valid(t)
        m = np.asarray(per_tile_preds[t][0])[sel.row[k]] != 0
        m[:, vh:] = False
        m[:, :, vw:] = False
        tile_masks[k] = m
        tile_labels[t] = instances.label_map_host(m, ids=k + 1)
    labels = stitch_host(tile_labels, plan)
    table = table_from_labels_host(labels, _ids_jobs(sel), tile_masks.sum((1, 2), dtype=np.int64))
    return TiledInstances(labels, sel.dets, table, sel.tile, sel.origin, tile_masks)


# ---- device -------------------------------------------------------------------------------------------------------------------------------

def _cuda(fn, t, dtype, what):
    if not is_device(t):
        raise KGLibraryError(f"{fn} (MI355X build) needs {what} on a GPU device; the host route is {fn}_host")
    if t.dtype != dtype:
        raise KGLibraryError(f"{fn}: {what} must be {dtype}")
    return t.contiguous()


def cut_tiles(image, plan, device=None):
    """image: host uint8 [H, W, 3] (uploaded once) or a device uint8 tensor -> device float32 [T, 3, th, tw] (kg_tile_cut, one launch)."""
    import torch
    from . import ops
    from ._lib import ptr, stream_ptr
    if not torch.is_tensor(image):
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise KGLibraryError("cut_tiles (MI355X build) needs a GPU device; the host route is cut_tiles_host")
        image = ops.h2d(_host_image(image), dev)
    img = _cuda("cut_tiles", image, torch.uint8, "the image")
    if tuple(img.shape) != (plan.H, plan.W, 3):
        raise KGLibraryError(f"cut_tiles: image {tuple(img.shape)} for a plan of {plan.H} x {plan.W} x 3")
    out = torch.empty(len(plan), 3, plan.th, plan.tw, dtype=torch.float32, device=img.device)
    with torch.cuda.device(img.device):
        _lib.call("kg_tile_cut", ptr(img), plan.H, plan.W, plan.ys.ctypes.data, len(plan.ys), plan.xs.ctypes.data, len(plan.xs), plan.th, plan.tw,
                  ptr(out), stream_ptr())
    return out


def clip_masks(masks, vh, vw):
    """Clears in place every bit of the BitMasks at y >= vh or x >= vw (kg_bitmask_clip).  The words must be contiguous."""
    from ._lib import ptr, stream_ptr, c_long
    wd = masks.words
    if wd.device.type != "cuda" or not wd.is_contiguous():
        raise KGLibraryError("clip_masks (MI355X build) needs contiguous words on a GPU device")
    import torch
    with torch.cuda.device(wd.device):
        _lib.call("kg_bitmask_clip", ptr(wd) if len(masks) else None, c_long(wd.shape[1]), len(masks), masks.h, masks.w, int(vh), int(vw),
                  stream_ptr())
    return masks


def stitch(tile_labels, plan):
    """device int32 [T, th, tw] (values >= 0) -> device int32 [H, W] (kg_tile_stitch, one launch, every pixel written once)."""
    import torch
    from ._lib import ptr, stream_ptr
    tl = _cuda("stitch", tile_labels, torch.int32, "the tile label maps")
    if tuple(tl.shape) != (len(plan), plan.th, plan.tw):
        raise KGLibraryError(f"stitch: tile labels {tuple(tl.shape)} for {len(plan)} tiles of {plan.th} x {plan.tw}")
    labels = torch.empty(plan.H, plan.W, dtype=torch.int32, device=tl.device)
    with torch.cuda.device(tl.device):
        _lib.call("kg_tile_stitch", ptr(tl), plan.ys.ctypes.data, len(plan.ys), plan.xs.ctypes.data, len(plan.xs), plan.th, plan.tw, plan.H, plan.W,
                  ptr(labels), stream_ptr())
    return labels


def table_from_labels(labels, jobs, area_full=None):
    """labels: device int32 [H, W]; jobs: host int [n, 5] = (id, y1, x1, y2, x2), validated here and uploaded once (or a device int32
    tensor the caller built from validated boxes); area_full: device int64 [n] or None -> device int64 [n, 8] (kg_label_table)."""
    import torch
    from ._lib import ptr, stream_ptr
    lab = _cuda("table_from_labels", labels, torch.int32, "the label map")
    if lab.dim() != 2:
        raise KGLibraryError("table_from_labels: labels must be [H, W]")
    H, W = lab.shape
    dev = lab.device
    if torch.is_tensor(jobs):
        jd = device_jobs("table_from_labels", _cuda("table_from_labels", jobs, torch.int32, "device jobs"), 5, "", dev, "n", "labels'")
    else:
        jd = upload_jobs(_jobs(jobs, H, W), dev)                     # _jobs is the stricter validation: nothing is scanned twice
    n = jd.shape[0]
    if area_full is not None:
        area_full = _cuda("table_from_labels", area_full, torch.int64, "area_full")
        if tuple(area_full.shape) != (n,) or area_full.device != dev:
            raise KGLibraryError(f"table_from_labels: area_full must be int64 [{n}] on the labels' device")
    table = torch.empty(n, 8, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.call("kg_label_table", ptr(lab), H, W, ptr(jd) if n else None, n, ptr(area_full) if n else None, ptr(table) if n else None,
                  stream_ptr())
    return table


def assemble(plan, per_tile_preds, nms_thresh=0.5, device=None, stage=None, clean=None, split=None):
    """Everything after the per-tile predict calls.  per_tile_preds: per tile None or predict(packed=True)'s [BitMasks of th x tw, dets];
    the masks of a tile that reaches past the image are clipped in place.  device: where an empty result's labels go when no tile has a
    detection (default: the masks' device, else the current GPU).  stage: optional callable(name), called on the stream before the label
    launches, the stitch, the table and at the end (tools/tiling_bench.py puts device events there).
    Host <-> device traffic: ONE upload (the job table, with the ids and the row indices of the two mask gathers behind it) and ONE
    device -> host copy (the global table).
    clean: None, or a dict of components.clean's policy arguments: the stitched map then goes through components.clean_instances (its
    launches and copies on top).
    split: None, a distance in pixels, or a dict of split.split_instances' arguments: the (cleaned) stitched map then goes through
    split.split_instances (its launches and copies on top); None adds no launch and no import."""
    if split is not None:
        from . import split as _split
        return _split.split_instances(assemble(plan, per_tile_preds, nms_thresh, device, stage, clean),
                                      **(dict(split) if isinstance(split, dict) else {"distance": split}))
    if clean is not None:
        from . import components
        return components.clean_instances(assemble(plan, per_tile_preds, nms_thresh, device, stage), **dict(clean))
    import torch
    from . import ops
    mark = stage if stage is not None else (lambda name: None)
    T = len(plan)
    if len(per_tile_preds) != T:
        raise KGLibraryError(f"assemble: {len(per_tile_preds)} entries for {T} tiles")
    for p in per_tile_preds:
        if p is None:
            continue
        if not isinstance(p[0], BitMasks) or (p[0].h, p[0].w) != (plan.th, plan.tw) or len(p[0]) != len(p[1]):
            raise KGLibraryError(f"assemble: every tile needs [BitMasks of {plan.th} x {plan.tw}, dets of as many rows]")
        if p[0].device.type != "cuda":
            raise KGLibraryError("assemble (MI355X build) needs masks on a GPU device; the host route is assemble_host")
        device = p[0].device
    sel = select(plan, [None if p is None else p[1] for p in per_tile_preds], nms_thresh)
    n = len(sel.tile)
    if n == 0:
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        return TiledInstances(torch.zeros(plan.H, plan.W, dtype=torch.int32, device=dev), sel.dets, np.zeros((0, 8), np.int64), sel.tile, sel.origin,
                              BitMasks.empty(plan.th, plan.tw, dev))
    dev = device
    # rows grouped by tile, ascending id within a tile: the order of the label launch (g = position in that order -> id - 1)
    g = np.lexsort((np.arange(n), sel.tile))
    row_start = np.searchsorted(sel.tile[g], np.arange(T + 1), side="left")
    back = np.empty(n, np.int64)
    back[g] = np.arange(n)
    jobs = _jobs(_ids_jobs(sel)[g], plan.H, plan.W)
    up = ops.h2d(np.concatenate([jobs.reshape(-1), sel.row[g].astype(np.int32), back.astype(np.int32)]), dev)
    jobs_d, rows_d, back_d = up[:5 * n].view(n, 5), up[5 * n:6 * n], up[6 * n:]
    ids_d = jobs_d[:, 0].contiguous()
    mark("labels")
    grouped = BitMasks.empty(plan.th, plan.tw, dev, n)
    for t in range(T):
        a, b = int(row_start[t]), int(row_start[t + 1])
        if a == b:
            continue
        m = per_tile_preds[t][0]
        vh, vw = plan.valid(t)
        if (vh, vw) != (plan.th, plan.tw):
            if not m.words.is_contiguous():
                m = BitMasks(m.words.contiguous(), m.h, m.w)
            clip_masks(m, vh, vw)
        torch.index_select(m.words, 0, rows_d[a:b], out=grouped.words[a:b])
    tile_labels, tile_table = instances.label_map(grouped, row_start, ids=ids_d)
    mark("stitch")
    labels = stitch(tile_labels, plan)
    mark("table")
    table = table_from_labels(labels, jobs_d, tile_table[:, 0].contiguous())
    tile_masks = grouped[back_d]
    mark("end")
    host = table.cpu().numpy()[back]
    return TiledInstances(labels, sel.dets, host, sel.tile, sel.origin, tile_masks)


def predict_tiled(model, image, tile=(512, 512), overlap=128, batch=8, nms_thresh=0.5, seg_thresh=0.5, max_workspace_bytes=None, stage=None,
                  clean=None, measure=False, expand=None, neighbours=None, runs=None, contours=None, hulls=None, quantiles=None, split=None, texture=None, thin=None, crops=None):
    """Instance segmentation of a whole image at native resolution -> TiledInstances.  image: host uint8 [H, W, 3] (uploaded once, to the
    model's device) or a device uint8 tensor; tile: the network input size, (th, tw) or one int, multiples of 32; overlap: pixels two
    neighbouring tiles share at least (choose it at least as large as the largest object: an object is cut at the edge of the tile that
    owns its centre); batch: tiles per predict call; clean: None, or a dict of components.clean's policy arguments (assemble);
    expand: None, or a distance in pixels (a number, at most 64): every instance of the STITCHED map is then grown by that much without
    two instances merging (distance.expand_instances: no tile seams), after the clean-up and before the measurements;
    measure: with True the result's `measurements` holds measure.measure_instances of the final (cleaned, expanded, if asked) label map
    against the uploaded uint8 image -- one more launch, one more upload (the jobs) and one more device -> host copy (the rows);
    neighbours: None; True, or a dict of neighbours.neighbours_instances' keyword arguments (connectivity, expand, slots,
    max_job_pixels): the result's `neighbours` then holds the touching-neighbour graph of the final label map (neighbours.py) -- one more
    launch, upload and copy back per round of paging.  None adds no launch and no import;
    runs: None; True, or a dict of runlengths.runs_instances' keyword arguments (max_job_pixels): the result's `runs` then holds the
    run-length lists of the instances (runlengths.py: Kaggle rows, COCO counts), taken last, on the final label map -- two more launches
    and two more copies back.  None adds no launch and no import;
    contours: None; True, or a dict (contours.contours_instances takes no keyword arguments yet, so an empty one): the result's
    `contours` then holds the polygon rings of the instances (contours.py: COCO polygons, GeoJSON), taken last, next to runs, on the
    final label map -- two more launches and two more copies back.  None adds no launch and no import;
    hulls: None; True, or a dict of hulls.hulls_instances' keyword arguments (max_job_pixels): the result's `hulls` then holds the convex
    hull of the instances (hulls.py: solidity, Feret diameters, hull rings), taken last, next to contours, on the final label map -- one
    more launch and one more copy back.  None adds no launch and no import;
    quantiles: None; True, or a dict of intensity.quantiles_instances' keyword arguments (q, max_job_pixels): the result's `quantiles`
    then holds the intensity order statistics of the instances (intensity.py: median, quartiles, a 5 % / 95 % range) against the uploaded
    uint8 image, taken next to measure on the final label map -- one more launch, upload and copy back.  None adds no launch and no
    import;
    texture: None; True, or a dict of texture.texture_instances' keyword arguments (levels, distance, channels, range, max_job_pixels;
    "image": another uint8 / uint16 [H, W, C] image to take the texture of): the result's `texture` then holds the co-occurrence matrices
    of the instances (texture.py: Haralick's features) against the uploaded uint8 image, taken next to quantiles on the final label map
    -- one more launch, upload and copy back.  None adds no launch and no import;
    split: None; a distance in pixels (1 .. 64), or a dict of split.split_instances' arguments (distance, connectivity, min_seed_area,
    frame, only): merged instances of the STITCHED map are then split into their core seeds' regions (split.py, through assemble), after
    the clean-up and before the expansion and everything else; the result has `parent` set, dets / tile / origin extended by a copy of
    the parent's row per new id and tile_masks unchanged.  None adds no launch and no import;
    thin: None; True, or a dict of thinning.thin_instances' keyword arguments (max_passes): the result's `midlines` then holds the midline
    of the instances of the STITCHED map (thinning.py: length, tips, branch points, and the midline map `skel`; no tile seams), taken
    next to the other measurements on the final label map -- one more upload, launch and copy back.  None adds no launch and no
    import;
    crops: None; True (patches of the uploaded uint8 image), another uint8 / uint16 [H, W, C] image, or a dict of crops.crops_instances'
    keyword arguments (size, window, margin, angle, side, flip, mode, masked, fill, masks; "image": another image, None for masks only):
    the result's `crops` then holds one fixed-size patch and mask per instance, on the device (crops.py: what a second network takes),
    taken last, next to hulls, on the final label map -- one more upload (the table) and launch, nothing copied back.  None adds no launch
    and no import."""
    import torch
    from . import inference
    quantiles = None if quantiles is False else quantiles
    texture = None if texture is False else texture
    crops = None if crops is False else crops
    crops_own = crops is True or (isinstance(crops, dict) and "image" not in crops)     # crops of the uploaded image
    if int(batch) < 1:
        raise KGLibraryError(f"predict_tiled: batch {batch}")
    mark = stage if stage is not None else (lambda name: None)
    if torch.is_tensor(image):
        shape, dev = tuple(image.shape), image.device
    else:
        shape, dev = _host_image(image).shape, next(model.parameters()).device
        if measure or quantiles is not None or texture is not None or crops_own:   # the one upload serves the tiles and the measurements
            from . import ops
            image = ops.h2d(_host_image(image), dev)
    if len(shape) != 3 or shape[2] != 3:
        raise KGLibraryError("predict_tiled: image must be uint8 [H, W, 3]")
    pl = plan(shape[0], shape[1], tile, overlap)
    mark("cut")
    x = cut_tiles(image, pl, dev)
    mark("predict")
    preds = []
    for a in range(0, len(pl), int(batch)):
        preds += inference.predict(model, x[a:a + int(batch)], nms_thresh, seg_thresh, None, max_workspace_bytes=max_workspace_bytes, packed=True)
    out = assemble(pl, preds, nms_thresh, dev, stage, clean, split)
    if expand is not None:
        from . import distance
        out = distance.expand_instances(out, expand)
    if measure:
        from . import measure as _measure
        out.measurements = _measure.measure_instances(out, image)
    if quantiles is not None:
        from . import intensity
        out.quantiles = intensity.quantiles_instances(out, image, **({} if quantiles is True else dict(quantiles)))
    if texture is not None:
        from . import texture as _texture
        kw = {} if texture is True else dict(texture)
        out.texture = _texture.texture_instances(out, kw.pop("image", image), **kw)
    if thin is not None and thin is not False:
        from . import thinning
        out.midlines = thinning.thin_instances(out, **({} if thin is True else dict(thin)))
    if neighbours is not None and neighbours is not False:
        from . import neighbours as _neighbours
        out.neighbours = _neighbours.neighbours_instances(out, **({} if neighbours is True else dict(neighbours)))
    if runs is not None and runs is not False:
        from . import runlengths
        out.runs = runlengths.runs_instances(out, **({} if runs is True else dict(runs)))
    if contours is not None and contours is not False:
        from . import contours as _contours
        out.contours = _contours.contours_instances(out, **({} if contours is True else dict(contours)))
    if hulls is not None and hulls is not False:
        from . import hulls as _hulls
        out.hulls = _hulls.hulls_instances(out, **({} if hulls is True else dict(hulls)))
    if crops is not None:
        from . import crops as _crops
        kw = dict(crops) if isinstance(crops, dict) else {} if crops is True else {"image": crops}
        out.crops = _crops.crops_instances(out, kw.pop("image", image), **kw)
    return out
