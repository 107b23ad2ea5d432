"""Label-map evaluation: the Kaggle DSB-2018 score, AJI, PQ, Dice and the reference's AP straight from two instance label maps.

predict_instances and predict_tiled end in ONE int32 label map per image; evaluation.Evaluator needs one mask per detection at one common
size, which predict_tiled never builds (at 1040 x 1388 with ~800 instances that is ~1.2 GB as bytes, and the ground truth as much again).
Every metric named above is a function of one small object, the CONTINGENCY of the two maps: the area of every predicted id, the area of
every ground-truth id, and the pixel count of every (predicted id, GT id) pair that meets -- a few thousand integers for two 2048^2 maps.

    label_stats      per id {area, y1, x1, y2, x2} of one map               (kg_label_stats, csrc/labelmetrics.hip)
    candidate_pairs  the id pairs whose boxes overlap, with the box they share (host)
    contingency      the pixel count of every candidate pair inside that box (kg_label_inter_jobs), pairs that do not meet dropped
    match / kaggle_score / panoptic / aji / dice   pure host float64 over a Contingency
    LabelEvaluator   accumulates them over images; evaluate_tiled(model, samples) runs predict_tiled and scores every image;
                     boundary= adds the boundary distances of the true-positive pairs (boundaries.py): hd, hd95, assd, nsd

The *_host functions state the same semantics in NumPy (the CPU route, and the yardstick of the GPU tests); every count is an exact integer.

Semantics
  ids         a label map of n instances holds 0 (background) and the ids 1 .. n; any other value is an error that names the pixel count.
  stats       int64 [n, 5], row id - 1 = {area, y1, x1, y2, x2} of the pixels equal to id, half-open box, zeros for an id with no pixel.
  candidates  every pair (id_a, id_b) of ids with non-zero area whose boxes overlap (max(y1) < min(y2), the same in x), in lexicographic
              order; the job's box is the intersection of the two boxes: outside it the pair cannot meet.
  bands       a job whose box holds more than max_job_pixels pixels is split on the host into bands of whole rows (of row pieces, for a
              box wider than max_job_pixels) of at most that many pixels; the band counts are added on the host in int64.
  iou         I / (A_p + A_g - I) in float64; a pair that does not meet has 0."""
import math

import numpy as np

from . import _lib, evaluation, instances, polygons
from ._labelmaps import device_jobs, device_maps, host_maps, is_device
from .bitmasks import BitMasks, unpack_host

KGLibraryError = _lib.KGLibraryError
STATS_COLUMNS = ("area", "y1", "x1", "y2", "x2")


class Contingency:
    """area_pred int64 [n_pred], area_gt int64 [n_gt]; pairs int32 [k, 2] = the (pred id, gt id) that meet, 1-based, in lexicographic order;
    inter int64 [k] > 0, their pixel counts."""
    __slots__ = ("area_pred", "area_gt", "pairs", "inter")

    def __init__(self, area_pred, area_gt, pairs, inter):
        self.area_pred = np.ascontiguousarray(area_pred, np.int64).reshape(-1)
        self.area_gt = np.ascontiguousarray(area_gt, np.int64).reshape(-1)
        self.pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        self.inter = np.ascontiguousarray(inter, np.int64).reshape(-1)
        if len(self.pairs) != len(self.inter):
            raise ValueError("Contingency: one count per pair")

    def iou(self):
        """float64 [k]: the IoU of every pair."""
        p, g = self.pairs[:, 0].astype(np.int64) - 1, self.pairs[:, 1].astype(np.int64) - 1
        i = self.inter.astype(np.float64)
        return i / (self.area_pred[p] + self.area_gt[g] - self.inter).astype(np.float64) if len(i) else i

    def __eq__(self, other):
        return isinstance(other, Contingency) and all(np.array_equal(getattr(self, k), getattr(other, k)) for k in self.__slots__)

    __hash__ = None


# ---- host statements of the semantics ---------------------------------------------------------------------------------------------------

def _count(fn, n):
    if int(n) != n or not 0 <= int(n) < 2 ** 31 // 5:
        raise KGLibraryError(f"{fn}: instance count {n}")
    return int(n)


def label_stats_counts_host(labels, n):
    """(stats int64 [n, 5], invalid): the raw entry's two outputs -- the stats of every valid id are exact whatever the other pixels hold."""
    lab = host_maps("label_stats_host", labels, False).astype(np.int64)
    n = _count("label_stats_host", n)
    ys, xs = np.nonzero((lab >= 1) & (lab <= n))
    ids = lab[ys, xs] - 1
    out = np.zeros((n, 5), np.int64)
    out[:, 0] = np.bincount(ids, minlength=n)
    big = np.iinfo(np.int64).max
    y1, x1 = np.full(n, big), np.full(n, big)
    np.minimum.at(y1, ids, ys); np.minimum.at(x1, ids, xs)
    np.maximum.at(out[:, 3], ids, ys + 1); np.maximum.at(out[:, 4], ids, xs + 1)
    have = out[:, 0] > 0
    out[have, 1], out[have, 2] = y1[have], x1[have]
    return out, int(np.count_nonzero((lab < 0) | (lab > n)))


def _raise_invalid(fn, invalid, n):
    if invalid:
        raise KGLibraryError(f"{fn}: {invalid} pixel(s) of the label map lie outside [0, {n}]")


def label_stats_host(labels, n):
    """Label map [H, W] with ids 1 .. n -> int64 [n, 5] (STATS_COLUMNS); raises when a pixel lies outside [0, n]."""
    stats, invalid = label_stats_counts_host(labels, n)
    _raise_invalid("label_stats_host", invalid, int(n))
    return stats


def _stats(fn, stats, n=None):
    s = np.asarray(stats)
    if s.ndim != 2 or s.shape[1] != 5 or s.dtype.kind not in "iu" or (n is not None and len(s) != n):
        raise KGLibraryError(f"{fn}: stats must be integers [{'n' if n is None else n}, 5] = (area, y1, x1, y2, x2)")
    return s.astype(np.int64)


def candidate_pairs(stats_a, stats_b):
    """int32 [m, 6] jobs (id_a, id_b, y1, x1, y2, x2): every pair of ids with non-zero area whose half-open boxes overlap, in lexicographic
    order of (id_a, id_b), with the intersection of the two boxes."""
    a, b = _stats("candidate_pairs", stats_a), _stats("candidate_pairs", stats_b)
    ia, ib = np.flatnonzero(a[:, 0] > 0), np.flatnonzero(b[:, 0] > 0)
    if len(ia) == 0 or len(ib) == 0:
        return np.zeros((0, 6), np.int32)
    # Not all n_a * n_b pairs are tested: with b sorted by y1, the rows of b that can overlap a in y are a contiguous range -- b.y1 < a.y2,
    # and b.y1 > a.y1 - (the tallest box of b), which b.y2 > a.y1 implies.  The exact test follows on those alone.
    ib = ib[np.argsort(b[ib, 1], kind="stable")]
    by1, tallest = b[ib, 1], int((b[ib, 3] - b[ib, 1]).max())
    lo = np.searchsorted(by1, a[ia, 1] - tallest, side="right")
    cnt = np.maximum(np.searchsorted(by1, a[ia, 3], side="left") - lo, 0)
    i = np.repeat(ia, cnt)
    j = ib[np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt - lo, cnt)]
    y1 = np.maximum(a[i, 1], b[j, 1]); x1 = np.maximum(a[i, 2], b[j, 2])
    y2 = np.minimum(a[i, 3], b[j, 3]); x2 = np.minimum(a[i, 4], b[j, 4])
    k = np.flatnonzero((y1 < y2) & (x1 < x2))
    k = k[np.lexsort((j[k], i[k]))]                                  # lexicographic in (id_a, id_b)
    return np.ascontiguousarray(np.stack([i[k] + 1, j[k] + 1, y1[k], x1[k], y2[k], x2[k]], 1).astype(np.int32)).reshape(-1, 6)


def split_jobs(jobs, max_job_pixels=65536):
    """Jobs int [m, 6] -> (pieces int32 [m2, 6], owner int64 [m2]): a job whose box holds more than max_job_pixels pixels becomes bands of
    at most that many pixels that tile its box exactly, in row-major order; owner[k] is the job piece k belongs to."""
    j = np.asarray(jobs, np.int64).reshape(-1, 6)
    cap = int(max_job_pixels)
    if cap < 1:
        raise KGLibraryError(f"split_jobs: max_job_pixels {max_job_pixels}")
    h, w = np.maximum(j[:, 4] - j[:, 2], 0), np.maximum(j[:, 5] - j[:, 3], 0)
    small = h * w <= cap
    pieces, owner = [j[small]], [np.flatnonzero(small)]
    for k in np.flatnonzero(~small):
        ia, ib, y1, x1, y2, x2 = j[k]
        cw = min(int(w[k]), cap)                                     # a box wider than the cap is cut along x too
        rows = max(cap // cw, 1)
        ys, xs = np.arange(y1, y2, rows), np.arange(x1, x2, cw)
        gy, gx = np.meshgrid(ys, xs, indexing="ij")
        gy, gx = gy.reshape(-1), gx.reshape(-1)
        pieces.append(np.stack([np.full(len(gy), ia), np.full(len(gy), ib), gy, gx, np.minimum(gy + rows, y2), np.minimum(gx + cw, x2)], 1))
        owner.append(np.full(len(gy), k))
    pieces, owner = np.concatenate(pieces), np.concatenate(owner)
    order = np.argsort(owner, kind="stable")
    return np.ascontiguousarray(pieces[order].astype(np.int32)), owner[order].astype(np.int64)


def inter_jobs_host(a, b, jobs):
    """int64 [m]: per job (id_a, id_b, y1, x1, y2, x2) the pixels of the box, clamped to the map, with a == id_a and b == id_b."""
    a, b = host_maps("inter_jobs_host", a, False), host_maps("inter_jobs_host", b, False)
    if a.shape != b.shape:
        raise KGLibraryError(f"inter_jobs_host: maps of {a.shape} and {b.shape}")
    H, W = a.shape
    out = np.zeros(len(jobs), np.int64)
    for k, (ia, ib, y1, x1, y2, x2) in enumerate(np.asarray(jobs, np.int64).reshape(-1, 6)):
        y1, x1, y2, x2 = max(y1, 0), max(x1, 0), min(y2, H), min(x2, W)
        if y2 > y1 and x2 > x1:
            out[k] = np.count_nonzero((a[y1:y2, x1:x2] == ia) & (b[y1:y2, x1:x2] == ib))
    return out


def contingency_host(pred, gt, n_pred, n_gt):
    """The Contingency of two host label maps: ONE np.unique over pred * (n_gt + 1) + gt."""
    p, g = host_maps("contingency_host", pred, False), host_maps("contingency_host", gt, False)
    n_pred, n_gt = _count("contingency_host", n_pred), _count("contingency_host", n_gt)
    if p.shape != g.shape:
        raise KGLibraryError(f"contingency_host: a predicted map of {p.shape} against a ground truth of {g.shape}")
    _raise_invalid("contingency_host (pred)", int(np.count_nonzero((p < 0) | (p > n_pred))), n_pred)
    _raise_invalid("contingency_host (gt)", int(np.count_nonzero((g < 0) | (g > n_gt))), n_gt)
    key, cnt = np.unique(p.astype(np.int64) * (n_gt + 1) + g, return_counts=True)
    kp, kg = np.divmod(key, n_gt + 1)
    cnt = cnt.astype(np.int64)
    area_pred, area_gt = np.zeros(n_pred + 1, np.int64), np.zeros(n_gt + 1, np.int64)
    np.add.at(area_pred, kp, cnt); np.add.at(area_gt, kg, cnt)
    both = (kp > 0) & (kg > 0)                                       # np.unique sorts the keys: lexicographic in (pred id, gt id)
    return Contingency(area_pred[1:], area_gt[1:], np.stack([kp[both], kg[both]], 1), cnt[both])


# ---- device -----------------------------------------------------------------------------------------------------------------------------

def _stats_buffer(labels, n):
    """device int32 [5 n + 1]: the stats of kg_label_stats with its invalid count behind them (one buffer, so one copy brings both back)"""
    import torch
    from ._lib import ptr, stream_ptr
    lab = device_maps("label_stats", labels, False)
    n = _count("label_stats", n)
    buf = torch.empty(n * 5 + 1, dtype=torch.int32, device=lab.device)
    with torch.cuda.device(lab.device):
        _lib.call("kg_label_stats", ptr(lab), lab.shape[0], lab.shape[1], n, ptr(buf) if n else None, ptr(buf[n * 5:]), stream_ptr())
    return buf


def label_stats_device(labels, n):
    """labels: device int32 [H, W] -> (stats device int32 [n, 5], invalid device int32 [1]): kg_label_stats as it is, no copy, no check."""
    buf = _stats_buffer(labels, n)
    return buf[:-1].view(len(buf) // 5, 5), buf[-1:]


def label_stats(labels, n):
    """labels: device int32 [H, W] with ids 1 .. n -> host int64 [n, 5] (STATS_COLUMNS); one device -> host copy; raises when a pixel lies
    outside [0, n]."""
    both = _stats_buffer(labels, n).cpu().numpy().astype(np.int64)
    _raise_invalid("label_stats", int(both[-1]), int(n))
    return both[:-1].reshape(-1, 5)


def inter_jobs(a, b, jobs):
    """a, b: device int32 [H, W]; jobs: host int [m, 6] (uploaded once) or a device int32 tensor -> device int64 [m] (kg_label_inter_jobs)."""
    import torch
    from ._lib import ptr, stream_ptr
    a, b = device_maps("inter_jobs", a, False), device_maps("inter_jobs", b, False)
    if a.shape != b.shape or a.device != b.device:
        raise KGLibraryError(f"inter_jobs: maps of {tuple(a.shape)} and {tuple(b.shape)} must have one size and one device")
    dev = a.device
    jd = device_jobs("inter_jobs", jobs, 6, "(id_a, id_b, y1, x1, y2, x2)", dev)
    m = jd.shape[0]
    count = torch.empty(m, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.call("kg_label_inter_jobs", ptr(a), ptr(b), a.shape[0], a.shape[1], ptr(jd) if m else None, m, ptr(count) if m else None, stream_ptr())
    return count


def contingency(pred, gt, n_pred, n_gt, pred_stats=None, gt_stats=None, max_job_pixels=65536):
    """The Contingency of two device label maps (int32 [H, W], ids 1 .. n_pred / 1 .. n_gt).  pred_stats / gt_stats: host integers [n, 5]
    (STATS_COLUMNS) when the caller has them -- columns 1:6 of an Instances / TiledInstances table are the stats of its label map -- and
    then no stats launch is made for that side.  A box of more than max_job_pixels pixels is counted in bands (split_jobs).
    Device -> host copies: one for the counts, and one for each side whose stats were computed here."""
    pred, gt = device_maps("contingency", pred, False), device_maps("contingency", gt, False)
    n_pred, n_gt = _count("contingency", n_pred), _count("contingency", n_gt)
    if pred.shape != gt.shape or pred.device != gt.device:
        raise KGLibraryError(f"contingency: a predicted map of {tuple(pred.shape)} against a ground truth of {tuple(gt.shape)} (one size, one device)")
    sp = label_stats(pred, n_pred) if pred_stats is None else _stats("contingency", pred_stats, n_pred)
    sg = label_stats(gt, n_gt) if gt_stats is None else _stats("contingency", gt_stats, n_gt)
    jobs = candidate_pairs(sp, sg)
    pieces, owner = split_jobs(jobs, max_job_pixels)
    inter = np.zeros(len(jobs), np.int64)
    if len(pieces):
        np.add.at(inter, owner, inter_jobs(pred, gt, pieces).cpu().numpy())
    met = inter > 0
    return Contingency(sp[:, 0], sg[:, 0], jobs[met, :2], inter[met])


# ---- metrics: host float64 over a Contingency -------------------------------------------------------------------------------------------

def _present(c):
    return int(np.count_nonzero(c.area_pred)), int(np.count_nonzero(c.area_gt))


def match(c, conf, thresholds=evaluation.THRESHOLDS):
    """The reference's greedy matching (evaluation.match_thresholds) of the predicted ids, confidences conf [n_pred] in id order, against the
    GT ids at every threshold, with the pairs that meet in place of the box test: a pair that does not meet has IoU 0 and matches nothing."""
    conf = np.asarray(conf).reshape(-1)
    if len(conf) != len(c.area_pred):
        raise ValueError(f"match: {len(conf)} confidences for {len(c.area_pred)} predicted ids")
    keep = np.zeros((len(c.area_pred), len(c.area_gt)), bool)
    iou = np.zeros(keep.shape, np.float64)
    p, g = c.pairs[:, 0].astype(np.int64) - 1, c.pairs[:, 1].astype(np.int64) - 1
    keep[p, g] = True
    iou[p, g] = c.iou()
    return evaluation.match_thresholds(conf, keep, iou, thresholds)


def _at_least_half(fn, thresholds):
    t = np.asarray(thresholds, np.float64).reshape(-1)
    if len(t) == 0 or not np.all(t >= 0.5):
        raise ValueError(f"{fn}: every threshold must be >= 0.5 (above it an id is in at most one matching pair)")
    return t


def kaggle_score(c, thresholds=evaluation.THRESHOLDS):
    """The DSB-2018 image score: the mean over t of TP_t / (P + G - TP_t), TP_t = the pairs with iou > t (strict), P and G = the ids with
    non-zero area on each side; None for an image with neither."""
    t = _at_least_half("kaggle_score", thresholds)
    P, G = _present(c)
    if P + G == 0:
        return None
    tp = (c.iou()[None, :] > t[:, None]).sum(1).astype(np.float64)
    return float(np.mean(tp / (P + G - tp)))


def panoptic(c, thr=0.5):
    """{tp, fp, fn, sum_iou} of panoptic quality: tp = the pairs with iou > thr (strict), fp = P - tp, fn = G - tp."""
    thr = float(_at_least_half("panoptic", [thr])[0])
    P, G = _present(c)
    iou = c.iou()
    hit = iou > thr
    tp = int(hit.sum())
    return {"tp": tp, "fp": P - tp, "fn": G - tp, "sum_iou": float(iou[hit].sum())}


def aji(c):
    """(C, U) of the aggregated Jaccard index: every GT id g with non-zero area, ascending, takes the prediction j of largest IoU among
    those that meet it (a tie: the smallest id): C += I(j, g), U += A_g + A_j - I(j, g), j is used; a g nothing meets adds A_g to U; at
    the end every prediction that was never used adds its area to U."""
    j, g = c.pairs[:, 0].astype(np.int64) - 1, c.pairs[:, 1].astype(np.int64) - 1
    order = np.lexsort((j, -c.iou(), g))                              # by g; within a g the largest IoU first, a tie by ascending j
    best = order[np.flatnonzero(np.diff(g[order], prepend=-1))]       # the first pair of every g that meets anything
    used = np.zeros(len(c.area_pred), bool)
    used[j[best]] = True
    met = np.zeros(len(c.area_gt), bool)
    met[g[best]] = True
    C = int(c.inter[best].sum())
    U = int((c.area_gt[g[best]] + c.area_pred[j[best]] - c.inter[best]).sum()) + int(c.area_gt[~met].sum()) + int(c.area_pred[~used].sum())
    return C, U


def dice(c):
    """(2 * sum of the intersections, sum of the predicted areas + sum of the GT areas): foreground Dice is their quotient."""
    return 2 * int(c.inter.sum()), int(c.area_pred.sum()) + int(c.area_gt.sum())


# ---- accumulation over images -----------------------------------------------------------------------------------------------------------

def _is_map_pair(v):
    return isinstance(v, (tuple, list)) and len(v) == 2 and np.ndim(v[1]) == 0


class LabelEvaluator:
    """Accumulates the label-map metrics over images: add(pred, gt) per image, summary() at the end."""

    def __init__(self, thresholds=evaluation.THRESHOLDS, use_07_metric=False, boundary=None):
        """boundary: None (overlap metrics only), True, or dict(tolerance=2, sources='border', targets='border'): add() then also runs
        boundaries.pair_distances on the true-positive pairs of panoptic (IoU > 0.5), on whichever side the maps live, and summary() gains
        hd, hd95, assd, nsd (at the tolerance) and boundary_pairs."""
        self.thresholds = np.asarray(thresholds, np.float64).reshape(-1)
        self.boundary = self._boundary_options(boundary)
        self.distances = {"hd": [], "hd95": [], "assd": [], "nsd": []}   # one value per true-positive pair added
        self.use_07_metric = use_07_metric
        self.seg = evaluation._Stream(len(self.thresholds))
        self.scores = []                                             # kaggle image scores
        self.pq = {"tp": 0, "fp": 0, "fn": 0, "sum_iou": 0.0}
        self.aji = []
        self.dice = [0, 0]
        self.images = 0

    @staticmethod
    def _boundary_options(boundary):
        if boundary is None or boundary is False:
            return None
        opts = {"tolerance": 2, "sources": "border", "targets": "border"}
        if boundary is not True:
            if not isinstance(boundary, dict) or set(boundary) - set(opts):
                raise KGLibraryError(f"LabelEvaluator: boundary must be None, True or a dict with keys among {sorted(opts)}")
            opts.update(boundary)
        from . import boundaries
        boundaries.mode_of("LabelEvaluator", opts["sources"], opts["targets"])
        if not float(opts["tolerance"]) >= 0:
            raise KGLibraryError(f"LabelEvaluator: boundary tolerance {opts['tolerance']!r}")
        return opts

    def _add_boundary(self, plab, glab, c, pred_stats, gt_stats, on_device):
        """The boundary distances of the true-positive pairs of one image (panoptic's: IoU > 0.5), where the maps live"""
        from . import boundaries
        o = self.boundary
        route = boundaries.pair_distances if on_device else boundaries.pair_distances_host
        d = route(plab, glab, c.pairs[c.iou() > 0.5], pred_stats, gt_stats, sources=o["sources"], targets=o["targets"])
        for key, v in (("hd", d.hausdorff()), ("hd95", d.hd95()), ("assd", d.assd()), ("nsd", d.nsd(o["tolerance"]))):
            self.distances[key].extend(v.tolist())

    def add(self, pred, gt, conf=None):
        """pred: an Instances / TiledInstances (its label map, its table as the stats, its dets' confidences), or a (labels, n_pred) pair,
        for which conf [n_pred] is needed for the AP part (without it seg_ap / seg_iou do not see the image).
        gt: a (labels, n_gt) pair, host or device; a BitMasks; dense [ng, H, W] masks (NumPy or tensor); or a polygons.Polygons, which is
        filled at the prediction's size with the ids 1 .. m (polygons.fill on the prediction's device, fill_host for a host prediction: the
        first row wins a pixel, n_gt = m).  The two mask forms become a
        label map and its stats through instances.label_map(with_table=True): where GT masks overlap, the FIRST row wins the pixel, and a
        GT row wholly hidden that way has area 0 and is not counted in G.
        A device predicted map is scored on the device (contingency), a host one through contingency_host.  Returns the Contingency."""
        pred_stats = None
        if isinstance(pred, instances.Instances):
            plab, n_pred, pred_stats = pred.labels, len(pred), np.asarray(pred.table)[:, 1:6]
            if conf is None:
                conf = np.asarray(pred.dets)[:, 4]
        elif _is_map_pair(pred):
            plab, n_pred = pred[0], int(pred[1])
        else:
            raise KGLibraryError("LabelEvaluator.add: pred must be an Instances or a (labels, n_pred) pair")
        import torch
        on_device = is_device(plab)
        if torch.is_tensor(plab) and not on_device:
            plab = plab.numpy()
        shape = tuple(plab.shape)
        if isinstance(gt, polygons.Polygons):                         # filled at the prediction's size, where the prediction lives
            if len(shape) != 2:
                raise KGLibraryError(f"LabelEvaluator.add: a predicted map of {shape} against polygons")
            gt = (polygons.fill(gt, *shape, plab.device) if on_device else polygons.fill_host(gt, *shape), len(gt))
        if on_device:
            glab, n_gt, gt_stats = self._device_gt(gt, plab.device)
            if tuple(glab.shape) != shape:
                raise KGLibraryError(f"LabelEvaluator.add: a predicted map of {shape} against a ground truth of {tuple(glab.shape)}")
            if self.boundary is not None:                             # the boxes are needed twice: computed here, once
                pred_stats = label_stats(plab, n_pred) if pred_stats is None else pred_stats
                gt_stats = label_stats(glab, n_gt) if gt_stats is None else gt_stats
            c = contingency(plab, glab, n_pred, n_gt, pred_stats, gt_stats)
            if self.boundary is not None:
                self._add_boundary(plab, glab, c, pred_stats, gt_stats, True)
        else:
            glab, n_gt = self._host_gt(gt)
            if tuple(glab.shape) != shape:
                raise KGLibraryError(f"LabelEvaluator.add: a predicted map of {shape} against a ground truth of {tuple(glab.shape)}")
            c = contingency_host(plab, glab, n_pred, n_gt)
            if self.boundary is not None:
                self._add_boundary(plab, glab, c, label_stats_host(plab, n_pred), label_stats_host(glab, n_gt), False)
        self.add_contingency(c, conf)
        return c

    @staticmethod
    def _device_gt(gt, dev):
        import torch
        from . import ops
        if _is_map_pair(gt):
            lab, n = gt[0], int(gt[1])
            if not torch.is_tensor(lab):
                lab = ops.h2d(np.ascontiguousarray(host_maps("LabelEvaluator.add", lab, False).astype(np.int32)), dev)
            return lab.to(dev), n, None
        m = BitMasks.from_dense(gt, dev)                             # (a BitMasks passes through)
        if m.device != dev:
            m = BitMasks(m.words.to(dev), m.h, m.w)
        labels, table = instances.label_map(m, with_table=True)
        return labels[0], len(m), table.cpu().numpy()[:, 1:6]

    @staticmethod
    def _host_gt(gt):
        import torch
        if _is_map_pair(gt):
            lab = gt[0].cpu().numpy() if torch.is_tensor(gt[0]) else gt[0]
            return host_maps("LabelEvaluator.add", lab, False), int(gt[1])
        if isinstance(gt, BitMasks):
            dense = unpack_host(gt.words_cpu(), gt.h, gt.w)
        else:
            dense = gt.cpu().numpy() if torch.is_tensor(gt) else np.asarray(gt)
        return instances.label_map_host(dense), len(dense)

    def add_contingency(self, c, conf=None):
        """One image's Contingency (and the confidences of its predicted ids, for the AP part)."""
        if conf is not None:                                          # without confidences the AP part does not see the image
            m = match(c, conf, self.thresholds)
            self.seg.npos += _present(c)[1]
            self.seg.add(m)
        k = kaggle_score(c, self.thresholds) if np.all(self.thresholds >= 0.5) else None
        if k is not None:
            self.scores.append(k)
        for key, v in panoptic(c).items():
            self.pq[key] += v
        C, U = aji(c)
        if U:
            self.aji.append(C / U)
        num, den = dice(c)
        self.dice[0] += num; self.dice[1] += den
        self.images += 1

    def summary(self):
        """thresholds; seg_ap, seg_iou per threshold (as Evaluator.summary; npos is the number of GT ids with non-zero area); kaggle = the
        mean of the image scores; pq, sq, dq from the summed tp, fp, fn, sum_iou; aji = the mean over images of C / U (images with U == 0
        skipped); dice from the summed numerators and denominators; images.  A part nothing was added to is None.  With boundary= set:
        hd, hd95, assd, nsd = the means over all true-positive pairs added (math.fsum, so no order matters; inf when a pair has an
        unreachable side) and boundary_pairs, their number."""
        nt = len(self.thresholds)
        seg = self.seg.scores or self.seg.npos
        tp, fp, fn, s = self.pq["tp"], self.pq["fp"], self.pq["fn"], self.pq["sum_iou"]
        den = tp + 0.5 * fp + 0.5 * fn
        out = {"thresholds": self.thresholds,
               "seg_ap": np.array([self.seg.ap(t, self.use_07_metric) for t in range(nt)]) if seg else None,
               "seg_iou": np.array([np.mean(self.seg.overlaps[t]) for t in range(nt)]) if seg else None,
               "kaggle": float(np.mean(self.scores)) if self.scores else None,
               "pq": s / den if den else None, "sq": (s / tp if tp else 0.0) if den else None, "dq": tp / den if den else None,
               "aji": float(np.mean(self.aji)) if self.aji else None,
               "dice": self.dice[0] / self.dice[1] if self.dice[1] else None,
               "images": self.images}
        if self.boundary is not None:
            for key, v in self.distances.items():
                out[key] = math.fsum(v) / len(v) if v else None
            out["boundary_pairs"] = len(self.distances["hd"])
        return out


def evaluate_tiled(model, samples, tile=(512, 512), overlap=128, boundary=None, **predict_tiled_kwargs):
    """samples yields (image, gt): image as predict_tiled takes it (uint8 [H, W, 3]), gt as LabelEvaluator.add takes it, at the image's
    size.  Per sample: tiling.predict_tiled, then LabelEvaluator.add on its result.  boundary: LabelEvaluator's.  Returns
    LabelEvaluator.summary()."""
    from . import tiling
    ev = LabelEvaluator(boundary=boundary)
    for image, gt in samples:
        ev.add(tiling.predict_tiled(model, image, tile=tile, overlap=overlap, **predict_tiled_kwargs), gt)
    return ev.summary()
