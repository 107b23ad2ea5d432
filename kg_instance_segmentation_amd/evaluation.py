"""Single-pass dataset evaluation: AP and mean mask IoU of eval.py (:130-259) at every threshold from ONE pass over the data.

The reference runs `instance_segmentation_evaluation` once per threshold (run_seg_ap: ten passes of network, post-processing, seg branch
and mask paste, image by image).  Nothing but the final comparison `ovmax >= ov_thresh` depends on the threshold: the mask IoU of a
(detection, GT) pair, the GT instance a detection overlaps most, and the order of the detections do not.  So the masks are pasted once, as
bits (bitmasks.BitMasks), the IoU table of a whole batch is counted once on the device (one areas launch per side and one intersection
launch per output size, one copy back), and the greedy matching -- a few hundred numbers per image -- runs on the host at all thresholds.

    ev = Evaluator()
    for x, image_sizes, gt_masks, gt_boxes in batches: ...      # or simply: evaluate(model, batches)
    ev.summary() -> {"thresholds", "seg_ap", "seg_iou", "dec_ap"}   (arrays, one entry per threshold)"""
import numpy as np

from . import eval_parts

THRESHOLDS = np.linspace(0.5, 0.95, 10)        # eval.py:240


def box_keep(gt_boxes, det_boxes):
    """keep[d, g] = the box test of eval_parts.py:125-131 (`inters > 0`) of detection box d (y1, x1, y2, x2) against GT box g, evaluated
    in the reference's dtype promotion (the arrays are used as they come)."""
    gt, b = np.asarray(gt_boxes), np.asarray(det_boxes)
    if len(gt) == 0 or len(b) == 0:
        return np.zeros((len(b), len(gt)), bool)
    gt, b = gt[None, :, :4], b[:, None, :4]
    iymin = np.maximum(gt[..., 0], b[..., 0]); ixmin = np.maximum(gt[..., 1], b[..., 1])
    iymax = np.minimum(gt[..., 2], b[..., 2]); ixmax = np.minimum(gt[..., 3], b[..., 3])
    return np.maximum(ixmax - ixmin, 0.) * np.maximum(iymax - iymin, 0.) > 0.


def _greedy(ovmax, jmax, ng, thresholds, with_overlaps):
    """The threshold-dependent part of the greedy matching: detections in confidence order, a GT instance is taken once."""
    nd = len(ovmax)
    res = []
    for thr in thresholds:
        tp = np.zeros(nd); fp = np.zeros(nd)
        taken = [False] * ng
        ovl = []
        for d in range(nd):
            if ovmax[d] >= thr and not taken[jmax[d]]:
                tp[d] = 1.; taken[jmax[d]] = True; ovl.append(ovmax[d])
            else:
                fp[d] = 1.
        r = {"fp": fp, "tp": tp}
        if with_overlaps:
            r["overlaps"] = ovl
        res.append(r)
    return res


def match_thresholds(conf, keep, iou, thresholds):
    """seg_evaluation's matching (eval_parts.py:98-150) at every threshold from one IoU table.
    conf [nd]: confidences in the detections' own order; keep [nd, ng] bool: the box test; iou [nd, ng]: mask IoUs (read where keep).
    Returns {"scores": confidences sorted as np.argsort(-conf), "order": that permutation, "per_threshold": [{"fp", "tp", "overlaps"}]}."""
    conf = np.asarray(conf)
    order = np.argsort(-conf)
    keep = np.asarray(keep, bool)[order]
    if keep.ndim != 2:
        raise ValueError("match_thresholds: keep must be [nd, ng]")
    iou = np.asarray(iou, np.float64).reshape(keep.shape)[order]
    nd, ng = keep.shape
    ovmax = [-np.inf] * nd; jmax = [-1] * nd
    for d in range(nd):                          # the first GT of the largest IoU among the kept ones (strict >, ascending j)
        for j in np.nonzero(keep[d])[0]:
            if iou[d, j] > ovmax[d]:
                ovmax[d], jmax[d] = float(iou[d, j]), int(j)
    return {"scores": conf[order], "order": order, "per_threshold": _greedy(ovmax, jmax, ng, thresholds, True)}


def match_thresholds_boxes(dets, gt_boxes, thresholds):
    """bbox_evaluation's matching (eval_parts.py:45-93) at every threshold: dets [nd, 5] (y1, x1, y2, x2, conf), box IoU against every GT
    box in float64.  Returns {"scores", "order", "per_threshold": [{"fp", "tp"}]}."""
    dets = np.asarray(dets)
    order = np.argsort(-dets[:, 4])
    boxes = dets[order, :4]
    gt = np.asarray(gt_boxes).astype(float)
    nd = len(boxes)
    ovmax = [-np.inf] * nd; jmax = [-1] * nd
    for d in range(nd):
        bb = boxes[d, :].astype(float)
        if gt.shape[0] > 0:
            inters = eval_parts._box_inter(gt, bb)
            union = (bb[2] - bb[0]) * (bb[3] - bb[1]) + (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1]) - inters
            ov = inters / union
            ovmax[d] = np.max(ov); jmax[d] = int(np.argmax(ov))
    return {"scores": dets[order, 4], "order": order, "per_threshold": _greedy(ovmax, jmax, gt.shape[0], thresholds, False)}


class _Stream:
    """all_fp / all_tp / all_scores / npos of eval.py:138-162 for every threshold at once (the scores do not depend on it)."""

    def __init__(self, nthr):
        self.fp = [[] for _ in range(nthr)]
        self.tp = [[] for _ in range(nthr)]
        self.overlaps = [[] for _ in range(nthr)]
        self.scores = []
        self.npos = 0

    def add(self, m):
        self.scores.extend(m["scores"])
        for t, r in enumerate(m["per_threshold"]):
            self.fp[t].extend(r["fp"]); self.tp[t].extend(r["tp"])
            self.overlaps[t].extend(r.get("overlaps", ()))

    def ap(self, t, use_07_metric):
        """eval.py:163-176 / :219-232 as written."""
        all_fp = np.asarray(self.fp[t]); all_tp = np.asarray(self.tp[t]); all_scores = np.asarray(self.scores)
        sorted_ind = np.argsort(-all_scores)
        all_fp = np.cumsum(all_fp[sorted_ind]); all_tp = np.cumsum(all_tp[sorted_ind])
        rec = all_tp / float(self.npos)
        prec = all_tp / np.maximum(all_tp + all_fp, np.finfo(np.float64).eps)
        return eval_parts.voc_ap(rec, prec, use_07_metric=use_07_metric)


class Evaluator:
    """Accumulates the segmentation (add_batch) and detection (add_boxes) evaluation of eval.py at all `thresholds` in one pass."""

    def __init__(self, thresholds=THRESHOLDS, use_07_metric=False):
        self.thresholds = np.asarray(thresholds, np.float64).reshape(-1)
        self.use_07_metric = use_07_metric
        self.seg = _Stream(len(self.thresholds))
        self.dec = _Stream(len(self.thresholds))

    # ---- segmentation: eval.py:143-162 for the images of a batch -----------------------------------------------------------------------
    def add_batch(self, preds, gt_masks, gt_boxes, iou_tables=None):
        """preds: predict()'s list, entry None or [masks, dets] with the masks packed (BitMasks), dense device bytes or dense NumPy;
        gt_masks: per image [ng, h, w] NumPy / tensor / BitMasks; gt_boxes: per image [ng, 4] (y1, x1, y2, x2).
        iou_tables: per image a precomputed [nd, ng] mask IoU table in the detections' own order (None entries for images without
        prediction); the masks are then not read and no GPU is needed."""
        n = len(preds)
        if len(gt_masks) != n or len(gt_boxes) != n:
            raise ValueError("add_batch: one ground-truth entry per prediction")
        keeps = [None if p is None else box_keep(gt_boxes[i], np.asarray(p[1])[:, :4]) for i, p in enumerate(preds)]
        if iou_tables is None:
            iou_tables = self._iou_tables(preds, gt_masks, keeps)
        for i, p in enumerate(preds):
            if p is None:                                  # eval.py:147-149
                self.seg.npos += len(gt_boxes[i])
                continue
            self.seg.npos += len(gt_masks[i]) if gt_masks[i] is not None else len(gt_boxes[i])
            self.seg.add(match_thresholds(np.asarray(p[1])[:, 4], keeps[i], iou_tables[i], self.thresholds))

    @staticmethod
    def _iou_tables(preds, gt_masks, keeps):
        """The mask IoU tables of a batch: per output size one kg_bitmask_areas launch over the detection masks of all its images, one over
        their GT masks, one kg_bitmask_inter_pairs launch over all box-overlapping pairs; ONE device-to-host copy for the whole batch."""
        import torch
        from .bitmasks import BitMasks, pack_host
        tables = [None if k is None else np.zeros(k.shape, np.float64) for k in keeps]
        groups = {}
        dev = None
        for i, k in enumerate(keeps):
            if k is None or not k.any():
                continue
            m = preds[i][0]
            if dev is None:
                dev = m.device if isinstance(m, BitMasks) or torch.is_tensor(m) else torch.device("cuda", torch.cuda.current_device())
            groups.setdefault(tuple(int(v) for v in m.shape[1:]), []).append(i)
        jobs, counts = [], []
        for (h, w), imgs in groups.items():
            det = BitMasks.cat([BitMasks.from_dense(preds[i][0], dev) for i in imgs])
            gts, host = [], []
            for i in imgs:                                 # NumPy GT is packed on the host: the words of a size group go up in one copy
                g = gt_masks[i]
                if isinstance(g, BitMasks) or torch.is_tensor(g):
                    if host:
                        gts.append(BitMasks.from_words(np.concatenate(host), h, w, dev)); host = []
                    gts.append(BitMasks.from_dense(g, dev))
                else:
                    g = np.asarray(g)
                    if g.shape[1:] != (h, w):
                        raise ValueError(f"add_batch: image {i}: GT masks {g.shape[1:]} against predicted masks {(h, w)}")
                    host.append(pack_host(g))
            if host:
                gts.append(BitMasks.from_words(np.concatenate(host), h, w, dev))
            gt = BitMasks.cat(gts)
            pairs, d0, g0 = [], 0, 0
            for i in imgs:
                pr = np.argwhere(keeps[i])
                pairs.append(pr + [d0, g0])
                d0 += keeps[i].shape[0]; g0 += keeps[i].shape[1]
            if d0 != len(det) or g0 != len(gt):
                raise ValueError("add_batch: masks and boxes disagree in number")
            pairs = np.concatenate(pairs).astype(np.int32)
            aa, ab, inter = eval_parts.bit_counts(det, gt, pairs)
            jobs.append((imgs, pairs, len(det), len(gt)))
            counts += [aa, ab, inter]
        if not jobs:
            return tables
        c = torch.cat(counts).cpu().numpy()               # the one copy
        o = 0
        for imgs, pairs, na, nb in jobs:
            aa, ab, ia = c[o:o + na], c[o + na:o + na + nb], c[o + na + nb:o + na + nb + len(pairs)]
            o += na + nb + len(pairs)
            iou = eval_parts.iou_from_counts(aa, ab, ia, pairs)
            d0, g0, q = 0, 0, 0
            for i in imgs:
                k = int(keeps[i].sum())
                pr = pairs[q:q + k]
                tables[i][pr[:, 0] - d0, pr[:, 1] - g0] = iou[q:q + k]
                q += k; d0 += keeps[i].shape[0]; g0 += keeps[i].shape[1]
        return tables

    # ---- detection: eval.py:198-218 for one image --------------------------------------------------------------------------------------
    def add_boxes(self, dets, gt_boxes, image_size, input_size):
        """dets: the image's boxes after NMS in network-input pixels ([n, 5], detect / detect_batch's entry) or None;
        image_size = (height, width) of the source image, input_size = (input_h, input_w)."""
        if dets is None:
            self.dec.npos += len(gt_boxes)
            return
        (height, width), (input_h, input_w) = image_size, input_size
        b = np.array(dets, np.float32)
        b[:, 0] = b[:, 0] / int(input_h) * int(height)
        b[:, 1] = b[:, 1] / int(input_w) * int(width)
        b[:, 2] = b[:, 2] / int(input_h) * int(height)
        b[:, 3] = b[:, 3] / int(input_w) * int(width)
        self.dec.npos += np.asarray(gt_boxes).shape[0]
        self.dec.add(match_thresholds_boxes(b, gt_boxes, self.thresholds))

    def summary(self):
        """Per threshold: seg_ap and seg_iou (mean overlap of the true positives) as eval.py:163-179, dec_ap as eval.py:219-234; a part
        nothing was added to is None."""
        nt = len(self.thresholds)
        seg = self.seg.scores or self.seg.npos
        dec = self.dec.scores or self.dec.npos
        return {"thresholds": self.thresholds,
                "seg_ap": np.array([self.seg.ap(t, self.use_07_metric) for t in range(nt)]) if seg else None,
                "seg_iou": np.array([np.mean(self.seg.overlaps[t]) for t in range(nt)]) if seg else None,
                "dec_ap": np.array([self.dec.ap(t, self.use_07_metric) for t in range(nt)]) if dec else None}


def evaluate(model, batches, nms_thresh=0.5, seg_thresh=0.5, thresholds=THRESHOLDS, use_07_metric=False, max_workspace_bytes=None):
    """eval.py's run_seg_ap + run_dec_ap in one pass.  batches yields (x, image_sizes, gt_masks, gt_boxes): x [N,3,H,W] resized and
    normalised as predict() takes it, image_sizes the (h, w) of the source images (None: the input size), gt_masks / gt_boxes per image at
    the source image's size.  Per batch: forward_dec, detect_batch, predict(packed=True) on those detections, Evaluator.add_batch and
    add_boxes.  Returns Evaluator.summary()."""
    import torch
    from . import inference, postprocessing
    ev = Evaluator(thresholds, use_07_metric)
    for x, image_sizes, gt_masks, gt_boxes in batches:
        with torch.no_grad():
            d0, d1, d2, d3, feat_seg = model.forward_dec(x)
        dec = [d0, d1, d2, d3]
        H, W = int(x.shape[2]), int(x.shape[3])
        sizes = [(H, W)] * x.shape[0] if image_sizes is None else [(int(h), int(w)) for h, w in image_sizes]
        dets = postprocessing.detect_batch(dec, nms_thresh, max_workspace_bytes=max_workspace_bytes)
        preds = inference.predict_from_heads(model, dec, feat_seg, H, W, nms_thresh, seg_thresh, sizes, False, max_workspace_bytes, packed=True,
                                             dets=dets)
        ev.add_batch(preds, gt_masks, gt_boxes)
        for i, d in enumerate(dets):
            ev.add_boxes(d, gt_boxes[i], sizes[i], (H, W))
    return ev.summary()
