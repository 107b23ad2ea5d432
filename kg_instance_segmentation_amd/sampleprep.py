"""Training samples prepared on the device: augmentation, boxes and targets of a whole batch (csrc/sampleprep.hip).

`prepare_batch` produces what `BaseDataset.__getitem__` (dataset_base.py:81-116) plus `collater` (collater.py:4-25) produce under
train.py:77-85's two transform pipelines
    train: ConvertImgFloat -> PhotometricDistort -> Expand(max_scale 2, mean 0) -> RandomMirror_w -> RandomMirror_h -> Resize
    val:   ConvertImgFloat -> Resize
from decoded uint8 images and their instance masks, without any full-size array leaving the GPU: one launch resizes the images
(kg_sp_image), one warps every instance mask of the batch and accumulates its boxes at the four divide scales (kg_sp_warp_masks), one
builds the ordered keypoint / box lists (kg_sp_boxes), and the existing kg_gt_maps fills the stacked target tensors.  All results are
bit-identical to the reference's semantics; the interpolation rules are the ones oracle/paste.py pins (OpenCV itself is not available to
this repository).

The random parameters are drawn on the host by `draw_train_params`, in the reference's call order, so that a seeded `np.random` gives
the reference's own augmentation.

Deviations from the reference, both on inputs it cannot process: an image with zero instances gives empty lists and all-zero targets
(the reference raises IndexError at `masks[0]`, dataset_base.py:60); source masks are taken as foreground where non-zero (the reference
compares the float mask with 1., dataset_base.py:47,66: identical for 0 / 1 masks).

Ground truth may also be a label map (`LabelSource`: what runlengths.paint, polygons.fill and predict_instances produce): the masks
launch is then kg_sp_warp_labels, which reads `labels == id` inside each id's box, and nothing goes through the host.  `warp_labels`
is the warped map itself (kg_sp_warp_labelmap); `label_masks_host` / `warp_labels_host` state both in NumPy.

Opt-in, like batched inference: the reference drivers and `dropin/` do not use it (INTEGRATION.md shows the loop change)."""
from dataclasses import dataclass
from typing import NamedTuple, Tuple

import numpy as np
import torch

from . import _lib, config as cfg, ops, preprocessing
from ._lib import ptr, stream_ptr
from .bitmasks import BitMasks

# transforms.py:58-60
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
DIVIDE_SCALES = (1, 2, 4, 8)            # dataset_base.py:89-92
MAX_WIDTH = 4096                        # SP_MAXW of csrc/sampleprep.hip

_MIRROR_W, _MIRROR_H, _BITS, _LABELS = 1, 2, 4, 8
# struct SpImage of csrc/sampleprep.hip (80 bytes)
_REC = np.dtype([("img", "<u8"), ("masks", "<u8"), ("h", "<i4"), ("w", "<i4"), ("He", "<i4"), ("We", "<i4"), ("oy", "<i4"), ("ox", "<i4"),
                 ("flags", "<i4"), ("perm", "<i4"), ("delta", "<f4"), ("alpha", "<f4"), ("inst0", "<i4"), ("n", "<i4"), ("ld", "<i8"),
                 ("pad", "<i8")])
assert _REC.itemsize == 80


@dataclass(frozen=True)
class SampleParams:
    """The augmentation of one sample.  `delta` / `alpha` / `perm` / `canvas` / `offset` matter only when their switch is on."""
    brightness: bool = False
    delta: float = 0.0                      # transforms.py:44
    contrast: bool = False
    alpha: float = 1.0                      # transforms.py:31
    swap: bool = False
    perm: Tuple[int, int, int] = (0, 1, 2)  # transforms.py:63
    expand: bool = False
    canvas: Tuple[int, int] = (0, 0)        # (He, We) = (int(h r), int(w r)), transforms.py:99
    offset: Tuple[int, int] = (0, 0)        # (int(y1), int(x1)), transforms.py:101
    mirror_w: bool = False
    mirror_h: bool = False

    def switches(self):
        return (self.brightness, self.contrast, self.swap, self.expand, self.mirror_w, self.mirror_h)

    def resolved(self, h, w):
        """(delta, alpha, perm, He, We, oy, ox) as the kernels take them for an h x w source; raises ValueError on a record that the
        reference's Expand could not have produced (a paste window that does not fit its canvas, transforms.py:101)."""
        h, w = int(h), int(w)
        perm = tuple(int(c) for c in self.perm) if self.swap else (0, 1, 2)
        if sorted(perm) != [0, 1, 2]:
            raise ValueError(f"sampleprep: perm {self.perm} is not a permutation of the three channels")
        He, We, oy, ox = h, w, 0, 0
        if self.expand:
            (He, We), (oy, ox) = (int(v) for v in self.canvas), (int(v) for v in self.offset)
            if oy < 0 or ox < 0 or oy + h > He or ox + w > We:
                raise ValueError(f"sampleprep: the {h} x {w} window at ({oy}, {ox}) does not fit the {He} x {We} canvas")
        delta = float(self.delta) if self.brightness else 0.0
        alpha = float(self.alpha) if self.contrast else 1.0
        if not (np.isfinite(delta) and np.isfinite(alpha)):
            raise ValueError("sampleprep: delta and alpha must be finite")
        return delta, alpha, perm, He, We, oy, ox


def identity_params():
    """The `val` pipeline (train.py:84-85): no augmentation, only the resize."""
    return SampleParams()


def draw_train_params(h, w, rng=np.random):
    """Draws the `train` pipeline's parameters for an h x w image, consuming `rng` (np.random or a RandomState) in the reference's
    exact call order, so that after np.random.seed(s) it draws what transforms.Compose would."""
    h, w = int(h), int(w)
    brightness = bool(rng.randint(2))                                    # transforms.py:43
    delta = float(rng.uniform(-32, 32)) if brightness else 0.0           # :44 (RandomBrightness(delta=32))
    rng.randint(2)                                                       # :77, both branches pick RandomContrast
    contrast = bool(rng.randint(2))                                      # :30
    alpha = float(rng.uniform(0.5, 1.5)) if contrast else 1.0            # :31
    swap = bool(rng.randint(2))                                          # :62
    perm = PERMS[rng.randint(len(PERMS))] if swap else (0, 1, 2)         # :63
    expand = not rng.randint(2)                                          # :92, expands on a 0
    canvas, offset = (0, 0), (0, 0)
    if expand:
        ratio = rng.uniform(1, 2)                                        # :95
        y1 = rng.uniform(0, h * ratio - h)                               # :96
        x1 = rng.uniform(0, w * ratio - w)                               # :97
        canvas, offset = (int(h * ratio), int(w * ratio)), (int(y1), int(x1))
        if int(y1 + h) - int(y1) != h or int(x1 + w) - int(x1) != w:     # (:101 would fail to broadcast)
            raise ValueError("sampleprep: the drawn paste window does not have the image's size")
    mirror_w = bool(rng.randint(2))                                      # :151
    mirror_h = bool(rng.randint(2))                                      # :159
    p = SampleParams(brightness, delta, contrast, alpha, swap, perm, expand, canvas, offset, mirror_w, mirror_h)
    p.resolved(h, w)
    return p


class PreparedBatch(NamedTuple):
    """Everything prepare_batch_full leaves on the device (+ the two small host tables)."""
    img: torch.Tensor           # [N,3,H,W] float32
    gt: tuple                   # gt_c0..gt_c3: [N,55,H/s,W/s] float32
    instance_masks: list        # per image [m,H,W] uint8 of 0 / 1, the masks load_gt_masks_bboxes keeps
    gt_bboxes: list             # per image HOST float32 [m,5] = (y1,x1,y2,x2,1)
    warped: list                # per image [n,H,W] uint8: every instance after the transform
    keypoints: list             # per image, per scale: device float32 [n_l,5,2] (bboxes_c0..c3 of dataset_base.py:89-92)
    counts: np.ndarray          # host int32 [N,5]: n_l of the four scales, m


def _device(device):
    try:
        from torch.utils.data import get_worker_info
        in_worker = get_worker_info() is not None
    except Exception:
        in_worker = False
    if in_worker:
        raise _lib.KGLibraryError("sampleprep.prepare_batch (MI355X build) was called inside a DataLoader worker process; workers cannot "
                                  "use the GPU: call it from the training loop on the decoded samples the workers return, or build the "
                                  "DataLoader with num_workers=0")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise _lib.KGLibraryError("sampleprep (MI355X build) needs a GPU device")
    return dev


def _image_on(img, dev):
    if torch.is_tensor(img):
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
            raise ValueError("sampleprep: images must be uint8 [h, w, 3]")
        return img.to(dev).contiguous()
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("sampleprep: images must be uint8 [h, w, 3]")
    return ops.h2d(a, dev)


def _masks_on(m, h, w, dev):
    """-> (holder, pointer, is_bits, n, ld): device bytes [n,h,w] or BitMasks words."""
    if isinstance(m, BitMasks):
        if m.device != dev:
            m = BitMasks(m.words.to(dev), m.h, m.w)
    elif torch.is_tensor(m):
        if m.dim() != 3:
            raise ValueError("sampleprep: masks must be [n, h, w]")
        if m.dtype == torch.uint8:
            t = m.to(dev).contiguous()
            if tuple(t.shape[1:]) != (h, w):
                raise ValueError(f"sampleprep: masks {tuple(t.shape[1:])} do not have the image's size {(h, w)}")
            return t, t.data_ptr(), False, t.shape[0], h * w
        m = BitMasks.from_dense(m, dev)                      # float32 (kg_mask_pack_bits) and other dtypes
    else:
        a = np.asarray(m)
        if a.ndim != 3:
            a = a.reshape(0, h, w) if a.size == 0 else a
        if a.ndim != 3:
            raise ValueError("sampleprep: masks must be [n, h, w]")
        m = BitMasks.from_dense(a, dev)                      # packed on the host: only the bits are uploaded
    if (m.h, m.w) != (h, w):
        raise ValueError(f"sampleprep: masks {(m.h, m.w)} do not have the image's size {(h, w)}")
    wd = m.words.contiguous()
    return wd, wd.data_ptr(), True, wd.shape[0], wd.shape[1]


class LabelSource:
    """The ground truth of one image as a label map instead of one mask per instance: what runlengths.paint, polygons.fill and
    predict_instances produce.  prepare_batch takes it wherever it takes masks (a batch is all label sources or all mask sources).
    labels: an int32 [h, w] device tensor, or a host integer array.  A host array is uploaded once, on first use, and the source keeps
    that device copy: the array must not change afterwards (a later change is NOT seen by later batches); build a new LabelSource for a
    changed map.  (A device tensor is read as it is at every batch.)  Give n or jobs, not both:
      n     the instances are the ids 1 .. n, in that order.  Their boxes come from stats, [n, 5] = labelmetrics.STATS_COLUMNS as a host
            array or as the device tensor of labelmetrics.label_stats_device; without stats they come from label_stats_device, on the
            device.  Neither adds a device -> host copy.  A pixel value outside [0, n] belongs to no instance.
      jobs  integers [m, 5] = (id, y1, x1, y2, x2): arbitrary ids in a chosen order, each with the half-open box that holds its pixels
            (a smaller box cuts the instance to the box).
    An id with no pixel keeps its row, as an all-zero mask, exactly like an all-zero plane among masks."""
    __slots__ = ("labels", "n", "stats", "jobs", "_on")

    def __init__(self, labels, n=None, stats=None, jobs=None):
        if torch.is_tensor(labels) and labels.device.type == "cuda":
            if labels.dtype != torch.int32 or labels.dim() != 2 or labels.numel() == 0:
                raise ValueError("sampleprep.LabelSource: a device label map must be a non-empty int32 [h, w] tensor")
        else:
            a = labels.numpy() if torch.is_tensor(labels) else np.asarray(labels)
            if a.ndim != 2 or a.dtype.kind not in "iu" or a.size == 0 or a.min() < -2 ** 31 or a.max() > 2 ** 31 - 1:
                raise ValueError("sampleprep.LabelSource: a host label map must be a non-empty integer array [h, w] that fits int32")
            labels = np.ascontiguousarray(a, np.int32)
        if (n is None) == (jobs is None):
            raise ValueError("sampleprep.LabelSource: give the instance count n or a job table, not both and not neither")
        if jobs is not None:
            if stats is not None:
                raise ValueError("sampleprep.LabelSource: stats belong to n; a job table carries its own boxes")
            j = np.asarray(jobs)
            if j.ndim != 2 or j.shape[1] != 5 or j.dtype.kind not in "iu" or (j.size and (j.min() < -2 ** 31 or j.max() > 2 ** 31 - 1)):
                raise ValueError("sampleprep.LabelSource: jobs must be integers [m, 5] = (id, y1, x1, y2, x2) that fit int32")
            jobs = np.ascontiguousarray(j, np.int32)
        else:
            if isinstance(n, (bool, np.bool_)) or int(n) != n or not 0 <= int(n) < 2 ** 31 // 5:
                raise ValueError(f"sampleprep.LabelSource: instance count {n!r}")
            n = int(n)
            if torch.is_tensor(stats):
                if stats.dtype != torch.int32 or tuple(stats.shape) != (n, 5):
                    raise ValueError(f"sampleprep.LabelSource: a stats tensor must be int32 [{n}, 5] = (area, y1, x1, y2, x2)")
                if stats.device.type != "cuda":
                    stats = stats.numpy()
            elif stats is not None:
                stats = np.asarray(stats)
                if stats.shape != (n, 5) or stats.dtype.kind not in "iu" or (stats.size and (stats.min() < -2 ** 31 or stats.max() > 2 ** 31 - 1)):
                    raise ValueError(f"sampleprep.LabelSource: stats must be integers [{n}, 5] = (area, y1, x1, y2, x2) that fit int32")
        self.labels, self.n, self.stats, self.jobs, self._on = labels, n, stats, jobs, None

    @staticmethod
    def from_instances(inst):
        """The label map and the table boxes of an Instances / TiledInstances (predict_instances, predict_tiled): the pseudo-label route.
        An instance with no visible pixel gets an empty box, hence an all-zero mask."""
        from . import _labelmaps
        try:
            stats = _labelmaps.instance_stats("sampleprep.LabelSource.from_instances", inst)
        except _lib.KGLibraryError as e:
            raise ValueError(str(e)) from None
        return LabelSource(inst.labels, n=len(stats), stats=stats)

    @property
    def shape(self):
        return tuple(int(v) for v in self.labels.shape)

    def __len__(self):
        return self.n if self.jobs is None else len(self.jobs)

    def on(self, dev):
        """the label map as a contiguous device int32 [h, w] on dev (a host map is uploaded once and kept)"""
        if self._on is None or self._on.device != dev:
            self._on = self.labels.to(dev).contiguous() if torch.is_tensor(self.labels) else ops.h2d(self.labels, dev)
        return self._on

    def job_rows(self, img, lab):
        """The rows (img, id, y1, x1, y2, x2) of this source as image `img` of a batch, in two halves: (host int32 [m, 2] = (img, id),
        host int32 [m, 4] boxes, None) or, when the boxes are device stats, (the same, None, device int32 [m, 4]); lab = on(dev)."""
        from . import _labelmaps
        if self.jobs is not None:
            return np.concatenate([np.full((len(self.jobs), 1), img, np.int32), self.jobs[:, :1]], 1), self.jobs[:, 1:], None
        stats = self.stats
        if self.n and stats is None:
            from . import labelmetrics
            stats = labelmetrics.label_stats_device(lab, self.n)[0]          # no copy back: an id without pixels has an empty box there
        if torch.is_tensor(stats) and self.n:
            if stats.device != lab.device:
                raise ValueError("sampleprep.LabelSource: the stats tensor must be on the batch's device")
            head = np.stack([np.full(self.n, img, np.int32), np.arange(1, self.n + 1, dtype=np.int32)], 1)
            return head, None, stats[:, 1:5]
        rows = _labelmaps.jobs_from_stats(stats, img) if self.n else np.zeros((0, 6), np.int32)
        return rows[:, :2], rows[:, 2:], None


def _label_route(masks):
    """True when every entry is a LabelSource, False when none is; a mixed batch is refused."""
    k = sum(isinstance(m, LabelSource) for m in masks)
    if k not in (0, len(masks)):
        raise ValueError("sampleprep: a batch is either all label sources (LabelSource) or all mask sources, not a mix of the two")
    return k > 0


def _jobs_upload(rows):
    """rows: LabelSource.job_rows of every image.  -> flat int32: what of the batch's job table travels with the image table.  With all
    boxes known on the host that is the table itself, [ntot, 6]; when some are device stats it is the (img, id) columns [ntot, 2], then
    the host boxes [., 4] in image order."""
    heads = np.concatenate([hd for hd, _, _ in rows]).reshape(-1, 2)
    if any(d is not None for _, _, d in rows):
        return np.concatenate([heads.reshape(-1)] + [b.reshape(-1) for _, b, _ in rows if b is not None]).astype(np.int32)
    return np.concatenate([heads, np.concatenate([b for _, b, _ in rows]).reshape(-1, 4)], 1).astype(np.int32).reshape(-1)


def _jobs_device(rows, up, ntot):
    """up: _jobs_upload(rows) on the device.  -> the batch's job table, device int32 [ntot, 6]: `up` itself, or -- with device stats --
    its (img, id) columns beside the boxes of every image in order, joined by a device concatenation."""
    if all(d is None for _, _, d in rows):
        return up.view(ntot, 6)
    at, boxes = 2 * ntot, []
    for _, b, d in rows:
        boxes.append(d if b is None else up[at:at + b.size].view(-1, 4))
        at += 0 if b is None else b.size
    return torch.cat([up[:2 * ntot].view(ntot, 2), torch.cat(boxes)], 1)


def prepare_batch_full(images, masks, params, input_h, input_w, device=None):
    """prepare_batch with everything it computed (PreparedBatch)."""
    from_labels = _label_route(masks)                        # (before the device is touched: a mixed batch is refused anywhere)
    dev = _device(device)
    H, W = int(input_h), int(input_w)
    N = len(images)
    if N == 0 or len(masks) != N or len(params) != N:
        raise ValueError("sampleprep: images, masks and params must be non-empty lists of one length")
    if H <= 0 or W <= 0 or H % 8 or W % 8 or W > MAX_WIDTH:
        raise ValueError(f"sampleprep: the network input {H} x {W} must be multiples of 8 (KGnet's pyramid), at most {MAX_WIDTH} wide")
    rec = np.zeros(N, _REC)
    holders, ntot = [], 0
    resolved = []
    for i in range(N):                                       # validate every record before anything is uploaded
        shp = tuple(images[i].shape)
        if len(shp) != 3:
            raise ValueError("sampleprep: images must be uint8 [h, w, 3]")
        resolved.append(params[i].resolved(shp[0], shp[1]))
        if from_labels and masks[i].shape != tuple(int(v) for v in shp[:2]):
            raise ValueError(f"sampleprep: a label map of {masks[i].shape} does not have the image's size {tuple(shp[:2])}")
    with torch.cuda.device(dev):
        rows = []                                            # label sources: LabelSource.job_rows of every image
        for i in range(N):
            img = _image_on(images[i], dev)
            h, w = int(img.shape[0]), int(img.shape[1])
            if from_labels:
                mh = masks[i].on(dev)
                rows.append(masks[i].job_rows(i, mh))
                mptr, bits, n, ld = mh.data_ptr(), False, len(masks[i]), 0
            else:
                mh, mptr, bits, n, ld = _masks_on(masks[i], h, w, dev)
            holders += [img, mh]
            delta, alpha, perm, He, We, oy, ox = resolved[i]
            flags = (_MIRROR_W if params[i].mirror_w else 0) | (_MIRROR_H if params[i].mirror_h else 0) | (_BITS if bits else 0) | \
                (_LABELS if from_labels else 0)
            rec[i] = (img.data_ptr(), mptr if n or from_labels else 0, h, w, He, We, oy, ox, flags, perm[0] | perm[1] << 2 | perm[2] << 4,
                      np.float32(delta), np.float32(alpha), ntot, n, ld, 0)
            ntot += n
        if from_labels:
            # one upload: the image table, then what the host knows of the job table
            tab = np.concatenate([rec.view(np.uint8), _jobs_upload(rows).view(np.uint8)])
        else:
            # one upload: the image table, then the image of every instance
            inst_img = np.repeat(np.arange(N, dtype=np.int32), rec["n"])
            tab = np.concatenate([rec.view(np.uint8), inst_img.view(np.uint8)])
        tab_d = ops.h2d(tab, dev)
        rec_p = _lib.c_void_p(tab_d.data_ptr())
        inst_p = _lib.c_void_p(tab_d.data_ptr() + rec.nbytes)
        if from_labels:
            jobs_d = _jobs_device(rows, tab_d[rec.nbytes:].view(torch.int32), ntot)
            holders.append(jobs_d)
            inst_p = ptr(jobs_d)
        s = stream_ptr()
        img_out = torch.empty(N, 3, H, W, dtype=torch.float32, device=dev)
        _lib.call("kg_sp_image", rec_p, N, H, W, ptr(img_out), s)
        warped = torch.empty(ntot, H, W, dtype=torch.uint8, device=dev)
        # 4-byte cells: counts [N,5] | gtb [ntot,5] (the part the host reads) | keep [ntot] | kp [4,ntot,5,2] | box [ntot,16]
        n_host = N * 5 + ntot * 5
        cells = torch.zeros(n_host + ntot + 40 * ntot + 16 * ntot, dtype=torch.int32, device=dev)
        counts_d, gtb_d = cells[:N * 5], cells[N * 5:n_host].view(torch.float32)
        keep_d = cells[n_host:n_host + ntot]
        kp_d = cells[n_host + ntot:n_host + 41 * ntot].view(torch.float32).view(4, ntot, 5, 2)
        box_d = cells[n_host + 41 * ntot:]
        if from_labels:
            _lib.call("kg_sp_warp_labels", rec_p, N, inst_p if ntot else None, ntot, H, W, ptr(warped) if ntot else None,
                      ptr(box_d) if ntot else None, s)
        else:
            _lib.call("kg_sp_warp_masks", rec_p, inst_p, ntot, H, W, ptr(warped) if ntot else None, ptr(box_d) if ntot else None, s)
        _lib.call("kg_sp_boxes", rec_p, N, ptr(box_d) if ntot else None, ntot, cfg.KP_RADIUS, ptr(counts_d), ptr(gtb_d) if ntot else None,
                  ptr(kp_d) if ntot else None, ptr(keep_d) if ntot else None, s)
        # the batch's only device -> host copy: the counts and the gt_bboxes rows
        host = torch.empty(n_host, dtype=torch.int32, pin_memory=True)
        host.copy_(cells[:n_host], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        hn = host.numpy()
        counts = hn[:N * 5].reshape(N, 5).copy()
        gtb = hn[N * 5:].view(np.float32).reshape(ntot, 5)
        gts = [torch.empty(N, 55, H // sc, W // sc, dtype=torch.float32, device=dev) for sc in DIVIDE_SCALES]
        inst_masks, gt_bboxes, warped_l, kps = [], [], [], []
        for i in range(N):
            i0, n = int(rec["inst0"][i]), int(rec["n"][i])
            m = int(counts[i, 4])
            wi = warped[i0:i0 + n]
            warped_l.append(wi)
            # every instance kept (the usual case): the warped masks are gt_masks as they are
            inst_masks.append(wi if m == n else wi.index_select(0, keep_d[i0:i0 + m].long()))
            gt_bboxes.append(gtb[i0:i0 + m].copy())
            kl = []
            for l, sc in enumerate(DIVIDE_SCALES):
                k = kp_d[l, i0:i0 + int(counts[i, l])]
                kl.append(k)
                preprocessing.get_ground_truth_device(k, H // sc, W // sc, dev, out=gts[l][i])   # dataset_base.py:94-102
            kps.append(kl)
    return PreparedBatch(img_out, tuple(gts), inst_masks, gt_bboxes, warped_l, kps, counts)


def prepare_batch(images, masks, params, input_h, input_w, device=None):
    """images: N uint8 [h,w,3] arrays or tensors (host or device, any sizes); masks: per image the [n,h,w] instance masks as a device
    uint8 / float32 tensor, a BitMasks or a host NumPy array, or -- for all images of the batch or for none -- a LabelSource; params: N
    SampleParams (draw_train_params / identity_params).
    Returns collater's tuple (img, gt_c0, gt_c1, gt_c2, gt_c3, instance_masks, bboxes_c0) with device tensors throughout, except the
    [m,5] box arrays of the last element, which SEG_loss matches on the host."""
    b = prepare_batch_full(images, masks, params, input_h, input_w, device)
    return (b.img,) + b.gt + (b.instance_masks, b.gt_bboxes)


def warp_labels(labels_list, params, input_h, input_w, device=None):
    """The label maps themselves through the transform: labels_list = N int32 [h, w] device tensors or host integer arrays (any sizes),
    params = N SampleParams -> device int32 [N, H, W], out[i][y][x] = labels_i[sy][sx] inside the paste window and 0 outside
    (kg_sp_warp_labelmap, one launch).  Ground truth at the network's size, for labelmetrics against a prediction made there."""
    dev = _device(device)
    H, W = int(input_h), int(input_w)
    N = len(labels_list)
    if N == 0 or len(params) != N:
        raise ValueError("sampleprep: labels_list and params must be non-empty lists of one length")
    if H <= 0 or W <= 0 or H % 8 or W % 8 or W > MAX_WIDTH:
        raise ValueError(f"sampleprep: the network input {H} x {W} must be multiples of 8 (KGnet's pyramid), at most {MAX_WIDTH} wide")
    srcs = [m if isinstance(m, LabelSource) else LabelSource(m, n=0) for m in labels_list]
    rec = np.zeros(N, _REC)
    resolved = [p.resolved(*s.shape) for p, s in zip(params, srcs)]
    with torch.cuda.device(dev):
        maps = [s.on(dev) for s in srcs]
        for i, (lab, p) in enumerate(zip(maps, params)):
            _, _, _, He, We, oy, ox = resolved[i]
            flags = (_MIRROR_W if p.mirror_w else 0) | (_MIRROR_H if p.mirror_h else 0) | _LABELS
            rec[i] = (0, lab.data_ptr(), lab.shape[0], lab.shape[1], He, We, oy, ox, flags, 0, np.float32(0), np.float32(1), 0, 0, 0, 0)
        tab_d = ops.h2d(rec.view(np.uint8), dev)
        out = torch.empty(N, H, W, dtype=torch.int32, device=dev)
        _lib.call("kg_sp_warp_labelmap", ptr(tab_d), N, H, W, ptr(out), stream_ptr())
    return out


# ---- host statements of the label route (NumPy; the yardstick of the GPU tests) ---------------------------------------------------------

def source_index_host(size, ce, off, mirror, dsize):
    """The composed map of one axis (the one tests/sampleprep_ref.py states): destination index -> source index, -1 outside the paste
    window.  v = min(floor(d * scale), ce - 1) with scale = 1 / (dsize / ce) in double; mirrored, v = ce - 1 - v; s = v - off."""
    scale = 1.0 / (float(dsize) / float(ce))
    v = np.minimum(np.floor(np.arange(dsize, dtype=np.float64) * scale).astype(np.int64), ce - 1)
    if mirror:
        v = ce - 1 - v
    s = v - off
    return np.where((s >= 0) & (s < size), s, -1)


def _host_map(fn, labels):
    lab = labels.cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)
    if lab.ndim != 2 or lab.dtype.kind not in "iu" or lab.size == 0:
        raise ValueError(f"sampleprep.{fn}: a label map must be a non-empty integer array [h, w]")
    return lab.astype(np.int64)


def _host_axes(lab, p, H, W):
    h, w = lab.shape
    _, _, _, He, We, oy, ox = p.resolved(h, w)
    return source_index_host(h, He, oy, p.mirror_h, H), source_index_host(w, We, ox, p.mirror_w, W)


def warp_labels_host(labels_list, params, input_h, input_w):
    """warp_labels in NumPy -> int32 [N, H, W]: labels[sy][sx] where sy and sx lie inside the paste window, 0 elsewhere."""
    H, W = int(input_h), int(input_w)
    out = np.zeros((len(labels_list), H, W), np.int32)
    for i, (labels, p) in enumerate(zip(labels_list, params)):
        lab = _host_map("warp_labels_host", labels)
        sy, sx = _host_axes(lab, p, H, W)
        inside = (sy >= 0)[:, None] & (sx >= 0)[None, :]
        out[i] = np.where(inside, lab[np.maximum(sy, 0)][:, np.maximum(sx, 0)], 0)
    return out


def label_masks_host(labels, jobs, params, input_h, input_w):
    """The masks kg_sp_warp_labels makes for ONE image, in NumPy: labels = integer [h, w]; jobs = integers [m, 5] = (id, y1, x1, y2, x2);
    params = the image's SampleParams -> uint8 [m, H, W].  Pixel (y, x) of row k is 1 iff its source index (sy, sx) lies inside the paste
    window, inside the job's half-open box clamped to [0, h] x [0, w], and labels[sy][sx] == id; otherwise 0."""
    H, W = int(input_h), int(input_w)
    lab = _host_map("label_masks_host", labels)
    h, w = lab.shape
    j = np.asarray(jobs, np.int64).reshape(-1, 5)
    sy, sx = _host_axes(lab, params, H, W)
    at = lab[np.maximum(sy, 0)][:, np.maximum(sx, 0)]                                    # [H, W]: the label every output pixel looks at
    y1, x1 = np.clip(j[:, 1], 0, h), np.clip(j[:, 2], 0, w)
    y2, x2 = np.clip(j[:, 3], 0, h), np.clip(j[:, 4], 0, w)
    rows = (sy[None, :] >= 0) & (sy[None, :] >= y1[:, None]) & (sy[None, :] < y2[:, None])   # [m, H]
    cols = (sx[None, :] >= 0) & (sx[None, :] >= x1[:, None]) & (sx[None, :] < x2[:, None])   # [m, W]
    out = np.empty((len(j), H, W), np.uint8)
    for a in range(0, len(j), 1024):
        b = min(a + 1024, len(j))
        out[a:b] = rows[a:b, :, None] & cols[a:b, None, :] & (at[None] == j[a:b, 0, None, None])
    return out
