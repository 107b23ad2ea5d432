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

_MIRROR_W, _MIRROR_H, _BITS = 1, 2, 4
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


def prepare_batch_full(images, masks, params, input_h, input_w, device=None):
    """prepare_batch with everything it computed (PreparedBatch)."""
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
    with torch.cuda.device(dev):
        for i in range(N):
            img = _image_on(images[i], dev)
            h, w = int(img.shape[0]), int(img.shape[1])
            mh, mptr, bits, n, ld = _masks_on(masks[i], h, w, dev)
            holders += [img, mh]
            delta, alpha, perm, He, We, oy, ox = resolved[i]
            flags = (_MIRROR_W if params[i].mirror_w else 0) | (_MIRROR_H if params[i].mirror_h else 0) | (_BITS if bits else 0)
            rec[i] = (img.data_ptr(), mptr if n else 0, h, w, He, We, oy, ox, flags, perm[0] | perm[1] << 2 | perm[2] << 4,
                      np.float32(delta), np.float32(alpha), ntot, n, ld, 0)
            ntot += n
        # one upload: the image table, then the image of every instance
        inst_img = np.repeat(np.arange(N, dtype=np.int32), rec["n"])
        tab = np.concatenate([rec.view(np.uint8), inst_img.view(np.uint8)])
        tab_d = ops.h2d(tab, dev)
        rec_p = _lib.c_void_p(tab_d.data_ptr())
        inst_p = _lib.c_void_p(tab_d.data_ptr() + rec.nbytes)
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
    uint8 / float32 tensor, a BitMasks or a host NumPy array; params: N SampleParams (draw_train_params / identity_params).
    Returns collater's tuple (img, gt_c0, gt_c1, gt_c2, gt_c3, instance_masks, bboxes_c0) with device tensors throughout, except the
    [m,5] box arrays of the last element, which SEG_loss matches on the host."""
    b = prepare_batch_full(images, masks, params, input_h, input_w, device)
    return (b.img,) + b.gt + (b.instance_masks, b.gt_bboxes)
