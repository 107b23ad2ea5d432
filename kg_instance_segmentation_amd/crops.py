"""Instance crops: one fixed-size image patch and one mask per instance of a label map, without copying the map or the image back.

Every other label-map module produces integers ABOUT an instance.  The most common consumer of a nucleus segmentation is a second
network -- a cell-type classifier, a mitosis detector, an embedding model -- and it takes the instance itself: one fixed-size patch per
id, usually with the instance mask, often turned to the object's major axis.  The device gathers them in one launch (kg_label_crops,
csrc/crops.hip) from the label map and the source image that are already there, and the result stays there, channel-first, ready for
a torch model.

    crops_host              the semantics in NumPy, vectorised over jobs (the CPU route, the yardstick of the GPU tests)
    affine_jobs             the job table of windows, rotations and flips: the kernel knows nothing of them
    crop_rows               kg_label_crops as it is: ONE launch, everything stays on the device
    crops                   affine_jobs + crop_rows for a label map -> Crops
    crops_instances         crops for an Instances / TiledInstances
    crops_instances_batch   the same for predict_instances' list, one launch per output size
    Crops                   patches [m, C, OH, OW], masks uint8 [m, OH, OW], the job table; to_float, source_yx

Semantics (include/kgnet_hip.h is the normative text).  Everything is exact in integers.
  job         {img, id, oy, ox, ay, by, cy, ax, bx, cx}, ten int32.  Output pixel (i, j), 0 <= i < OH, 0 <= j < OW, samples the source
              position, in units of 1/65536 pixel with pixel centres at integers,
                  Y = (oy << 16) + ay*i + by*j + cy        X = (ox << 16) + ax*i + bx*j + cx        (int64)
  mask        yn = (Y + 32768) >> 16, xn = (X + 32768) >> 16 (arithmetic shifts).  mask = 1 iff 0 <= yn < H, 0 <= xn < W and
              labels[img][yn][xn] == id.  Labels are compared only: 0, -1, INT_MIN and INT_MAX are ordinary ids.
  linear      y0 = Y >> 16, fy = Y & 65535, x0 and fx likewise.  A tap (y, x) inside the map is the image element, read unsigned; a tap
              outside is `fill`.  acc = (65536-fy)*((65536-fx)*v00 + fx*v01) + fy*((65536-fx)*v10 + fx*v11), the value is
              (acc + 2^31) >> 32.  acc < 2^48.
  nearest     the tap at (yn, xn), or fill
  masked      after sampling, a pixel whose mask is 0 becomes fill
  outputs     patches [m][C][OH][OW] in the image's element type, masks [m][OH][OW] uint8.  No image gives masks only, masks=False gives
              patches only.  1 <= OH, OW <= 256, 0 <= fill <= 65535 (<= 255 for uint8 patches), m * C * OH * OW <= 2^31 - 1.
  bad jobs    a job with img outside [0, nimg) gets fill and a zero mask.  No other job is bad: a window that lies beyond the map is
              padding.  Every output element is written.
  closed forms  ay = bx = 65536, the rest 0: an exact copy of the slice.  ay = bx = 131072, cy = cx = 32768: the mean of each 2 x 2 block
              rounded half up.  An all-65535 image stays 65535 under any fractions.  {ay, by, ax, bx} = {0, -65536, 65536, 0}: np.rot90(k=-1)
              of the unrotated patch and of its mask.

The table (affine_jobs; rhu = round half up, Python integers, so scale 1 is exact)
  angle=None  window="square" (the default): a square of side max(h, w) + 2 margin around the box centre; window="box": the box grown by
              margin, mapped anisotropically onto OH x OW.  A window [wy, wy + wh) gives ay = rhu(65536 wh / OH), oy = wy,
              cy = rhu(65536 (wh - OH) / (2 OH)) -- the align_corners=False convention; a square window whose centre falls between two
              pixel edges has wy = floor and 32768 more in cy.  X likewise.
  angle=t     radians per instance in measure.py's orientation convention (from the row axis towards the column axis); "major" takes
              it from the measurements.  The patch's row axis points along (cos t, sin t) in (y, x): ay = rhu(s cos t), ax = rhu(s sin t),
              by = rhu(-s sin t), bx = rhu(s cos t) with s = 65536 side / OH; side=None is the box diagonal rounded up, + 2 margin (what
              no rotation can cut), a number, or one per instance.  The offset places the window centre ((y1 + y2 - 1) / 2,
              (x1 + x2 - 1) / 2) at the patch centre and is split into oy and a remainder cy in [0, 65536).  OH == OW.  Float64 builds
              these coefficients, rounded once; the table is the contract between the host and the device route.
  flip        "h" mirrors the patch's columns (by, bx negated), "v" its rows (ay, ax negated), "hv" both; the offset moves by the
              negated column times (size - 1).
  empty       an instance with no visible pixel (an empty box) gets img = -1, hence fill and an empty mask."""
import math

import numpy as np

from . import _lib, _labelmaps, labelmetrics
from ._labelmaps import device_jobs, instance_stats, is_device, job_table

KGLibraryError = _lib.KGLibraryError
MAX_SIZE = 256
ONE = 65536
NEAREST, MASKED = 1, 2                                                   # flags of kg_label_crops
MODES = ("linear", "nearest")
_JOB_COLUMNS = "(img, id, oy, ox, ay, by, cy, ax, bx, cx)"
_I32 = (-2 ** 31, 2 ** 31 - 1)


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------

def _size(fn, size):
    s = (size, size) if np.ndim(size) == 0 else tuple(size)
    if len(s) != 2 or any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 1 <= v <= MAX_SIZE for v in s):
        raise KGLibraryError(f"{fn}: size {size!r} (an integer in 1 .. {MAX_SIZE}, or (OH, OW) of them)")
    return int(s[0]), int(s[1])


def _flags(fn, mode, masked):
    if mode not in MODES:
        raise KGLibraryError(f"{fn}: mode {mode!r} ({' or '.join(MODES)})")
    return (NEAREST if mode == "nearest" else 0) | (MASKED if masked else 0)


def _fill(fn, fill, elem_bytes):
    top = 65535 if elem_bytes != 1 else 255
    if isinstance(fill, (bool, np.bool_)) or not isinstance(fill, (int, np.integer)) or not 0 <= fill <= top:
        raise KGLibraryError(f"{fn}: fill {fill!r} (an integer in 0 .. {top})")
    return int(fill)


def _count(fn, m, C, OH, OW):
    if m * C * OH * OW > 2 ** 31 - 1:
        raise KGLibraryError(f"{fn}: m * C * OH * OW exceeds 2^31 - 1 ({m} jobs, {C} channel(s), {OH} x {OW})")


# ---- the table ------------------------------------------------------------------------------------------------------------------------

def _rhu_div(num, den):
    """round-half-up of num / den on int64 arrays, den > 0"""
    return (2 * num + den) // (2 * den)


def affine_jobs(jobs, size=64, window="square", margin=0, angle=None, side=None, flip=None):
    """jobs: integers [m, 6] = (img, id, y1, x1, y2, x2), half-open boxes (job_table's result); size: OH == OW, or (OH, OW); window:
    "square" or "box"; margin: pixels of context around the box, an integer >= 0; angle: None, or radians, a number or one per job;
    side: with an angle, the side of the square window in source pixels: None (the box diagonal rounded up + 2 margin), a number or one
    per job; flip: None, "h", "v" or "hv" -> int64 [m, 10] = (img, id, oy, ox, ay, by, cy, ax, bx, cx), every entry inside int32.  An
    empty box gets img = -1.  The module docstring states the rule."""
    fn = "affine_jobs"
    OH, OW = _size(fn, size)
    j = np.asarray(jobs)
    if j.ndim != 2 or j.shape[1] != 6 or j.dtype.kind not in "iu":
        raise KGLibraryError(f"{fn}: jobs must be integers [m, 6] = {_labelmaps.JOB_COLUMNS}")
    j = j.astype(np.int64)
    m = len(j)
    if window not in ("square", "box"):
        raise KGLibraryError(f"{fn}: window {window!r} (\"square\" or \"box\")")
    if isinstance(margin, (bool, np.bool_)) or not isinstance(margin, (int, np.integer)) or not 0 <= margin <= _labelmaps.MAX_SIDE:
        raise KGLibraryError(f"{fn}: margin {margin!r} (an integer in 0 .. {_labelmaps.MAX_SIDE})")
    if flip not in (None, "h", "v", "hv", "vh"):
        raise KGLibraryError(f"{fn}: flip {flip!r} (None, \"h\", \"v\" or \"hv\")")
    margin = int(margin)
    y1, x1, y2, x2 = j[:, 2], j[:, 3], j[:, 4], j[:, 5]
    h, w = y2 - y1, x2 - x1
    empty = (h <= 0) | (w <= 0)
    if angle is None:
        if side is not None:
            raise KGLibraryError(f"{fn}: side is the window of a rotated crop: it needs an angle")
        if window == "square":
            s = np.maximum(h, w) + 2 * margin
            ty, tx, wh, ww = y1 + y2 - s, x1 + x2 - s, s, s          # twice the window's first edge: the centre may fall between two edges
            wy, wx, hy, hx = ty >> 1, tx >> 1, (ty & 1) * (ONE // 2), (tx & 1) * (ONE // 2)
        else:
            wy, wx, wh, ww = y1 - margin, x1 - margin, h + 2 * margin, w + 2 * margin
            hy = hx = np.zeros(m, np.int64)
        wh, ww = np.where(empty, OH, wh), np.where(empty, OW, ww)
        ay, bx = _rhu_div(ONE * wh, OH), _rhu_div(ONE * ww, OW)
        by = ax = np.zeros(m, np.int64)
        oy, ox = wy, wx
        cy, cx = (ONE * (wh - OH) + OH) // (2 * OH) + hy, (ONE * (ww - OW) + OW) // (2 * OW) + hx
    else:
        if OH != OW:
            raise KGLibraryError(f"{fn}: a rotated crop needs a square patch, not {OH} x {OW}")
        t = np.asarray(angle, np.float64)
        if t.ndim > 1 or (t.ndim == 1 and len(t) != m):
            raise KGLibraryError(f"{fn}: angle must be a number or one per job ({m})")
        t = np.where(empty, 0.0, np.broadcast_to(t, (m,)))
        if not np.isfinite(t).all():
            raise KGLibraryError(f"{fn}: an angle is not finite")
        if side is None:
            sd = np.array([math.isqrt(int(a) * int(a) + int(b) * int(b) - 1) + 1 if a > 0 and b > 0 else 1 for a, b in zip(h.tolist(), w.tolist())],
                          np.float64).reshape(m) + 2 * margin
        else:
            sd = np.asarray(side, np.float64)
            if sd.ndim > 1 or (sd.ndim == 1 and len(sd) != m) or not (np.isfinite(sd).all() and (sd > 0).all() and (sd <= 4 * _labelmaps.MAX_SIDE).all()):
                raise KGLibraryError(f"{fn}: side must be a positive number or one per job ({m}), at most {4 * _labelmaps.MAX_SIDE}")
            sd = np.broadcast_to(sd, (m,))
        sc = ONE * sd / OH
        co, si = np.floor(sc * np.cos(t) + 0.5).astype(np.int64), np.floor(sc * np.sin(t) + 0.5).astype(np.int64)
        ay, ax, by, bx = co, si, np.floor(-sc * np.sin(t) + 0.5).astype(np.int64), co
        # twice the offset: 65536 (y1 + y2 - 1) - (ay (OH - 1) + by (OW - 1)), halved with round half up
        Ty = (ONE * (y1 + y2 - 1) - (ay * (OH - 1) + by * (OW - 1)) + 1) >> 1
        Tx = (ONE * (x1 + x2 - 1) - (ax * (OH - 1) + bx * (OW - 1)) + 1) >> 1
        oy, ox, cy, cx = Ty >> 16, Tx >> 16, Ty & (ONE - 1), Tx & (ONE - 1)
    if flip is not None and "h" in flip:
        cy, cx, by, bx = cy + by * (OW - 1), cx + bx * (OW - 1), -by, -bx
    if flip is not None and "v" in flip:
        cy, cx, ay, ax = cy + ay * (OH - 1), cx + ax * (OH - 1), -ay, -ax
    far_y, far_x = np.abs(cy) >= 2 ** 30, np.abs(cx) >= 2 ** 30          # a remainder that a flip pushed out: whole pixels go to the origin
    oy, cy = np.where(far_y, oy + (cy >> 16), oy), np.where(far_y, cy & (ONE - 1), cy)
    ox, cx = np.where(far_x, ox + (cx >> 16), ox), np.where(far_x, cx & (ONE - 1), cx)
    out = np.stack([np.where(empty, -1, j[:, 0]), j[:, 1], oy, ox, ay, by, cy, ax, bx, cx], 1).astype(np.int64).reshape(-1, 10)
    if out.size and (out.min() < _I32[0] or out.max() > _I32[1]):
        raise KGLibraryError(f"{fn}: a coefficient leaves int32")
    return out


# ---- host statement of the semantics ----------------------------------------------------------------------------------------------------

def _crops_host(maps, img, j, OH, OW, flags, fill, want_masks):
    nimg, H, W = maps.shape
    m = len(j)
    nearest, masked = bool(flags & NEAREST), bool(flags & MASKED)
    patches = None if img is None else np.empty((m, img.shape[3], OH, OW), img.dtype)
    masks = np.empty((m, OH, OW), np.uint8) if want_masks else None
    ii, jj = np.arange(OH, dtype=np.int64)[None, :, None], np.arange(OW, dtype=np.int64)[None, None, :]
    step = max(1, (1 << 20) // (OH * OW))                                # jobs per slab: the temporaries stay small
    for a in range(0, m, step):
        q = j[a:a + step]

        def col(k):
            return q[:, k][:, None, None]
        Y = (col(2) << 16) + col(4) * ii + col(5) * jj + col(6)
        X = (col(3) << 16) + col(7) * ii + col(8) * jj + col(9)
        live = ((q[:, 0] >= 0) & (q[:, 0] < nimg))[:, None, None]
        im = np.where(live, col(0), 0)

        def inside(y, x):
            return live & (y >= 0) & (y < H) & (x >= 0) & (x < W)
        yn, xn = (Y + 32768) >> 16, (X + 32768) >> 16
        inn = inside(yn, xn)
        mk = None
        if want_masks or masked:
            mk = inn & (maps[im, np.clip(yn, 0, H - 1), np.clip(xn, 0, W - 1)].astype(np.int64) == col(1))
        if want_masks:
            masks[a:a + step] = mk
        if img is None:
            continue

        def tap(y, x):
            v = img[im, np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)].astype(np.int64)
            return np.where(inside(y, x)[..., None], v, fill)
        if nearest:
            val = tap(yn, xn)
        else:
            y0, x0, fy, fx = Y >> 16, X >> 16, (Y & 65535)[..., None], (X & 65535)[..., None]
            acc = (ONE - fy) * ((ONE - fx) * tap(y0, x0) + fx * tap(y0, x0 + 1)) + fy * ((ONE - fx) * tap(y0 + 1, x0) + fx * tap(y0 + 1, x0 + 1))
            val = (acc + 2 ** 31) >> 32
        if masked:
            val = np.where(mk[..., None], val, fill)
        patches[a:a + step] = np.moveaxis(val, 3, 1)
    return patches, masks


def crops_host(labels, jobs, image=None, size=64, mode="linear", masked=False, fill=0, masks=True):
    """labels: integers [H, W] or [nimg, H, W]; jobs: integers [m, 10] = (img, id, oy, ox, ay, by, cy, ax, bx, cx); image: None (masks
    only) or uint8 / uint16 [H, W, C] / [nimg, H, W, C]; size: OH == OW or (OH, OW); masks=False: patches only -> (patches
    [m, C, OH, OW] in the image's dtype or None, masks uint8 [m, OH, OW] or None).  From the definition, vectorised over jobs."""
    fn = "crops_host"
    maps = _labelmaps.host_stack(fn, labels, _labelmaps.SUMS_FIT)
    img = _labelmaps.host_image(fn, image, maps.shape)
    if img is None and not masks:
        raise KGLibraryError(f"{fn}: no image and no masks: nothing to produce")
    OH, OW = _size(fn, size)
    j = _labelmaps.host_jobs(fn, jobs, 10, _JOB_COLUMNS).astype(np.int64)
    _count(fn, len(j), 1 if img is None else img.shape[3], OH, OW)
    return _crops_host(maps, img, j, OH, OW, _flags(fn, mode, masked), _fill(fn, fill, 2 if img is None else img.dtype.itemsize), bool(masks))


# ---- the result -------------------------------------------------------------------------------------------------------------------------

class Crops:
    """patches = a device tensor [m, C, OH, OW] in the image's element type (int16 storage of a uint16 image is read unsigned), or None;
    masks = device uint8 [m, OH, OW], or None; jobs = host int64 [m, 10], the table the patches were taken with (in a batch, img counts the
    images of one output size); size = (OH, OW); mode, fill as given.  (A host label map gives host tensors.)"""
    __slots__ = ("patches", "masks", "jobs", "size", "mode", "fill")

    def __init__(self, patches, masks, jobs, size, mode="linear", fill=0):
        self.patches, self.masks = patches, masks
        self.jobs = np.ascontiguousarray(jobs, np.int64).reshape(-1, 10)
        self.size, self.mode, self.fill = (int(size[0]), int(size[1])), mode, int(fill)

    def __len__(self):
        return len(self.jobs)

    def to_float(self, mean=None, std=None):
        """float32 [m, C, OH, OW] by torch ops, on the patches' device: (v - mean) / std with v the element read unsigned; mean, std: None,
        a number or one per channel."""
        import torch
        if self.patches is None:
            raise KGLibraryError("Crops.to_float: no patches were taken (masks only)")
        p = self.patches
        x = (p.to(torch.int32) & 0xFFFF).to(torch.float32) if p.dtype == torch.int16 else p.to(torch.float32)
        for v, op in ((mean, torch.sub), (std, torch.div)):
            if v is not None:
                x = op(x, torch.as_tensor(v, dtype=torch.float32, device=x.device).reshape(1, -1, 1, 1))
        return x

    def source_yx(self, k, i, j):
        """The source position (y, x), float64 in pixels with pixel centres at integers, of pixel (i, j) of patch k -- so that a result
        of the downstream model (a keypoint, a saliency map) maps back.  k, i, j broadcast; i and j may be fractional."""
        q = self.jobs[np.asarray(k, np.int64)].astype(np.float64)
        i, j = np.asarray(i, np.float64), np.asarray(j, np.float64)
        return (q[..., 2] + (q[..., 4] * i + q[..., 5] * j + q[..., 6]) / ONE, q[..., 3] + (q[..., 7] * i + q[..., 8] * j + q[..., 9]) / ONE)


# ---- device -----------------------------------------------------------------------------------------------------------------------------

def _device_maps_image(fn, labels, image):
    """-> (maps [nimg, H, W], image [nimg, H, W, C] or None): device_args, with the image optional"""
    if image is None:
        return _labelmaps.device_stack(fn, labels, _labelmaps.SUMS_FIT)[0], None
    return _labelmaps.device_args(fn, labels, image)


def _launch(lab, img, jd, OH, OW, flags, fill, want_masks):
    import torch
    from ._lib import ptr, stream_ptr
    nimg, H, W = lab.shape
    m = jd.shape[0]
    patches = None if img is None else torch.empty((m, img.shape[3], OH, OW), dtype=img.dtype, device=lab.device)
    masks = torch.empty((m, OH, OW), dtype=torch.uint8, device=lab.device) if want_masks else None
    C, eb = (1, 1) if img is None else (img.shape[3], img.element_size())
    with torch.cuda.device(lab.device):
        _lib.call("kg_label_crops", ptr(lab), nimg, H, W, ptr(img), C, eb, ptr(jd) if m else None, m, OH, OW, flags, fill,
                  ptr(patches) if m else None, ptr(masks) if m else None, stream_ptr())
    return patches, masks


def crop_rows(labels, jobs, image=None, size=64, mode="linear", masked=False, fill=0, masks=True):
    """kg_label_crops as it is: labels device int32 [H, W] or [nimg, H, W]; jobs host integers [m, 10] (uploaded once) or a device int32
    tensor; image None (masks only), a host array (uploaded once) or a device tensor -> (patches device [m, C, OH, OW] or None, masks
    device uint8 [m, OH, OW] or None).  One launch, no copy back, no synchronisation."""
    fn = "crop_rows"
    lab, img = _device_maps_image(fn, labels, image)
    if img is None and not masks:
        raise KGLibraryError(f"{fn}: no image and no masks: nothing to produce")
    OH, OW = _size(fn, size)
    flags, fill = _flags(fn, mode, masked), _fill(fn, fill, 2 if img is None else img.element_size())
    jd = device_jobs(fn, jobs, 10, _JOB_COLUMNS, lab.device)
    _count(fn, jd.shape[0], 1 if img is None else img.shape[3], OH, OW)
    return _launch(lab, img, jd, OH, OW, flags, fill, bool(masks))


def _angles(fn, angle, m, major):
    """angle: None, "major" (major: a function -> orientations [m]), a number or one per job"""
    if isinstance(angle, str):
        if angle != "major":
            raise KGLibraryError(f"{fn}: angle {angle!r} (None, radians, or \"major\")")
        if m == 0:
            return np.zeros(0)
        return np.nan_to_num(np.asarray(major(), np.float64).reshape(m), nan=0.0)
    return angle


def _device_crops(fn, lab, img, j, size, window, margin, angle, side, flip, mode, masked, fill, masks, major):
    """lab, img: device tensors (img may be None); j: clamped host jobs [m, 6] -> Crops"""
    OH, OW = _size(fn, size)
    if img is None and not masks:
        raise KGLibraryError(f"{fn}: no image and no masks: nothing to produce")
    flags, fill = _flags(fn, mode, masked), _fill(fn, fill, 2 if img is None else img.element_size())
    _count(fn, len(j), 1 if img is None else img.shape[3], OH, OW)
    table = affine_jobs(j, (OH, OW), window, margin, _angles(fn, angle, len(j), major), side, flip)
    patches, mk = _launch(lab, img, _labelmaps.upload_jobs(table, lab.device), OH, OW, flags, fill, bool(masks))
    return Crops(patches, mk, table, (OH, OW), mode, fill)


def crops(labels, n=None, jobs=None, stats=None, image=None, size=64, window="square", margin=0, angle=None, side=None, flip=None,
          mode="linear", masked=False, fill=0, masks=True):
    """crops_host over affine_jobs' table, on the device -> Crops.  labels: device int32 [H, W] or [nimg, H, W].  What is taken:
      jobs   integers [m, 6] = (img, id, y1, x1, y2, x2), a host array or a device tensor (copied back: the table is built on the host); or
      n      the instance count (one per map for a stack): the ids 1 .. n inside their own boxes.  The boxes come from stats -- host
             integers [n, 5] = (area, y1, x1, y2, x2), one array per map for a stack -- or, without stats, from labelmetrics.label_stats.
    image: None (masks only), a host uint8 / uint16 array [H, W, C] / [nimg, H, W, C] (uploaded once) or a device tensor; size, window,
    margin, angle, side, flip as affine_jobs (angle="major": measure.measure's orientation, one more launch and copy back); mode "linear"
    or "nearest"; masked; fill; masks=False: patches only.  ONE kg_label_crops launch, one upload (the table), nothing copied back."""
    import torch
    fn = "crops"
    lab, img = _device_maps_image(fn, labels, image)
    if torch.is_tensor(jobs):
        jobs = jobs.cpu().numpy()
    j = job_table(fn, lab, n, jobs, stats, labelmetrics.label_stats)

    def major():
        from . import measure
        return measure.measure(lab, jobs=j).props()["orientation"]
    return _device_crops(fn, lab, img, j, size, window, margin, angle, side, flip, mode, masked, fill, masks, major)


# ---- Instances ----------------------------------------------------------------------------------------------------------------------------

def _known_major(inst):
    ms = getattr(inst, "measurements", None)
    return None if ms is None or len(ms) != len(inst) else ms.props()["orientation"]


def crops_instances(inst, image=None, size=64, window="square", margin=0, angle=None, side=None, flip=None, mode="linear", masked=False,
                    fill=0, masks=True):
    """crops for an Instances / TiledInstances -> Crops with len(inst) rows: ids 1 .. n, boxes from table[:, 2:6]; an instance with no
    visible pixel gets fill and an empty mask.  image: None, or uint8 / uint16 [H, W, C] at the label map's size (host array or device
    tensor).  angle="major" takes the orientation from inst.measurements, and measures the geometry first when that is absent.  A host
    label map (assemble_host's result) goes through crops_host and gives host tensors."""
    import torch
    fn = "crops_instances"
    stats = instance_stats(fn, inst)

    def major():
        from . import measure
        known = _known_major(inst)
        return known if known is not None else measure.measure_instances(inst).props()["orientation"]
    if is_device(inst.labels):
        lab, img = _device_maps_image(fn, inst.labels, image)
        j = job_table(fn, lab, len(inst), None, stats, None)
        return _device_crops(fn, lab, img, j, size, window, margin, angle, side, flip, mode, masked, fill, masks, major)
    maps = _labelmaps.host_stack(fn, _labelmaps.host_labels(inst), _labelmaps.SUMS_FIT)
    table = affine_jobs(job_table(fn, maps, len(inst), None, stats, None), size, window, margin, _angles(fn, angle, len(inst), major), side, flip)
    p, k = crops_host(maps, table, None if image is None else _labelmaps.host_pixels(image), size, mode, masked, fill, masks)
    as_t = lambda a: None if a is None else torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)  # noqa: E731
    return Crops(as_t(p), as_t(k), table, _size(fn, size), mode, fill)


def crops_instances_batch(insts, images=None, size=64, window="square", margin=0, angle=None, side=None, flip=None, mode="linear",
                          masked=False, fill=0, masks=True):
    """crops_instances for predict_instances' list (entries may be None), in place: every entry's `crops` is set.  ONE kg_label_crops
    launch for all images of one output size.  images: None (masks only), or uint8 / uint16 [N, h, w, C] (host array or device tensor),
    one image per entry, at the label maps' size.  angle="major" takes the orientations from the entries' measurements when all of a
    size have them, and measures the geometry of that size otherwise (one more launch and copy back)."""
    fn = "crops_instances_batch"
    if images is not None and len(images) != len(insts):
        raise KGLibraryError(f"crops: {len(images)} images for {len(insts)} entries")
    if side is not None and np.ndim(side) != 0:
        raise KGLibraryError(f"{fn}: side must be None or one number for a batch")
    if angle is not None and not isinstance(angle, str) and np.ndim(angle) != 0:
        raise KGLibraryError(f"{fn}: angle must be None, \"major\" or one number for a batch")
    for idx, stack, _, _ in _labelmaps.size_batches(fn, insts):
        lab, img = _device_maps_image(fn, stack, None if images is None else (images[idx] if len(idx) != len(insts) else images))
        ns, stats = [len(insts[i]) for i in idx], [instance_stats(fn, insts[i]) for i in idx]
        j = job_table(fn, lab, ns, None, stats, None)

        def major():
            from . import measure
            known = [_known_major(insts[i]) for i in idx]
            if all(k is not None for k in known):
                return np.concatenate(known) if known else np.zeros(0)
            return measure.measure(lab, ns, stats=stats).props()["orientation"]
        got = _device_crops(fn, lab, img, j, size, window, margin, angle, side, flip, mode, masked, fill, masks, major)
        for i, a, b in _labelmaps.deal(insts, idx):
            insts[i].crops = Crops(None if got.patches is None else got.patches[a:b], None if got.masks is None else got.masks[a:b],
                                   got.jobs[a:b], got.size, got.mode, got.fill)
    return insts
