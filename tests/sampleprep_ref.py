"""NumPy restatement of the sample preparation (TEST INFRASTRUCTURE, not product), written from the reference's semantics:
BaseDataset.__getitem__ (dataset_base.py:81-116) under train.py:77-85's pipelines (transforms.py).  It is checked against the
reference's own outputs (tests/golden/sampleprep.npz, tools/gen_sampleprep_goldens.py) and against hand-computed vectors in
tests/test_sampleprep_cpu.py; kg_instance_segmentation_amd.sampleprep is checked against it bit for bit on the GPU.

The image follows the reference literally (float canvas, mirrors by slicing, one float32 INTER_LINEAR resize per channel with
oracle.paste.resize_linear_f32).  The masks go through the composed index map instead of an [n, He, We] canvas, so that 300-instance
samples fit in memory; `warp_masks_literal` is the canvas formulation, and the CPU test holds the two equal.

Parameters are any object with SampleParams' fields (brightness, delta, contrast, alpha, swap, perm, expand, canvas, offset,
mirror_w, mirror_h)."""
import numpy as np

from oracle.paste import resize_linear_f32

KP_RADIUS = 5
DIVIDE_SCALES = (1, 2, 4, 8)
EDGES = [(0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (1, 3), (1, 4), (2, 3), (2, 4), (3, 4)]
DIR_EDGES = EDGES + [e[::-1] for e in EDGES]


def nearest_index(ssize, dsize):
    """cv2.resize(..., INTER_NEAREST): source index of every destination index, src = min(floor(dst * scale), ssize - 1) with
    scale = 1 / (dsize / ssize) in double."""
    scale = 1.0 / (float(dsize) / float(ssize))
    return np.minimum(np.floor(np.arange(dsize, dtype=np.float64) * scale).astype(np.int64), ssize - 1)


def resize_nearest(a, dh, dw):
    return a[..., nearest_index(a.shape[-2], dh), :][..., nearest_index(a.shape[-1], dw)]


def _geometry(p, h, w):
    if p.expand:
        (He, We), (oy, ox) = p.canvas, p.offset
        return int(He), int(We), int(oy), int(ox)
    return h, w, 0, 0


def warp_image(img_u8, p, H, W):
    """uint8 [h,w,3] -> float32 [3,H,W] (transforms.py:18-176 on the image, dataset_base.py:104-106)."""
    img = np.asarray(img_u8).astype(np.float32)                       # ConvertImgFloat
    if p.brightness:
        img = (img + np.float32(p.delta)).astype(np.float32)          # transforms.py:45, float32 array += scalar
    if p.contrast:
        img = (img * np.float32(p.alpha)).astype(np.float32)          # transforms.py:32
    if p.swap:
        img = img[:, :, list(p.perm)]                                 # transforms.py:52
    h, w = img.shape[:2]
    He, We, oy, ox = _geometry(p, h, w)
    if p.expand:
        canvas = np.zeros((He, We, 3), np.float32)                    # mean 0 (train.py:79)
        canvas[oy:oy + h, ox:ox + w] = img
        img = canvas
    if p.mirror_w:
        img = img[:, ::-1, :]
    if p.mirror_h:
        img = img[::-1, :, :]
    out = np.stack([resize_linear_f32(img[:, :, c], H, W) for c in range(3)], 0)
    out = np.clip(out, np.float32(0.), np.float32(255.))
    return (out / np.float32(255) - np.float32(0.5)).astype(np.float32)


def source_index(size, ce, off, mirror, dsize):
    """The composed map of one axis: destination index -> source index, -1 outside Expand's window."""
    v = nearest_index(ce, dsize)
    if mirror:
        v = ce - 1 - v
    s = v - off
    return np.where((s >= 0) & (s < size), s, -1)


def warp_masks(masks, p, H, W):
    """[n,h,w] (non-zero = foreground) -> uint8 [n,H,W] of 0 / 1 through the composed index map."""
    m = (np.asarray(masks) != 0).astype(np.uint8)
    n, h, w = m.shape
    He, We, oy, ox = _geometry(p, h, w)
    sy = source_index(h, He, oy, p.mirror_h, H)
    sx = source_index(w, We, ox, p.mirror_w, W)
    out = m[:, np.maximum(sy, 0)][:, :, np.maximum(sx, 0)]
    out = out * ((sy >= 0)[None, :, None] & (sx >= 0)[None, None, :])
    return np.ascontiguousarray(out, np.uint8)


def warp_masks_literal(masks, p, H, W):
    """The same through the reference's own steps: canvas, mirrors by slicing, nearest resize per mask."""
    m = (np.asarray(masks) != 0).astype(np.float32)
    n, h, w = m.shape
    He, We, oy, ox = _geometry(p, h, w)
    if p.expand:
        canvas = np.zeros((n, He, We), np.float32)
        canvas[:, oy:oy + h, ox:ox + w] = m
        m = canvas
    if p.mirror_w:
        m = m[:, :, ::-1]
    if p.mirror_h:
        m = m[:, ::-1, :]
    return np.ascontiguousarray(resize_nearest(m, H, W)).astype(np.uint8).reshape(n, H, W)


def _extents(masks):
    """Per mask: non-empty flag and (y1, x1, y2, x2) of its ones."""
    rows, cols = masks.any(2), masks.any(1)
    ok = rows.any(1)
    H, W = rows.shape[1], cols.shape[1]
    y1, y2 = rows.argmax(1), H - 1 - rows[:, ::-1].argmax(1)
    x1, x2 = cols.argmax(1), W - 1 - cols[:, ::-1].argmax(1)
    return ok, y1, x1, y2, x2


def masks_to_bboxes(masks, scale):
    """dataset_base.py:58-79: float32 [n_l,5,2] keypoints (x,y) of tl, tr, bl, br, centre at divide scale `scale`, and the kept indices."""
    n, H, W = masks.shape
    hs, ws = int(float(H) / float(scale)), int(float(W) / float(scale))
    small = resize_nearest(masks, hs, ws) if n else masks.reshape(0, hs, ws)
    ok, y1, x1, y2, x2 = _extents(small == 1)
    keep = ok & ((y2 - y1) > KP_RADIUS * 2 + 1) & ((x2 - x1) > KP_RADIUS * 2 + 1)
    out = []
    for i in np.nonzero(keep)[0]:
        a, b, c, d = int(x1[i]), int(y1[i]), int(x2[i]), int(y2[i])
        out.append([(a, b), (c, b), (a, d), (c, d), (float(a + c) / 2, float(b + d) / 2)])
    return np.asarray(out, np.float32).reshape(-1, 5, 2), np.nonzero(keep)[0]


def load_gt_masks_bboxes(masks):
    """dataset_base.py:43-56: (kept masks float32 [m,H,W], float32 [m,5] = (y1,x1,y2,x2,1), kept indices)."""
    ok, y1, x1, y2, x2 = _extents(masks == 1)
    keep = ok & (np.abs(y2 - y1) > 2) & (np.abs(x2 - x1) > 2)
    idx = np.nonzero(keep)[0]
    bb = np.stack([y1[idx], x1[idx], y2[idx], x2[idx], np.ones(len(idx), np.int64)], 1).astype(np.float32).reshape(-1, 5)
    return masks[idx].astype(np.float32), bb, idx


def ground_truth(bboxes, H, W):
    """oracle.preproc.ground_truth's rules (preprocessing.py:107-118) evaluated per instance window instead of over [n,H,W] arrays:
    only pixels within KP_RADIUS of a keypoint can be owned by it, so each instance visits the (2R+3)^2 window around its keypoint, in
    instance order with a strict `<` (np.argmin's first index).  float64 [55,H,W]; held equal to the oracle in the CPU test."""
    bboxes = np.asarray(bboxes, np.float32).reshape(-1, 5, 2)
    n, R = len(bboxes), KP_RADIUS
    out = np.zeros((55, H, W), np.float64)
    owner = np.full((5, H, W), -1, np.int64)
    for i in range(5):
        best = np.full((H, W), np.inf)
        for j in range(n):
            kx, ky = np.float64(bboxes[j, i, 0]), np.float64(bboxes[j, i, 1])
            cx, cy = int(bboxes[j, i, 0]), int(bboxes[j, i, 1])
            # ownership
            ya, yb = max(cy - R - 1, 0), min(cy + R + 2, H)
            xa, xb = max(cx - R - 1, 0), min(cx + R + 2, W)
            if ya < yb and xa < xb:
                wy, wx = np.mgrid[ya:yb, xa:xb]
                d = np.sqrt(np.square(kx - wx) + np.square(ky - wy))
                upd = (d <= R) & (d < best[ya:yb, xa:xb])
                best[ya:yb, xa:xb][upd] = d[upd]
                owner[i, ya:yb, xa:xb][upd] = j
            # short offsets: last writer wins over the whole window
            y1, y2 = max(cy - R, 0), min(cy + R, H - 1) + 1
            x1, x2 = max(cx - R, 0), min(cx + R, W - 1) + 1
            if y1 < y2 and x1 < x2:
                wy, wx = np.mgrid[y1:y2, x1:x2]
                ox, oy = cx - wx, cy - wy
                inside = np.sqrt(ox * ox + oy * oy) <= R
                out[5 + 2 * i, y1:y2, x1:x2] = ox * inside
                out[5 + 2 * i + 1, y1:y2, x1:x2] = oy * inside
        out[i] = owner[i] >= 0
    ys, xs = np.mgrid[0:H, 0:W]
    for e, (a, b) in enumerate(DIR_EDGES):
        ok = owner[a] >= 0
        j = np.where(ok, owner[a], 0)
        if n:
            out[15 + 2 * e] = np.where(ok, bboxes[j, b, 0].astype(np.float64) - xs, 0.0)
            out[15 + 2 * e + 1] = np.where(ok, bboxes[j, b, 1].astype(np.float64) - ys, 0.0)
    return out


def prepare_sample(img_u8, masks, p, H, W, targets=True):
    """One sample as BaseDataset.__getitem__ returns it, as a dict: img [3,H,W] f32, warped [n,H,W] u8, bboxes (4 x [n_l,5,2] f32),
    gt (4 x [55,H/s,W/s] f32, when `targets`), gt_masks [m,H,W] f32, gt_bboxes [m,5] f32, counts int32 [5]."""
    masks = np.asarray(masks)
    if masks.ndim != 3:
        masks = masks.reshape(0, img_u8.shape[0], img_u8.shape[1])
    warped = warp_masks(masks, p, H, W)
    bbs = [masks_to_bboxes(warped, sc)[0] for sc in DIVIDE_SCALES]
    gt_masks, gt_bboxes, _ = load_gt_masks_bboxes(warped)
    out = dict(img=warp_image(img_u8, p, H, W), warped=warped, bboxes=bbs, gt_masks=gt_masks.reshape(-1, H, W), gt_bboxes=gt_bboxes,
               counts=np.array([len(b) for b in bbs] + [len(gt_bboxes)], np.int32))
    if targets:
        out["gt"] = [ground_truth(b, int(H / sc), int(W / sc)).astype(np.float32) for b, sc in zip(bbs, DIVIDE_SCALES)]
    return out
