#!/usr/bin/env python
"""Generates tests/golden/sampleprep.npz by running THE REFERENCE's own sample preparation (read-only import, CPU only):
transforms.Compose (train and val pipelines of train.py:77-85), BaseDataset.__getitem__ through a tiny in-memory subclass, collater.

    PYTHONDONTWRITEBYTECODE=1 KG_REFERENCE=/path/to/reference python tools/gen_sampleprep_goldens.py

Shims, as in tools/gen_goldens.py: `np.int = int`, and a stub `cv2` whose `resize` is the two pinned interpolation rules -- INTER_NEAREST:
src = min(floor(dst * scale), ssize - 1) with scale = 1 / (dsize / ssize) in double; INTER_LINEAR: oracle.paste.resize_linear_f32 per
channel -- so interpolation parity with an OpenCV binary stays unpinned exactly as oracle/paste.py says.  Everything else is the
reference's arithmetic: RNG call order, photometric float arithmetic, Expand geometry, mirrors, box filters, tuple layout.

Recorded (data only): the two source samples, per seed and sample the random draws in call order (kind 0 = randint, 1 = uniform) and the
image shape after every transform, the four keypoint lists, gt_masks (as bytes), gt_bboxes, SHA-256 of the float32 image and of the four
target tensors, and the full image / targets of the first seeds."""
import hashlib
import os
import sys
import types
import warnings

sys.dont_write_bytecode = True
warnings.filterwarnings("ignore")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = os.environ.get("KG_REFERENCE")
if not REF or not os.path.isdir(REF):
    raise SystemExit("gen_sampleprep_goldens: set KG_REFERENCE to a checkout of the reference project")
sys.path.insert(1, REF)

import numpy as np

np.int = int
from oracle.paste import resize_linear_f32  # noqa: E402


def _nearest_index(ssize, dsize):
    scale = 1.0 / (float(dsize) / float(ssize))
    return np.minimum(np.floor(np.arange(dsize, dtype=np.float64) * scale).astype(np.int64), ssize - 1)


def _resize(a, dsize, interpolation=1):
    w1, h1 = dsize
    a = np.asarray(a)
    if interpolation == 0:
        return np.ascontiguousarray(a[_nearest_index(a.shape[0], h1)][:, _nearest_index(a.shape[1], w1)])
    if a.ndim == 2:
        return resize_linear_f32(a, h1, w1)
    return np.stack([resize_linear_f32(a[:, :, c], h1, w1) for c in range(a.shape[2])], 2)


cv2 = types.ModuleType("cv2")
cv2.INTER_NEAREST, cv2.INTER_LINEAR = 0, 1
cv2.resize = _resize
sys.modules["cv2"] = cv2

import collater as rcollater  # noqa: E402
import dataset_base as rdataset  # noqa: E402
import transforms as rtransforms  # noqa: E402

H = W = 64
SEEDS = list(range(16))
FULL = 2                         # seeds whose image and target tensors are stored in full


class _Draws:
    """np.random as transforms.py sees it, logging every draw in call order."""
    def __init__(self):
        self.log = []

    def randint(self, *a):
        v = np.random.randint(*a)
        self.log.append((0, float(v)))
        return v

    def uniform(self, *a):
        v = np.random.uniform(*a)
        self.log.append((1, float(v)))
        return v


class _Shapes:
    """A transform that records the image shape after itself."""
    def __init__(self, t, log):
        self.t, self.log = t, log

    def __call__(self, img, mask):
        img, mask = self.t(img, mask)
        self.log.append(img.shape[:2])
        return img, mask


class _Memory(rdataset.BaseDataset):
    def __init__(self, samples, transform):
        self.samples, self.transform, self.img_ids = samples, transform, list(range(len(samples)))
        self.boxes = []

    def load_image(self, index):
        return self.samples[index][0].copy()

    def load_annotation(self, index, type="mask"):
        return self.samples[index][1].copy()

    def masks_to_bboxes(self, masks, divide_scale=1.):
        r = super().masks_to_bboxes(masks, divide_scale)
        self.boxes.append(r[0])
        return r


def sources():
    """Two decoded samples: 40 x 56 with 7 instances, 64 x 48 with 8; each holds large, medium, thin and tiny instances so that the
    box filters of dataset_base.py:53,72 both keep and drop."""
    rng = np.random.RandomState(7)
    out = []
    for (h, w), shapes in (((40, 56), [(2, 3, 30, 36), (5, 20, 22, 30), (20, 2, 18, 20), (8, 40, 26, 14), (30, 30, 2, 2), (1, 50, 30, 3), (33, 8, 6, 40)]),
                           ((64, 48), [(0, 0, 40, 40), (10, 5, 30, 24), (30, 20, 28, 26), (45, 2, 16, 18), (3, 30, 20, 15), (60, 44, 3, 3), (20, 45, 40, 2),
                                       (50, 25, 13, 22)])):
        img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        yy, xx = np.mgrid[0:h, 0:w]
        masks = []
        for k, (y, x, a, b) in enumerate(shapes):
            box = (yy >= y) & (yy < y + a) & (xx >= x) & (xx < x + b)
            if k % 2 == 0 and a > 6 and b > 6:                     # every other large one is an ellipse
                box &= ((yy - (y + a / 2 - .5)) / (a / 2)) ** 2 + ((xx - (x + b / 2 - .5)) / (b / 2)) ** 2 <= 1
            masks.append(box)
        out.append((img, np.asarray(masks, np.uint8)))
    return out


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def run(samples, phase, seed, out, tag):
    draws, shapes = _Draws(), []
    rtransforms.random = draws
    if phase == "train":                                             # train.py:77-83
        ts = [rtransforms.ConvertImgFloat(), rtransforms.PhotometricDistort(), rtransforms.Expand(max_scale=2, mean=(0, 0, 0)),
              rtransforms.RandomMirror_w(), rtransforms.RandomMirror_h(), rtransforms.Resize(H, W)]
    else:                                                            # train.py:84-85
        ts = [rtransforms.ConvertImgFloat(), rtransforms.Resize(H, W)]
    ds = _Memory(samples, rtransforms.Compose([_Shapes(t, shapes) for t in ts]))
    np.random.seed(seed)
    items, marks = [], []
    for k in range(len(samples)):
        marks.append((len(draws.log), len(shapes)))
        items.append(ds[k])
    marks.append((len(draws.log), len(shapes)))
    batch = rcollater.collater(items)
    img, gts, gt_masks, gt_bboxes = batch[0].numpy(), [g.numpy() for g in batch[1:5]], batch[5], batch[6]
    assert img.dtype == np.float32 and img.shape == (len(samples), 3, H, W)
    for k in range(len(samples)):
        p = f"{tag}.s{k}."
        log = draws.log[marks[k][0]:marks[k + 1][0]]
        out[p + "draw_kind"] = np.array([d[0] for d in log], np.int8)
        out[p + "draw_val"] = np.array([d[1] for d in log], np.float64)
        out[p + "shapes"] = np.array(shapes[marks[k][1]:marks[k + 1][1]], np.int32).reshape(-1, 2)
        for l in range(4):
            out[p + f"bboxes{l}"] = np.asarray(ds.boxes[4 * k + l], np.float32).reshape(-1, 5, 2)
            out[p + f"gt{l}_sha"] = sha(gts[l][k])
        out[p + "img_sha"] = sha(img[k])
        gm = np.asarray(gt_masks[k], np.float32).reshape(-1, H, W)
        assert np.isin(gm, (0., 1.)).all()
        out[p + "gt_masks"] = gm.astype(np.uint8)
        out[p + "gt_bboxes"] = np.asarray(gt_bboxes[k], np.float32).reshape(-1, 5)
        if phase == "val" or seed in SEEDS[:FULL]:
            out[p + "img"] = img[k]
            for l in range(4):
                out[p + f"gt{l}"] = gts[l][k]


def main():
    samples = sources()
    out = {"hw": np.array([H, W], np.int32), "seeds": np.array(SEEDS, np.int64)}
    for k, (img, masks) in enumerate(samples):
        out[f"src{k}.img"], out[f"src{k}.masks"] = img, masks
    for t, seed in enumerate(SEEDS):
        run(samples, "train", seed, out, f"t{t}")
    run(samples, "val", 0, out, "val")
    path = os.path.join(ROOT, "tests", "golden", "sampleprep.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
