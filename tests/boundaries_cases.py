"""Shapes and plain re-statements the CPU and GPU boundary-distance tests share."""
import math

import numpy as np

I32 = np.iinfo(np.int32)
MODES = (0, 1, 2, 3)


def job(id_s, sbox, id_t, tbox, direction=0, img=0, first=0):
    """One row of the job table: {img, dir, id_s, source box, id_t, target box, first}"""
    return [img, direction, id_s, *sbox, id_t, *tbox, first]


def whole(lab):
    return (0, 0) + tuple(lab.shape[-2:])


def blob_maps(H, W, n, seed):
    """Two seeded ragged maps of one shape: ellipses and rectangles with ids 1 .. n painted over each other, some cut by the frame; the
    second is the first rolled by a few pixels with a few pixels knocked out, so that most ids meet their partner."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    a = np.zeros((H, W), np.int32)
    for i in range(1, n + 1):
        cy, cx = rng.integers(0, H), rng.integers(0, W)
        ry, rx = rng.integers(1, max(H // 4, 2) + 1), rng.integers(1, max(W // 5, 2) + 1)
        sel = (np.abs(yy - cy) <= ry) & (np.abs(xx - cx) <= rx) if i % 2 else ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
        a[sel & (rng.random((H, W)) < 0.95)] = i
    b = np.roll(a, (int(rng.integers(-3, 4)), int(rng.integers(-3, 4))), (0, 1)).copy()
    b[rng.random((H, W)) < 0.03] = 0
    return a, b


def boxes_of(lab, n):
    """int64 [n, 5] = (area, y1, x1, y2, x2) of the ids 1 .. n, by a plain loop"""
    out = np.zeros((n, 5), np.int64)
    for i in range(1, n + 1):
        ys, xs = np.nonzero(lab == i)
        if len(ys):
            out[i - 1] = [len(ys), ys.min(), xs.min(), ys.max() + 1, xs.max() + 1]
    return out


def all_pair_jobs(a, b, n, grow=0):
    """The jobs of every (i, i) pair in both directions over the ids' own boxes, grown by `grow` (the kernel clamps); ids without a pixel
    keep their empty box: a bad job"""
    sa, sb = boxes_of(a, n), boxes_of(b, n)
    g = np.array([-grow, -grow, grow, grow])
    rows = []
    for i in range(1, n + 1):
        ba, bb = sa[i - 1, 1:] + g * (sa[i - 1, 0] > 0), sb[i - 1, 1:] + g * (sb[i - 1, 0] > 0)
        rows.append(job(i, ba.tolist(), i, bb.tolist(), 0))
        rows.append(job(i, bb.tolist(), i, ba.tolist(), 1))
    return np.array(rows, np.int64)


def stripes(H, W, v=1, step=2):
    """Every `step`-th column holds v: one-pixel stripes, every pixel of v a border pixel"""
    lab = np.zeros((H, W), np.int32)
    lab[:, ::step] = v
    return lab


def thick_row(H, W, y, t, v=1):
    """Rows y .. y + t - 1 hold v; with t <= 2 every pixel of v is a border pixel, so the box of those rows is FULL of targets"""
    lab = np.zeros((H, W), np.int32)
    lab[y:y + t] = v
    return lab


def disc_in_ring(size=41, r_disc=6, r_in=12, r_out=16):
    """(a, b): a holds id 1 on a centred disc; b holds id 1 on a centred ring around it"""
    c = size // 2
    y, x = np.mgrid[0:size, 0:size]
    d2 = (y - c) ** 2 + (x - c) ** 2
    return (d2 <= r_disc ** 2).astype(np.int32), ((d2 >= r_in ** 2) & (d2 <= r_out ** 2)).astype(np.int32)


def ellipse_pair(size):
    """(a, b): id 1 on an ellipse whose box is a little over size x size, with a rectangular hole (an inner border); b is a moved by
    (6, -9) with a few one-pixel rows cut out.  Both boxes hold more than 8192 pixels from size 91 on."""
    H, W = size + 20, size + 30
    yy, xx = np.mgrid[0:H, 0:W]
    r = size / 2.0
    a = (((yy - r) / r) ** 2 + ((xx - r - 10) / r) ** 2 <= 1).astype(np.int32)
    a[size // 3:size // 3 + size // 8, size // 3:size // 3 + size // 4] = 0
    b = np.roll(a, (6, -9), (0, 1)).copy()
    b[yy % 61 == 17] = 0
    return a, b


def unsplit_d2(a, b, mode, direction):
    """The distances of id 1 between two maps, nothing split and no size rule: the plain minimum over ALL border pixels of the target,
    by broadcasting in slabs, straight from the definition"""
    src, dst = (b, a) if direction else (a, b)
    edge = lambda m: m & ~(np.pad(m, 1)[:-2, 1:-1] & np.pad(m, 1)[2:, 1:-1] & np.pad(m, 1)[1:-1, :-2] & np.pad(m, 1)[1:-1, 2:])  # noqa: E731
    ys, xs = np.nonzero(src == 1 if mode & 1 else edge(src == 1))
    yt, xt = (v.astype(np.int32) for v in np.nonzero(edge(dst == 1)))
    w = np.concatenate([((ys[k:k + 1024, None] - yt[None]) ** 2 + (xs[k:k + 1024, None] - xt[None]) ** 2).min(1) for k in range(0, len(ys), 1024)])
    if mode & 2:
        w[dst[ys, xs] == 1] = 0
    return w


# ---- plain Python re-statements -----------------------------------------------------------------------------------------------------------

def plain_border(lab, v):
    """The border pixels of v by a per-pixel loop -> a list of (y, x) in raster order"""
    H, W = lab.shape
    out = []
    for y in range(H):
        for x in range(W):
            if lab[y, x] != v:
                continue
            for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                if not (0 <= yy < H and 0 <= xx < W) or lab[yy, xx] != v:
                    out.append((y, x))
                    break
    return out


def plain_job(a, b, row, mode):
    """One job by per-pixel double loops -> (count row, list of d2)"""
    img, direction, id_s, sy1, sx1, sy2, sx2, id_t, ty1, tx1, ty2, tx2, _ = [int(v) for v in row]
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim == 2:
        a, b = a[None], b[None]
    nimg, H, W = a.shape
    sy1, sx1, sy2, sx2 = max(sy1, 0), max(sx1, 0), min(sy2, H), min(sx2, W)
    ty1, tx1, ty2, tx2 = max(ty1, 0), max(tx1, 0), min(ty2, H), min(tx2, W)
    if not 0 <= img < nimg or sy2 <= sy1 or sx2 <= sx1 or ty2 <= ty1 or tx2 <= tx1:
        return [0, 0, 0], []
    if (ty2 - ty1) * (tx2 - tx1) > 8192:
        return [0, 0, 1], []
    src, dst = (b[img], a[img]) if direction else (a[img], b[img])
    edge_s = set(plain_border(src, id_s))
    T = [(y, x) for (y, x) in plain_border(dst, id_t) if ty1 <= y < ty2 and tx1 <= x < tx2]
    out = []
    for y in range(sy1, sy2):
        for x in range(sx1, sx2):
            if src[y, x] != id_s or not (mode & 1 or (y, x) in edge_s):
                continue
            if mode & 2 and ty1 <= y < ty2 and tx1 <= x < tx2 and dst[y, x] == id_t:
                out.append(0)
            elif not T:
                out.append(-1)
            else:
                out.append(min((y - ty) ** 2 + (x - tx) ** 2 for ty, tx in T))
    return [len(out), len(T), 0], out


def plain_metrics(da, db, tolerance):
    """hausdorff, hd95, assd, nsd of one pair from the two integer lists, with math only (hd95 through np.percentile on the sorted roots)"""
    both = sorted(list(da) + list(db))
    if not both:
        return math.nan, math.nan, math.nan, math.nan
    if both[0] < 0 or not len(da) or not len(db):
        hd = math.inf
    else:
        hd = max(math.sqrt(max(da)), math.sqrt(max(db)))
    roots = sorted(math.sqrt(v) if v >= 0 else math.inf for v in both)
    with np.errstate(invalid="ignore"):
        p = float(np.percentile(np.array(roots, np.float64), 95))
    hd95 = math.inf if math.isnan(p) else p
    assd = math.fsum(roots) / len(roots)
    t2 = math.floor(tolerance * tolerance)
    nsd = sum(1 for v in both if 0 <= v <= t2) / len(both)
    return hd, hd95, assd, nsd
