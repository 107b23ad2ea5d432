"""Shapes and plain re-statements the CPU and GPU linking tests share."""
import numpy as np

I32 = np.iinfo(np.int32)

# five frames of 96 x 128; discs (cy, cx, r) with ids in listed order: a mover, a disc that dies after frame 1, a disc that divides between
# frames 1 and 2, a disc that leaves through the corner, and a disc born in frame 3
SEQUENCE_SHAPE = (96, 128)
SEQUENCE = (((20, 20, 9), (70, 100, 8), (48, 40, 9), (5, 5, 6)),
            ((21, 23, 9), (71, 102, 8), (48, 41, 9), (3, 3, 6)),
            ((22, 26, 9), (48, 34, 6), (48, 48, 6), (1, 1, 6)),
            ((23, 29, 9), (48, 32, 6), (48, 50, 6), (80, 30, 7)),
            ((24, 32, 9), (47, 30, 6), (49, 52, 6), (81, 31, 7)))


def discs(H, W, items):
    """int32 [H, W]: the discs (y - cy)^2 + (x - cx)^2 <= r^2 with ids 1, 2, ... in listed order"""
    yy, xx = np.mgrid[0:H, 0:W]
    lab = np.zeros((H, W), np.int32)
    for i, (cy, cx, r) in enumerate(items, 1):
        lab[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = i
    return lab


def sequence():
    """(stack int32 [5, 96, 128], counts)"""
    return np.stack([discs(*SEQUENCE_SHAPE, f) for f in SEQUENCE]), [len(f) for f in SEQUENCE]


def blob_map(H, W, n, seed):
    """A seeded ragged map: ellipses and rectangles with ids 1 .. n painted over each other, some cut by the frame, some touching."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    lab = np.zeros((H, W), np.int32)
    for i in range(1, n + 1):
        cy, cx = rng.integers(0, H), rng.integers(0, W)
        ry, rx = rng.integers(1, max(H // 4, 2) + 1), rng.integers(1, max(W // 6, 2) + 1)
        sel = (np.abs(yy - cy) <= ry) & (np.abs(xx - cx) <= rx) if i % 2 else ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
        lab[sel & (rng.random((H, W)) < 0.93)] = i
    return lab


def blob_pair(H=70, W=131, na=30, nb=40, seed=170):
    """Two unrelated ragged maps of one shape, with different instance counts"""
    return blob_map(H, W, na, seed), blob_map(H, W, nb, seed + 1)


def boxes_of(lab, n):
    """int64 [n, 5] = (area, y1, x1, y2, x2) of the ids 1 .. n, by a plain loop"""
    out = np.zeros((n, 5), np.int64)
    for i in range(1, n + 1):
        ys, xs = np.nonzero(lab == i)
        if len(ys):
            out[i - 1] = len(ys), ys.min(), xs.min(), ys.max() + 1, xs.max() + 1
    return out


def loop_overlaps(a, b, n, dy, dx):
    """Per id 1 .. n of a, by a per-pixel Python loop: ({value: pixels}, area, zero, outside)"""
    H, W = a.shape
    out = [[{}, 0, 0, 0] for _ in range(n)]
    for y in range(H):
        for x in range(W):
            v = int(a[y, x])
            if 1 <= v <= n:
                r = out[v - 1]
                r[1] += 1
                py, px = y + dy, x + dx
                if not (0 <= py < H and 0 <= px < W):
                    r[3] += 1
                elif b[py, px] == 0:
                    r[2] += 1
                else:
                    r[0][int(b[py, px])] = r[0].get(int(b[py, px]), 0) + 1
    return out


def as_lists(ov):
    """An Overlaps as loop_overlaps states it"""
    return [[dict(zip(*(c.tolist() for c in ov.of(k)))), int(ov.area[k]), int(ov.zero[k]), int(ov.outside[k])] for k in range(len(ov))]


def row_jobs(jobs9, resume=0, after=0):
    """[m, 9] -> the [m, 11] table of the raw entry"""
    j = np.asarray(jobs9, np.int64).reshape(-1, 9)
    return np.concatenate([j, np.full((len(j), 1), resume), np.full((len(j), 1), after)], 1)


def jobs9(stats, img_a=0, img_b=0, dy=0, dx=0):
    """stats [n, 5] -> int64 [n, 9]: the ids 1 .. n inside their own boxes"""
    s = np.asarray(stats, np.int64)
    n = len(s)
    col = lambda v: np.full((n, 1), v, np.int64)                      # noqa: E731
    return np.concatenate([col(img_a), np.arange(1, n + 1)[:, None], s[:, 1:], col(img_b), col(dy), col(dx)], 1)


def checkerboard():
    """(a, b, values): one 20 x 20 instance of id 5 in a; under it, b holds 100 distinct values in 2 x 2 cells, not in order of position,
    INT_MIN and INT_MAX among them and 5 itself too"""
    a = np.zeros((24, 26), np.int32)
    a[2:22, 3:23] = 5
    vals = (np.arange(100) * 37 % 100 + 1000).astype(np.int64)
    vals[13], vals[71], vals[40] = I32.min, I32.max, 5
    b = np.zeros((24, 26), np.int64)
    b[2:22, 3:23] = np.repeat(np.repeat(vals.reshape(10, 10), 2, 0), 2, 1)
    return a, b.astype(np.int32), vals


def link_rule(pairs, area_a, area_b, min_iou, min_child):
    """The linking rule restated over dense matrices: pairs [k, 3] = (a, b, pixels) -> (parent [n_b], children per a [n_a])"""
    na, nb = len(area_a), len(area_b)
    inter = np.zeros((na, nb), np.int64)
    for a, b, p in np.asarray(pairs).tolist():
        inter[a - 1, b - 1] = p
    iou = inter / (np.asarray(area_a)[:, None] + np.asarray(area_b)[None] - inter).astype(np.float64)
    parent = np.zeros(nb, np.int64)
    used = np.zeros(na, bool)
    cand = sorted((-iou[a, b], a, b) for a in range(na) for b in range(nb) if inter[a, b] > 0)
    for neg, a, b in cand:
        if -neg >= min_iou and not used[a] and parent[b] == 0:
            used[a], parent[b] = True, a + 1
    if min_child is not None:
        for b in range(nb):
            if parent[b] == 0 and inter[:, b].max(initial=0) > 0:
                a = int(np.argmax(inter[:, b]))                       # the first maximum: ties to the smallest a
                if inter[a, b] / float(area_b[b]) >= min_child:
                    parent[b] = a + 1
    return parent, np.bincount(parent[parent > 0] - 1, minlength=na)
