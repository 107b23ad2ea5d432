"""Shapes the split tests share (tests/test_split_cpu.py, tests/test_gpu_split.py): dumbbells, discs, a serpentine, ragged blobs, and the
plain-Python breadth-first search that states the regrow rule pixel by pixel."""
from collections import deque

import numpy as np

# (r, gap, d) -> the two parts under connectivity 4 and 8 (None: two seeds, areas not pinned)
DUMBBELLS = {(4, 7, 3): ((48, 48), (50, 46)), (6, 10, 4): ((112, 105), None), (8, 14, 5): ((196, 189), (196, 189)),
             (10, 17, 7): ((307, 307), (317, 297)), (12, 20, 8): ((431, 418), (433, 416))}
ONE_SEED = [(6, 9, 4), (8, 13, 5), (10, 16, 6)]


def disc(H, W, cy, cx, r):
    yy, xx = np.mgrid[0:H, 0:W]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r


def dumbbell(r, gap):
    """(2r + 5) x (2r + gap + 5): two discs of radius r around (r + 2, r + 2) and (r + 2, r + 2 + gap), as an int32 map of id 1"""
    H, W = 2 * r + 5, 2 * r + gap + 5
    return (disc(H, W, r + 2, r + 2, r) | disc(H, W, r + 2, r + 2 + gap, r)).astype(np.int32)


def three_discs():
    return (disc(40, 40, 8, 8, 6) | disc(40, 40, 8, 18, 6) | disc(40, 40, 18, 8, 6)).astype(np.int32)


def large_pair():
    """170 x 170: two discs of radius 30 joined by a 4-connected staircase, in a box of 141 x 141 that does not fit the device route"""
    lab = (disc(170, 170, 40, 40, 30) | disc(170, 170, 120, 120, 30)).astype(np.int32)
    lab[55:106, 55:107][np.eye(51, 52, dtype=bool) | np.eye(51, 52, k=1, dtype=bool)] = 1
    return lab


def serpentine(n=63):
    """n x n (n = 4k + 3): a one-pixel path that fills the even rows and joins them at alternating ends, and its two end pixels"""
    lab = np.zeros((n, n), np.int32)
    lab[0::2] = 1
    lab[1::4, n - 1] = 1
    lab[3::4, 0] = 1
    return lab, (0, 0), (n - 1, n - 1 if (n // 2) % 2 == 0 else 0)


def dumbbell_sheet(reps=2, transpose=True):
    """Every dumbbell of DUMBBELLS `reps` times (and its transpose), each under an id of its own, on one map with a margin that keeps the
    cores of d <= 8 apart from the neighbours -> (map int32, n, [(id, (r, gap, d), transposed)])"""
    tiles, meta = [], []
    for rep in range(reps):
        for key in DUMBBELLS:
            for tr in ((False, True) if transpose else (False,)):
                m = dumbbell(key[0], key[1])
                tiles.append(m.T if tr else m)
                meta.append((len(tiles), key, tr))
    side = max(max(t.shape) for t in tiles) + 2
    cols = int(np.ceil(np.sqrt(len(tiles))))
    rows = -(-len(tiles) // cols)
    lab = np.zeros((rows * side + 3, cols * side + 1), np.int32)
    for k, t in enumerate(tiles):
        y, x = (k // cols) * side + 1, (k % cols) * side + 1
        lab[y:y + t.shape[0], x:x + t.shape[1]] = t * (k + 1)
    return lab, len(tiles), meta


def blobs(H, W, n, seed, r_lo=3, r_hi=9):
    """A ragged multi-instance map: instance k is the union of two or three discs, later ids never overwrite earlier ones"""
    rng = np.random.default_rng(seed)
    lab = np.zeros((H, W), np.int32)
    for k in range(1, n + 1):
        cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
        for _ in range(int(rng.integers(2, 4))):
            r = int(rng.integers(r_lo, r_hi + 1))
            oy, ox = cy + int(rng.integers(-2 * r, 2 * r + 1)), cx + int(rng.integers(-2 * r, 2 * r + 1))
            lab[disc(H, W, oy, ox, r) & (lab == 0)] = k
    return lab


def random_seed_map(lab, count, seed, top):
    """`count` random one-pixel seeds with ranks drawn from 1 .. top, anywhere on the map (also off the instances)"""
    rng = np.random.default_rng(seed)
    s = np.zeros(lab.shape, np.int32)
    ys, xs = rng.integers(0, lab.shape[0], count), rng.integers(0, lab.shape[1], count)
    s[ys, xs] = rng.integers(1, top + 1, count)
    return s


NB4 = ((-1, 0), (0, -1), (0, 1), (1, 0))
NB8 = NB4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))


def bfs_plain(P, rank, conn):
    """The regrow rule pixel by pixel, in plain Python: per seed a deque breadth-first search inside P, then per pixel the smallest
    (distance, rank) -> (assign [h, w], 0 where no seed reaches; g: {rank: distance map, -1 = no path})"""
    P = np.asarray(P, bool)
    h, w = P.shape
    nb = NB8 if conn == 8 else NB4
    g = {}
    for s in sorted(set(np.asarray(rank)[P & (np.asarray(rank) > 0)].tolist())):
        d = np.full((h, w), -1, np.int64)
        q = deque()
        for y, x in zip(*np.nonzero(P & (np.asarray(rank) == s))):
            d[y, x] = 0
            q.append((int(y), int(x)))
        while q:
            y, x = q.popleft()
            for dy, dx in nb:
                yy, xx = y + dy, x + dx
                if 0 <= yy < h and 0 <= xx < w and P[yy, xx] and d[yy, xx] < 0:
                    d[yy, xx] = d[y, x] + 1
                    q.append((yy, xx))
        g[s] = d
    assign = np.zeros((h, w), np.int64)
    for y in range(h):
        for x in range(w):
            if P[y, x]:
                best = min(((int(d[y, x]), s) for s, d in g.items() if d[y, x] >= 0), default=None)
                assign[y, x] = 0 if best is None else best[1]
    return assign, g
