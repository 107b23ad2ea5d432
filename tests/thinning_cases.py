"""Shapes and plain-Python statements the thinning tests share (tests/test_thinning_cpu.py, tests/test_gpu_thinning.py): the deletion rule
and the row counts pixel by pixel, discs, rings, combs, a checkerboard, and the pinned example of include/kgnet_hip.h."""
import numpy as np

# (dy, dx) of P2 .. P9: clockwise from north, y growing downward
RING = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))


def _nb(m, y, x):
    h, w = m.shape
    return [bool(m[y + dy, x + dx]) if 0 <= y + dy < h and 0 <= x + dx < w else False for dy, dx in RING]


def deletable_plain(m, y, x, second):
    """The rule for one pixel of a boolean array, as the header writes it"""
    if not m[y, x]:
        return False
    P2, P3, P4, P5, P6, P7, P8, P9 = _nb(m, y, x)
    C = int(not P2 and (P3 or P4)) + int(not P4 and (P5 or P6)) + int(not P6 and (P7 or P8)) + int(not P8 and (P9 or P2))
    N1 = int(P9 or P2) + int(P3 or P4) + int(P5 or P6) + int(P7 or P8)
    N2 = int(P2 or P3) + int(P4 or P5) + int(P6 or P7) + int(P8 or P9)
    mm = ((P2 or P3 or not P5) and P4) if second else ((P6 or P7 or not P9) and P8)
    return C == 1 and 2 <= min(N1, N2) <= 3 and not mm


def thin_plain(mask, max_passes=0):
    """Pass after pass of the per-pixel rule -> (S, the passes that deleted something)"""
    m = np.asarray(mask, bool).copy()
    passes = 0
    while max_passes == 0 or passes < max_passes:
        deleted = False
        for second in (False, True):
            kill = [(y, x) for y in range(m.shape[0]) for x in range(m.shape[1]) if deletable_plain(m, y, x, second)]
            for y, x in kill:
                m[y, x] = False
            deleted |= bool(kill)
        if not deleted:
            break
        passes += 1
    return m, passes


def counts_plain(S):
    """(pixels, isolated, ends, junctions, ortho, diag) of a boolean array, pixel by pixel and pair by pair"""
    S = np.asarray(S, bool)
    h, w = S.shape
    px = iso = ends = junc = ortho = diag = 0
    at = lambda y, x: 0 <= y < h and 0 <= x < w and bool(S[y, x])  # noqa: E731
    for y in range(h):
        for x in range(w):
            if not S[y, x]:
                continue
            nb = _nb(S, y, x)
            px += 1
            iso += sum(nb) == 0
            ends += sum(nb) == 1
            junc += sum((not nb[q]) and nb[(q + 1) % 8] for q in range(8)) >= 3
            ortho += at(y, x + 1) + at(y + 1, x)
            diag += (at(y + 1, x + 1) and not at(y, x + 1) and not at(y + 1, x)) + (at(y + 1, x - 1) and not at(y, x - 1) and not at(y + 1, x))
    return [px, iso, ends, junc, ortho, diag]


def all_diagonal_pairs(S):
    S = np.asarray(S, bool)
    return int((S[:-1, :-1] & S[1:, 1:]).sum() + (S[:-1, 1:] & S[1:, :-1]).sum())


def degree_sum(S):
    S = np.asarray(S, bool)
    pad = np.zeros((S.shape[0] + 2, S.shape[1] + 2), np.int64)
    pad[1:-1, 1:-1] = S
    h, w = S.shape
    deg = sum(pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy, dx in RING)
    return int(deg[S].sum())


def disc(r, pad=2):
    yy, xx = np.mgrid[-r - pad:r + pad + 1, -r - pad:r + pad + 1]
    return yy * yy + xx * xx <= r * r


def annulus(lo2=16, hi2=81, pad=2):
    r = int(np.ceil(np.sqrt(hi2)))
    yy, xx = np.mgrid[-r - pad:r + pad + 1, -r - pad:r + pad + 1]
    d = yy * yy + xx * xx
    return (d >= lo2) & (d <= hi2)


def nested_rings():
    """a ring inside a ring: two components, three background components"""
    yy, xx = np.mgrid[-30:31, -30:31]
    d = yy * yy + xx * xx
    return ((d >= 20 * 20) & (d <= 27 * 27)) | ((d >= 6 * 6) & (d <= 12 * 12))


def comb(teeth=9, tooth_h=20, tooth_w=3, gap=4, back=5):
    w = teeth * (tooth_w + gap) - gap
    m = np.zeros((back + tooth_h + 2, w + 2), bool)
    m[1:1 + back, 1:1 + w] = True
    for t in range(teeth):
        x = 1 + t * (tooth_w + gap)
        m[1 + back:1 + back + tooth_h, x:x + tooth_w] = True
    return m


def checkerboard(h=8, w=8):
    yy, xx = np.mgrid[0:h, 0:w]
    return (yy + xx) % 2 == 0


def serpentine(n=63):
    """n x n (n = 4k + 3): a one-pixel path that fills the even rows and joins them at alternating ends"""
    m = np.zeros((n, n), bool)
    m[0::2] = True
    m[1::4, n - 1] = True
    m[3::4, 0] = True
    return m


def pinned_example():
    lab = np.zeros((16, 21), np.int32)
    lab[2:5, 2:19] = 1
    lab[5:14, 9:12] = 1
    S = np.zeros((16, 21), bool)
    S[3, 3:18] = True
    S[3, 10] = False
    S[4:13, 10] = True
    return lab, S, [78, 23, 0, 3, 1, 20, 2, 2, 0]


def blobs(H, W, n, seed, r_lo=3, r_hi=9):
    """A ragged multi-instance map: instance k is the union of two or three discs, later ids never overwrite earlier ones"""
    rng = np.random.default_rng(seed)
    lab = np.zeros((H, W), np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    for k in range(1, n + 1):
        cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
        for _ in range(int(rng.integers(2, 4))):
            r = int(rng.integers(r_lo, r_hi + 1))
            oy, ox = cy + int(rng.integers(-2 * r, 2 * r + 1)), cx + int(rng.integers(-2 * r, 2 * r + 1))
            lab[((yy - oy) ** 2 + (xx - ox) ** 2 <= r * r) & (lab == 0)] = k
    return lab


def stats_of(lab, n):
    """int64 [n, 5] = (area, y1, x1, y2, x2) of the ids 1 .. n"""
    out = np.zeros((n, 5), np.int64)
    for k in range(1, n + 1):
        ys, xs = np.nonzero(lab == k)
        if len(ys):
            out[k - 1] = [len(ys), ys.min(), xs.min(), ys.max() + 1, xs.max() + 1]
    return out
