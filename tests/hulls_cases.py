"""Shapes the CPU and GPU hull tests share."""
import numpy as np

from kg_instance_segmentation_amd import polygons as pg


def disc(r):
    """int32 [2 r + 1, 2 r + 1]: the pixels whose centre lies within r of the centre pixel's"""
    y, x = np.mgrid[-r:r + 1, -r:r + 1]
    return (y * y + x * x <= r * r).astype(np.int32)


def random_mask(H, W, seed, density=0.5, empty_rows=False):
    rng = np.random.default_rng(seed)
    m = rng.random((H, W)) < density
    if empty_rows:
        m[rng.random(H) < 0.4] = False
    return m.astype(np.int32)


def whole(lab, ids=(1,), img=0):
    H, W = lab.shape[-2:]
    return np.array([[img, int(i), 0, 0, H, W] for i in ids], np.int64).reshape(-1, 6)


_DIRECTIONS = [(1, 0), (2, 1), (1, 1), (1, 2), (0, 1), (-1, 2), (-1, 1), (-2, 1), (-1, 0), (-2, -1), (-1, -1), (-1, -2), (0, -1), (1, -2), (1, -1),
               (2, -1)]                                               # (dx, dy), clockwise on the screen


def wide_polygon(seed, H=2048, W=3072):
    """A seeded convex polygon of at most 16 sides with integer vertices that nearly fills H x W -> float64 [16, 2] of (x, y), a left-out side repeating a vertex.  Its edges run along
    _DIRECTIONS with random lengths, so their digitisation keeps them whole as hull edges: edges hundreds of pixels long, whose
    c^2 d products pass 2^64."""
    rng = np.random.default_rng(seed)
    d = np.array(_DIRECTIONS, np.int64)

    def closed(k):
        k = k.copy()
        r = (k[:, None] * d).sum(0)                                    # the residual goes to the axis directions
        k[8 if r[0] > 0 else 0] += abs(r[0]); k[12 if r[1] > 0 else 4] += abs(r[1])
        v = np.cumsum(k[:, None] * d, 0)
        return v - v.min(0)
    k = rng.integers(20, 100, 16) * (rng.random(16) < 0.4)               # a few long edges: most directions are left out
    k[[0, 4]] = np.maximum(k[[0, 4]], 20)
    ext = closed(k).max(0)
    v = closed(k * int(min((W - 80) // ext[0], (H - 80) // ext[1])))
    assert v[:, 0].max() < W - 2 and v[:, 1].max() < H - 2
    return (v + 1).astype(np.float64)


def wide_shapes(seeds=(3, 4, 5), H=2048, W=3072):
    """wide_polygon of every seed, filled by polygons.fill_host -> a list of int32 [H, W] maps of 0 / 1"""
    return [pg.fill_host(pg.from_rings([[[wide_polygon(s, H, W)]]]), H, W) for s in seeds]


def wrapped_edge(ring):
    """The edge a comparison of c_a^2 d_b < c_b^2 d_a wrapped to 64 bits would choose for a ring [n, 2] of (Y, X)"""
    v = np.asarray(ring, np.int64)
    y, x = v[:, 0], v[:, 1]
    yn, xn = np.roll(y, -1), np.roll(x, -1)
    c = np.abs((xn - x)[:, None] * (y[None, :] - y[:, None]) - (yn - y)[:, None] * (x[None, :] - x[:, None])).max(1).tolist()
    d = ((yn - y) ** 2 + (xn - x) ** 2).tolist()

    def wrap(a):
        a &= 2 ** 64 - 1
        return a - 2 ** 64 if a >= 2 ** 63 else a
    k = 0
    for e in range(1, len(v)):
        if wrap(c[e] * c[e] * d[k]) < wrap(c[k] * c[k] * d[e]):
            k = e
    return k
