"""Per-instance texture: the grey-level co-occurrence matrices of every instance of a label map and Haralick's features, without copying
the map back.

measure.py says how large and how bright an instance is, intensity.py how its intensities are distributed; neither says what it looks
like inside.  Texture -- CellProfiler's MeasureTexture, mahotas' haralick, skimage's graycomatrix / graycoprops -- is a function of PAIRS
of pixels, so it is no function of measure's sums or of intensity's bins.  The device counts the pairs into four LDS matrices per job
(kg_label_glcm, csrc/texture.hip), 4 L^2 integers per job come back, and the host derives the floats in float64.

    glcm_host                 the semantics in NumPy: shifted comparisons per job and direction (the CPU route, the yardstick of the GPU tests)
    glcm_rows_host            the same for the raw ten-column jobs
    glcm_rows                 kg_label_glcm as it is: ONE launch, everything stays on the device
    glcm                      glcm_host on the device -> CoMatrices
    texture_instances         glcm for an Instances / TiledInstances
    texture_instances_batch   the same for predict_instances' list, one launch per output size
    CoMatrices                counts int64 [m, C, D, 4, L, L]; pairs / symmetric / haralick / props, shared by both routes
    fits                      the route rule of the kernel

Semantics (include/kgnet_hip.h is the normative text)
  job         {img, id, y1, x1, y2, x2, channel, distance, lo, span}: a half-open box, clamped to the map.  P = the pixels of the box in
              image img with labels == id.  Labels are compared only: 0, -1, INT_MIN and INT_MAX are ordinary ids.
  image       uint8 or uint16 [nimg, H, W, C] ([H, W, C] for one map), 1 <= C <= 4.  H, W <= 32768, nimg * H * W <= 2^31 - 1.
  level       u = max(v - lo, 0), lev = min(u * L // span, L - 1), 2 <= L <= 32.  uint8 with lo = 0, span = 256, L = 16 is v >> 4.
  directions  k = 0 .. 3 with offsets (dy, dx) = (0, d), (d, d), (d, 0), (d, -d), 1 <= d <= 32.  G[k][i][j] = the number of pixels p of P
              such that p + o_k lies inside the map, carries the id, lev(p) = i and lev(p + o_k) = j.  The partner is read from the MAP,
              not from the box: the matrices of disjoint pieces of a box add up exactly.
  row         int [4, L, L].  A bad job -- an image index outside [0, nimg), an empty or inverted box, a channel outside [0, C), a distance
              outside 1 .. 32, span <= 0 -- gets zeros.
  range       how lo and span are chosen: None = the full range of the element type (0, 256 or 65536); (lo, hi) = lo, hi - lo + 1; a list
              of such pairs, one per selected channel; "object" = per job and channel the min and max of measure.py over the job's pixels.
  large jobs  a job whose clamped box holds more than max_job_pixels pixels is cut into bands (labelmetrics.split_jobs); the pieces go
              through the same launch and their matrices are added on the host."""
import numpy as np

from . import _lib, _labelmaps, labelmetrics, measure
from ._labelmaps import check_cap, device_args, host_args, instance_stats, is_device, job_rows, job_table
from .labelmetrics import split_jobs

KGLibraryError = _lib.KGLibraryError
MIN_LEVELS, MAX_LEVELS = 2, 32
MAX_DISTANCE = 32
STAGE_CELLS = 16384
OFFSETS = ((0, 1), (1, 1), (1, 0), (1, -1))                             # (dy, dx) of direction k, times the distance
_JOB_COLUMNS = "(img, id, y1, x1, y2, x2, channel, distance, lo, span)"
FEATURES = ("asm", "contrast", "correlation", "variance", "idm", "sum_average", "sum_variance", "sum_entropy", "entropy",
            "difference_variance", "difference_entropy", "imc1", "imc2")


def fits(h, w, d):
    """True when a clamped box of h x w pixels at distance d takes the kernel's staged route: (h + d) * (w + 2 d) <= 16384."""
    return (int(h) + int(d)) * (int(w) + 2 * int(d)) <= STAGE_CELLS


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------

def _levels(fn, levels):
    if isinstance(levels, (bool, np.bool_)) or not isinstance(levels, (int, np.integer)) or not MIN_LEVELS <= levels <= MAX_LEVELS:
        raise KGLibraryError(f"{fn}: levels {levels!r} ({MIN_LEVELS} .. {MAX_LEVELS})")
    return int(levels)


def _distances(fn, distance):
    ds = [distance] if np.ndim(distance) == 0 else list(distance)
    if not ds or any(isinstance(d, (bool, np.bool_)) or not isinstance(d, (int, np.integer)) or not 1 <= d <= MAX_DISTANCE for d in ds):
        raise KGLibraryError(f"{fn}: distance {distance!r} (an integer in 1 .. {MAX_DISTANCE}, or a sequence of them)")
    return tuple(int(d) for d in ds)


def _channels(fn, channels, C):
    if channels is None:
        return tuple(np.arange(C).tolist())
    cs = [channels] if np.ndim(channels) == 0 else list(channels)
    if not cs or any(isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, np.integer)) or not 0 <= c < C for c in cs):
        raise KGLibraryError(f"{fn}: channels {channels!r} (indices into the image's {C} channel(s))")
    return tuple(int(c) for c in cs)


def _lo_span(fn, rng, chans, elem_bytes, m, minmax):
    """-> (lo, span) int64 [m, len(chans)].  minmax: a function -> (min, max) integers [m, C] over the image's channels ("object")."""
    nc = len(chans)
    if rng is None:
        return np.zeros((m, nc), np.int64), np.full((m, nc), 256 if elem_bytes == 1 else 65536, np.int64)
    if isinstance(rng, str):
        if rng != "object":
            raise KGLibraryError(f"{fn}: range {rng!r} (None, (lo, hi), a list of pairs per channel, or \"object\")")
        if m == 0:
            return np.zeros((0, nc), np.int64), np.ones((0, nc), np.int64)
        mn, mx = minmax()
        mn, mx = np.asarray(mn, np.int64).reshape(m, -1)[:, list(chans)], np.asarray(mx, np.int64).reshape(m, -1)[:, list(chans)]
        return mn, mx - mn + 1
    r = np.asarray(rng)
    if r.dtype.kind not in "iu" or r.shape not in ((2,), (nc, 2)):
        raise KGLibraryError(f"{fn}: range must be integers (lo, hi) or one such pair per selected channel ({nc}), not {rng!r}")
    r = np.broadcast_to(r.astype(np.int64).reshape(-1, 2), (nc, 2))
    if (r[:, 1] < r[:, 0]).any() or r.min() < -2 ** 31 or (r[:, 1] - r[:, 0] + 1).max() > 2 ** 31 - 1:
        raise KGLibraryError(f"{fn}: range {rng!r}: lo <= hi, both inside int32")
    return np.broadcast_to(r[None, :, 0], (m, nc)).copy(), np.broadcast_to((r[:, 1] - r[:, 0] + 1)[None], (m, nc)).copy()


def texture_jobs(pieces, chans, ds, lo, span, owner=None):
    """pieces [mp, 6], the selected channels, the distances, lo / span [m, len(chans)] of the OWNING jobs (owner [mp]; None: piece k is job
    k) -> int64 [mp * len(chans) * len(ds), 10], piece-major, then channel, then distance."""
    p = np.asarray(pieces, np.int64).reshape(-1, 6)
    mp, nc, nd = len(p), len(chans), len(ds)
    own = np.arange(mp) if owner is None else np.asarray(owner, np.int64)
    out = np.empty((mp, nc, nd, 10), np.int64)
    out[..., :6] = p[:, None, None, :]
    out[..., 6] = np.asarray(chans, np.int64)[None, :, None]
    out[..., 7] = np.asarray(ds, np.int64)[None, None, :]
    out[..., 8] = np.asarray(lo, np.int64).reshape(-1, nc)[own][:, :, None]
    out[..., 9] = np.asarray(span, np.int64).reshape(-1, nc)[own][:, :, None]
    return out.reshape(-1, 10)


# ---- the derived quantities -----------------------------------------------------------------------------------------------------------

def _plogp(p):
    """p log2 p, 0 where p == 0"""
    pos = p > 0
    return np.where(pos, p * np.log2(np.where(pos, p, 1.0)), 0.0)


class CoMatrices:
    """counts = host int64 [m, C, D, 4, L, L]: per job (or instance), selected channel, distance and direction the co-occurrence matrix
    G[i][j]; distances = the D distances; channels = the C selected channel indices.  Everything else is derived here, in float64, from
    those integers only."""
    __slots__ = ("counts", "distances", "channels")

    def __init__(self, counts, distances=None, channels=None):
        c = np.ascontiguousarray(counts, np.int64)
        if c.ndim != 6 or c.shape[3] != 4 or c.shape[4] != c.shape[5] or not MIN_LEVELS <= c.shape[5] <= MAX_LEVELS:
            raise KGLibraryError(f"CoMatrices: counts must be integers [m, C, D, 4, L, L] with {MIN_LEVELS} <= L <= {MAX_LEVELS}, not {c.shape}")
        self.counts = c
        self.distances = tuple(np.arange(1, c.shape[2] + 1).tolist()) if distances is None else tuple(int(d) for d in distances)
        self.channels = tuple(np.arange(c.shape[1]).tolist()) if channels is None else tuple(int(v) for v in channels)
        if len(self.distances) != c.shape[2] or len(self.channels) != c.shape[1]:
            raise KGLibraryError(f"CoMatrices: {len(self.distances)} distances and {len(self.channels)} channels for counts of {c.shape}")

    def __len__(self):
        return len(self.counts)

    @property
    def levels(self):
        return self.counts.shape[5]

    def pairs(self):
        """int64 [m, C, D, 4]: the pairs counted, sum_ij G[i][j]"""
        return self.counts.sum((-1, -2))

    def symmetric(self):
        """int64 [m, C, D, 4, L, L]: G + G^T, the matrix of the offset and its opposite over the whole object"""
        return self.counts + np.swapaxes(self.counts, -1, -2)

    def haralick(self):
        """float64 [m, C, D, 4, 13]: Haralick's f1 .. f13 (FEATURES) of the symmetric matrix normalised to a probability,
        p(i, j) = S[i][j] / sum S with S = G + G^T.  Levels i, j are numbered from 0, logarithms are base 2, and a term with probability
        0 contributes 0.  With px(i) = sum_j p(i, j) (= py, the matrix is symmetric), mu = sum_i i px(i), var = sum_i (i - mu)^2 px(i),
        p+(k) = sum_{i + j = k} p(i, j) for k = 0 .. 2 L - 2 and p-(k) = sum_{|i - j| = k} p(i, j) for k = 0 .. L - 1:

          f1  asm                  sum_ij p(i, j)^2
          f2  contrast             sum_ij (i - j)^2 p(i, j)
          f3  correlation          sum_ij (i - mu) (j - mu) p(i, j) / var; 1 when var == 0
          f4  variance             sum_ij (i - mu)^2 p(i, j)                        (= var)
          f5  idm                  sum_ij p(i, j) / (1 + (i - j)^2)
          f6  sum_average          sum_k k p+(k)
          f7  sum_variance         sum_k (k - f6)^2 p+(k)                           (about the sum average, not Haralick's misprinted f8)
          f8  sum_entropy          - sum_k p+(k) log2 p+(k)
          f9  entropy              HXY = - sum_ij p(i, j) log2 p(i, j)
          f10 difference_variance  sum_k (k - m)^2 p-(k) with m = sum_k k p-(k)
          f11 difference_entropy   - sum_k p-(k) log2 p-(k)
          f12 imc1                 (HXY - HXY1) / max(HX, HY) with HX = HY = - sum_i px(i) log2 px(i) and
                                   HXY1 = - sum_ij p(i, j) log2(px(i) py(j)); 0 when max(HX, HY) == 0
          f13 imc2                 sqrt(max(0, 1 - exp(-2 (HXY2 - HXY)))) with HXY2 = - sum_ij px(i) py(j) log2(px(i) py(j))

        A matrix without pairs gives NaN in all thirteen.  These are this project's definitions (f3's and f12's degenerate cases as
        mahotas has them)."""
        S = self.symmetric().astype(np.float64)
        L = self.levels
        tot = S.sum((-1, -2))
        live = tot > 0
        p = S / np.where(live, tot, 1.0)[..., None, None]
        lv = np.arange(L, dtype=np.float64)
        i, j = lv[:, None], lv[None, :]
        ii, jj = np.arange(L)[:, None], np.arange(L)[None, :]
        flat = p.reshape(p.shape[:-2] + (L * L,))
        to_sum = np.zeros((L * L, 2 * L - 1)); to_sum[np.arange(L * L), (ii + jj).reshape(-1)] = 1.0
        to_dif = np.zeros((L * L, L)); to_dif[np.arange(L * L), np.abs(ii - jj).reshape(-1)] = 1.0
        ps, pd = flat @ to_sum, flat @ to_dif                          # products with 0.0 and 1.0: only the additions round
        ks, kd = np.arange(2 * L - 1, dtype=np.float64), lv
        px = p.sum(-1)
        mu = (px * lv).sum(-1)
        ci, cj = i - mu[..., None, None], j - mu[..., None, None]
        var = (ci * ci * p).sum((-1, -2))
        out = np.empty(p.shape[:-2] + (13,), np.float64)
        out[..., 0] = (p * p).sum((-1, -2))
        out[..., 1] = ((i - j) ** 2 * p).sum((-1, -2))
        out[..., 2] = np.where(var > 0, (ci * cj * p).sum((-1, -2)) / np.where(var > 0, var, 1.0), 1.0)
        out[..., 3] = var
        out[..., 4] = (p / (1.0 + (i - j) ** 2)).sum((-1, -2))
        f6 = (ks * ps).sum(-1)
        out[..., 5] = f6
        out[..., 6] = ((ks - f6[..., None]) ** 2 * ps).sum(-1)
        out[..., 7] = -_plogp(ps).sum(-1)
        hxy = -_plogp(p).sum((-1, -2))
        out[..., 8] = hxy
        md = (kd * pd).sum(-1)
        out[..., 9] = ((kd - md[..., None]) ** 2 * pd).sum(-1)
        out[..., 10] = -_plogp(pd).sum(-1)
        hx = -_plogp(px).sum(-1)
        lpx = np.log2(np.where(px > 0, px, 1.0))
        lxy = lpx[..., :, None] + lpx[..., None, :]                    # log2(px(i) py(j)) wherever both are positive
        hxy1 = -(p * lxy).sum((-1, -2))
        hxy2 = -(px[..., :, None] * px[..., None, :] * lxy).sum((-1, -2))
        out[..., 11] = np.where(hx > 0, (hxy - hxy1) / np.where(hx > 0, hx, 1.0), 0.0)
        out[..., 12] = np.sqrt(np.maximum(0.0, 1.0 - np.exp(-2.0 * (hxy2 - hxy))))
        out[~live] = np.nan
        return out

    def props(self):
        """dict: pairs int64 [m, C, D, 4]; every name of FEATURES float64 [m, C, D], the feature averaged over the four directions, NaN
        where a direction has no pairs."""
        h = self.haralick()
        out = {"pairs": self.pairs()}
        for k, name in enumerate(FEATURES):
            out[name] = h[..., k].mean(-1)
        return out


# ---- host statement of the semantics ----------------------------------------------------------------------------------------------------

def levels_of(values, lo, span, levels):
    """The level rule on an integer array: min(max(v - lo, 0) * L // span, L - 1) in 64-bit integers (span > 0)."""
    u = np.maximum(np.asarray(values).astype(np.int64) - int(lo), 0)
    return np.minimum(u * int(levels) // int(span), int(levels) - 1)


def _rows_host(maps, img, jobs, L):
    nimg, H, W = maps.shape
    C = img.shape[3]
    out = np.zeros((len(jobs), 4, L, L), np.int64)
    for a, (i, v, y1, x1, y2, x2, ch, d, lo, span) in enumerate(np.asarray(jobs, np.int64).reshape(-1, 10).tolist()):
        y1, x1, y2, x2 = max(y1, 0), max(x1, 0), min(y2, H), min(x2, W)
        if not 0 <= i < nimg or y2 <= y1 or x2 <= x1 or not 0 <= ch < C or not 1 <= d <= MAX_DISTANCE or span <= 0:
            continue
        wy2, wx1, wx2 = min(y2 + d, H), max(x1 - d, 0), min(x2 + d, W)  # the window the pairs of the box can reach
        me = maps[i, y1:wy2, wx1:wx2] == v
        lev = levels_of(img[i, y1:wy2, wx1:wx2, ch], lo, span, L)
        for k, (oy, ox) in enumerate(OFFSETS):
            dy, dx = oy * d, ox * d
            # the centres of the box whose partner lies inside the map, in map coordinates
            ya, yb, xa, xb = y1, min(y2, H - dy), max(x1, -dx), min(x2, W - dx)
            if yb <= ya or xb <= xa:
                continue
            cen = (slice(ya - y1, yb - y1), slice(xa - wx1, xb - wx1))
            par = (slice(ya + dy - y1, yb + dy - y1), slice(xa + dx - wx1, xb + dx - wx1))
            both = me[cen] & me[par]
            out[a, k] = np.bincount(lev[cen][both] * L + lev[par][both], minlength=L * L).reshape(L, L)
    return out


def glcm_rows_host(labels, jobs, image, levels=16):
    """labels: integers [H, W] or [nimg, H, W]; jobs: integers [m, 10] = (img, id, y1, x1, y2, x2, channel, distance, lo, span); image:
    uint8 / uint16 [H, W, C] / [nimg, H, W, C] -> int64 [m, 4, L, L].  From the definition: per job and direction the box and the box
    shifted by the offset are compared and their levels counted.  Nothing split."""
    maps, img = host_args("glcm_rows_host", labels, image)
    j = _labelmaps.host_jobs("glcm_rows_host", jobs, 10, _JOB_COLUMNS).astype(np.int64)
    return _rows_host(maps, img, j, _levels("glcm_rows_host", levels))


def _assemble(rows, owner, m, nc, nd, L):
    """piece rows [mp * nc * nd, 4, L, L] -> counts int64 [m, nc, nd, 4, L, L], the pieces of a job added.  owner is split_jobs': sorted,
    and every job has at least one piece -- so mp == m means one piece per job, and the rows are the counts."""
    owner = np.asarray(owner, np.int64)
    r = np.asarray(rows).reshape(len(owner), nc, nd, 4, L, L)
    if len(owner) == m:
        return r.astype(np.int64)
    counts = np.zeros((m, nc, nd, 4, L, L), np.int64)
    one = np.bincount(owner, minlength=m)[owner] == 1
    counts[owner[one]] = r[one]
    np.add.at(counts, owner[~one], r[~one].astype(np.int64))
    return counts


def glcm_host(labels, jobs_or_n, image, levels=16, distance=1, channels=None, range=None):
    """labels: integers [H, W] or [nimg, H, W]; jobs_or_n: jobs [m, 6] = (img, id, y1, x1, y2, x2), or the instance count n (one per map
    for a stack): the ids 1 .. n inside their own boxes (labelmetrics.label_stats_host); image: uint8 / uint16 [H, W, C] /
    [nimg, H, W, C]; levels: L in 2 .. 32; distance: an integer in 1 .. 32 or a sequence of them; channels: None (all) or channel
    indices; range: None, (lo, hi), a list of such pairs per selected channel, or "object" (measure_host's min and max per job and
    channel) -> CoMatrices.  Nothing split."""
    fn = "glcm_host"
    maps, img = host_args(fn, labels, image)
    L, ds, chans = _levels(fn, levels), _distances(fn, distance), _channels(fn, channels, img.shape[3])
    j = _labelmaps.host_job_table(fn, maps, jobs_or_n, labelmetrics.label_stats_host)

    def minmax():
        raw = measure.measure_host(maps, j, img)
        return raw[:, 12::4], raw[:, 13::4]
    lo, span = _lo_span(fn, range, chans, img.dtype.itemsize, len(j), minmax)
    rows = _rows_host(maps, img, texture_jobs(j, chans, ds, lo, span), L)
    return CoMatrices(_assemble(rows, np.arange(len(j)), len(j), len(chans), len(ds), L), ds, chans)


# ---- device -----------------------------------------------------------------------------------------------------------------------------

def glcm_rows(labels, jobs, image, levels=16):
    """kg_label_glcm as it is: labels device int32 [H, W] or [nimg, H, W]; jobs host integers [m, 10] (uploaded once) or a device int32
    tensor; image a host array (uploaded once) or a device tensor -> device int32 [m, 4, L, L].  One launch, no copy back, no
    synchronisation, nothing split."""
    lab, img = device_args("glcm_rows", labels, image)
    L = _levels("glcm_rows", levels)
    jd = _labelmaps.device_jobs("glcm_rows", jobs, 10, _JOB_COLUMNS, lab.device)
    return job_rows("kg_label_glcm", lab, img, jd, (L,), (4, L, L))


def _device_glcm(fn, lab, img, j, L, ds, chans, rng, max_job_pixels, minmax=None):
    """lab, img: device tensors; j: clamped host jobs [m, 6]; minmax: None, or (min, max) [m, C] already known -> CoMatrices"""
    cap = check_cap(fn, max_job_pixels)

    def measured():
        if minmax is not None:
            return minmax
        raw = measure.measure(lab, jobs=j, image=img, max_job_pixels=cap).raw
        return raw[:, 12::4], raw[:, 13::4]
    lo, span = _lo_span(fn, rng, chans, img.element_size(), len(j), measured)
    pieces, owner = split_jobs(j, cap)
    rows = glcm_rows(lab, texture_jobs(pieces, chans, ds, lo, span, owner), img, L).cpu().numpy()
    return CoMatrices(_assemble(rows, owner, len(j), len(chans), len(ds), L), ds, chans)


def glcm(labels, n=None, jobs=None, image=None, levels=16, distance=1, channels=None, range=None, stats=None, max_job_pixels=65536):
    """glcm_host on the device -> CoMatrices (host).  labels: device int32 [H, W] or [nimg, H, W].  What is taken:
      jobs   integers [m, 6] = (img, id, y1, x1, y2, x2), a host array or a device tensor (copied back: the band rule runs on the host); or
      n      the instance count (one per map for a stack): the ids 1 .. n inside their own boxes.  The boxes come from stats -- host
             integers [n, 5] = (area, y1, x1, y2, x2), one array per map for a stack -- or, without stats, from labelmetrics.label_stats.
    image: a host uint8 / uint16 array [H, W, C] / [nimg, H, W, C] (uploaded once) or a device tensor; levels, distance, channels, range
    as glcm_host: every (job, channel, distance) is one kernel job, so a sequence of distances gives more jobs and still ONE
    kg_label_glcm launch, one upload (the jobs) and one copy back (4 L^2 integers per kernel job).  range="object" measures first
    (measure.measure: one more launch and copy back).  A job above max_job_pixels pixels is cut into row bands (labelmetrics.split_jobs)
    whose pieces go through the same launch and are added on the host."""
    import torch
    fn = "glcm"
    lab, img = device_args(fn, labels, image)
    L, ds, chans = _levels(fn, levels), _distances(fn, distance), _channels(fn, channels, img.shape[3])
    if torch.is_tensor(jobs):
        jobs = jobs.cpu().numpy()
    return _device_glcm(fn, lab, img, job_table(fn, lab, n, jobs, stats, labelmetrics.label_stats), L, ds, chans, range, max_job_pixels)


# ---- Instances ----------------------------------------------------------------------------------------------------------------------------

def _known_minmax(inst, C):
    """(min, max) [n, C] from measurements that carry the intensity columns of a C-channel image, else None"""
    ms = getattr(inst, "measurements", None)
    if ms is None or ms.channels != C or len(ms) != len(inst):
        return None
    return ms.raw[:, 12::4], ms.raw[:, 13::4]


def texture_instances(inst, image, levels=16, distance=1, channels=None, range=None, max_job_pixels=65536):
    """glcm for an Instances / TiledInstances -> CoMatrices with len(inst) rows: ids 1 .. n, boxes from table[:, 2:6]; an instance with no
    visible pixel gets zeros (NaN once derived).  image: uint8 / uint16 [H, W, C] at the label map's size (host array or device tensor).
    range="object" takes the min and max from inst.measurements when they carry the image's intensity columns, and measures otherwise.
    A host label map (assemble_host's result) goes through glcm_host."""
    fn = "texture_instances"
    stats = instance_stats(fn, inst)
    if is_device(inst.labels):
        lab, img = device_args(fn, inst.labels, image)
        L, ds, chans = _levels(fn, levels), _distances(fn, distance), _channels(fn, channels, img.shape[3])
        j = job_table(fn, lab, len(inst), None, stats, None)
        return _device_glcm(fn, lab, img, j, L, ds, chans, range, max_job_pixels, _known_minmax(inst, img.shape[3]))
    return glcm_host(_labelmaps.host_labels(inst), measure.jobs_from_stats(stats), _labelmaps.host_pixels(image), levels, distance, channels, range)


def texture_instances_batch(insts, images, levels=16, distance=1, channels=None, range=None, max_job_pixels=65536):
    """texture_instances for predict_instances' list (entries may be None), in place: every entry's `texture` is set.  ONE kg_label_glcm
    launch for all images of one output size.  images: uint8 / uint16 [N, h, w, C] (host array or device tensor), one image per entry,
    at the label maps' size."""
    fn = "texture_instances_batch"
    if images is None or len(images) != len(insts):
        raise KGLibraryError(f"texture: {0 if images is None else len(images)} images for {len(insts)} entries")
    for idx, stack, _, _ in _labelmaps.size_batches(fn, insts):
        lab, img = device_args(fn, stack, images[idx] if len(idx) != len(insts) else images)
        L, ds, chans = _levels(fn, levels), _distances(fn, distance), _channels(fn, channels, img.shape[3])
        j = job_table(fn, lab, [len(insts[i]) for i in idx], None, [instance_stats(fn, insts[i]) for i in idx], None)
        known = [_known_minmax(insts[i], img.shape[3]) for i in idx]
        minmax = None if any(k is None for k in known) else (np.concatenate([k[0] for k in known]), np.concatenate([k[1] for k in known]))
        got = _device_glcm(fn, lab, img, j, L, ds, chans, range, max_job_pixels, minmax)
        for i, a, b in _labelmaps.deal(insts, idx):
            insts[i].texture = CoMatrices(got.counts[a:b], ds, chans)
    return insts
