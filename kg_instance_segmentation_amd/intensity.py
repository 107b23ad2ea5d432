"""Per-instance intensity quantiles and histograms: the distribution of the intensity inside every instance of a label map, without
copying the map back.

measure.py gives, per instance and image channel, sum, sum of squares, min and max: mean and standard deviation.  The robust statistics --
median and quartiles (CellProfiler's MedianIntensity, LowerQuartileIntensity, UpperQuartileIntensity), a 5 % / 95 % range that ignores hot
pixels, a per-object histogram for a positivity threshold, entropy or mode -- are no function of those sums: an order statistic does not
add.  The device selects them from an LDS histogram per job (kg_label_quantiles, kg_label_histograms in csrc/intensity.hip), a few
integers per instance come back, and the host derives the floats in float64.

    quantiles_host             the semantics in NumPy: per job, sort and index (the CPU route, and the yardstick of the GPU tests)
    histograms_host            the same for the nine-column histogram jobs
    quantile_rows              kg_label_quantiles as it is: ONE launch, everything stays on the device
    histogram_rows             kg_label_histograms as it is
    quantiles                  quantiles_host on the device -> Quantiles
    histograms                 per job and channel the 256-bin histogram -> Histograms
    quantiles_instances        quantiles for an Instances / TiledInstances
    quantiles_instances_batch  the same for predict_instances' list, one launch per output size
    Quantiles                  raw int64 [n, C, 1 + 2 Q]; lower / higher / linear / median / iqr / props, shared by both routes
    Histograms                 counts int64 [n, C, 256]; totals / mode / entropy / otsu / quantile

Semantics (include/kgnet_hip.h is the normative text)
  job         {img, id, y1, x1, y2, x2}: a half-open box, clamped to the map.  P = the pixels of the box in image img with labels == id.
              Labels are compared only: 0, -1, INT_MIN and INT_MAX are ordinary ids.
  image       uint8 or uint16 [nimg, H, W, C] ([H, W, C] for one map), 1 <= C <= 4.  H, W <= 32768, nimg * H * W <= 2^31 - 1.
  quantile    a rational num / den, 0 <= num <= den <= 1 000 000; 1 <= Q <= 8 per call.  For a channel, n = |P| and v_0 <= ... <= v_(n-1)
              the sorted values of P: t = num * (n - 1), k_lo = t // den, rem = t % den, k_hi = k_lo + (rem != 0); lo = v[k_lo],
              hi = v[k_hi].
  row         int [C, 1 + 2 Q] = {n, lo_0, hi_0, ..., lo_(Q-1), hi_(Q-1)}.  A bad job -- an image index outside [0, nimg), an empty or
              inverted box, an id the box does not hold -- gets zeros.
  derived     lower = lo, higher = hi, linear = lo + (hi - lo) * rem / den (numpy's default percentile), iqr where 1/4 and 3/4 were
              asked for; n == 0 gives NaN.  Float64, from the integers only, in code both routes share.
  histogram   job {img, id, y1, x1, y2, x2, channel, shift, prefix} -> int [256].  w = value >> shift, 0 <= shift <= 8.  prefix < 0: every
              pixel of P counts into bin min(w, 255) (bin 255 is "255 and above"); prefix >= 0: only pixels with (w >> 8) == prefix
              count, into bin w & 255.  A channel outside [0, C), a shift outside [0, 8] or a bad job: a row of zeros.
  large jobs  an order statistic cannot be banded.  A job whose clamped box holds more than max_job_pixels pixels is cut into pieces
              (labelmetrics.split_jobs); ONE kg_label_histograms launch covers all pieces and channels of all such jobs; the piece
              histograms are added per job on the host, which selects.  For uint16 that histogram is of the high byte (shift 8), and one
              more launch (shift 0, prefix = the selected byte) gives the low bytes under the distinct selected bytes.  The sizes are
              known on the host, so the number of launches never depends on device data: 1 without a large job, at most 3 with one."""
from fractions import Fraction

import numpy as np

from . import _lib, _labelmaps, labelmetrics
from ._labelmaps import JOB_COLUMNS as _JOB_COLUMNS, MAX_CHANNELS, check_cap, device_args, host_args, is_device, job_rows, job_table
from .labelmetrics import split_jobs

KGLibraryError = _lib.KGLibraryError
MAX_Q = 8
MAX_DEN = 1_000_000
DEFAULT_Q = (Fraction(1, 20), Fraction(1, 4), Fraction(1, 2), Fraction(3, 4), Fraction(19, 20))
_HIST_JOB_COLUMNS = "(img, id, y1, x1, y2, x2, channel, shift, prefix)"


# ---- quantiles as rationals -------------------------------------------------------------------------------------------------------------

def as_fractions(q=None):
    """q: None (DEFAULT_Q), or a sequence of Fractions, (num, den) pairs or floats (a float becomes
    Fraction(q).limit_denominator(1 000 000)) -> a tuple of 1 .. 8 Fractions in [0, 1] with denominators <= 1 000 000."""
    if q is None:
        return DEFAULT_Q
    if isinstance(q, (Fraction, float, int)):
        q = [q]
    out = []
    for v in q:
        try:
            if isinstance(v, Fraction):
                f = v
            elif isinstance(v, (tuple, list, np.ndarray)):
                if len(v) != 2 or int(v[1]) <= 0:
                    raise ValueError
                f = Fraction(int(v[0]), int(v[1]))
            else:
                f = Fraction(float(v)).limit_denominator(MAX_DEN)
        except (ValueError, TypeError, OverflowError):
            raise KGLibraryError(f"quantiles: {v!r} is no quantile (a Fraction, a (num, den) pair or a float)") from None
        if not 0 <= f <= 1 or f.denominator > MAX_DEN:
            raise KGLibraryError(f"quantiles: {v!r} lies outside [0, 1] or has a denominator above {MAX_DEN}")
        out.append(f)
    if not 1 <= len(out) <= MAX_Q:
        raise KGLibraryError(f"quantiles: {len(out)} quantiles (1 .. {MAX_Q} per call)")
    return tuple(out)


def q_table(q):
    """-> int32 [Q, 2] rows (num, den): the table the device reads"""
    return np.array([[f.numerator, f.denominator] for f in as_fractions(q)], np.int32).reshape(-1, 2)


def ranks(n, q):
    """n: counts [m]; q -> (k_lo, k_hi, rem) int64 [m, Q] by the rank rule; all 0 where n == 0."""
    n = np.asarray(n, np.int64).reshape(-1)
    tab = q_table(q).astype(np.int64)
    t = np.maximum(n - 1, 0)[:, None] * tab[None, :, 0]             # < 2^30 * 2^20
    k_lo, rem = t // tab[None, :, 1], t % tab[None, :, 1]
    return k_lo, k_lo + (rem != 0), rem


def _select(cum, k):
    """cum: inclusive cumulative counts [..., 256]; k: ranks [...] -> (the first bin with cum > k, clipped to 255; k - the count below it)"""
    b = np.minimum((cum <= k[..., None]).sum(-1), 255)
    below = np.where(b > 0, np.take_along_axis(cum, np.maximum(b - 1, 0)[..., None], -1)[..., 0], 0)
    return b, k - below


# ---- the derived quantities -----------------------------------------------------------------------------------------------------------

class Quantiles:
    """raw = host int64 [n, C, 1 + 2 Q] rows {n, lo_0, hi_0, ...}, one per instance (or job) and channel; q = the Q quantiles as
    fractions.Fraction.  Everything else is derived here, in float64, from those integers only."""
    __slots__ = ("raw", "q")

    def __init__(self, raw, q=None):
        self.q = as_fractions(q)
        r = np.ascontiguousarray(raw, np.int64)
        if r.ndim != 3 or not 1 <= r.shape[1] <= MAX_CHANNELS or r.shape[2] != 1 + 2 * len(self.q):
            raise KGLibraryError(f"Quantiles: raw must be integers [n, C, 1 + 2 Q] with Q = {len(self.q)}, not {r.shape}")
        self.raw = r

    def __len__(self):
        return len(self.raw)

    @property
    def channels(self):
        return self.raw.shape[1]

    def counts(self):
        """int64 [n]: the pixels of every instance (the same in every channel)"""
        return self.raw[:, 0, 0]

    def _nan(self, a):
        return np.where((self.raw[:, :, :1] > 0), a.astype(np.float64), np.nan)

    def lower(self):
        """float64 [n, C, Q]: v[k_lo], numpy's method="lower"; NaN where n == 0"""
        return self._nan(self.raw[:, :, 1::2])

    def higher(self):
        """float64 [n, C, Q]: v[k_hi], numpy's method="higher"; NaN where n == 0"""
        return self._nan(self.raw[:, :, 2::2])

    def linear(self):
        """float64 [n, C, Q]: lo + (hi - lo) * rem / den, numpy's default percentile; NaN where n == 0"""
        rem = ranks(self.counts(), self.q)[2].astype(np.float64)
        den = np.array([f.denominator for f in self.q], np.float64)
        lo, hi = self.raw[:, :, 1::2].astype(np.float64), self.raw[:, :, 2::2].astype(np.float64)
        return self._nan(lo + (hi - lo) * (rem / den)[:, None, :])

    def _at(self, f):
        if f not in self.q:
            raise KGLibraryError(f"Quantiles: {f} was not among the quantiles asked for {tuple(str(v) for v in self.q)}")
        return self.q.index(f)

    def median(self):
        """float64 [n, C]: linear() at 1/2, which must have been asked for"""
        return self.linear()[:, :, self._at(Fraction(1, 2))]

    def iqr(self):
        """float64 [n, C]: linear() at 3/4 minus linear() at 1/4; both must have been asked for"""
        lin = self.linear()
        return lin[:, :, self._at(Fraction(3, 4))] - lin[:, :, self._at(Fraction(1, 4))]

    def props(self):
        """dict: count int64 [n]; lower, higher, linear float64 [n, C, Q]; median [n, C] where 1/2 was asked for; iqr [n, C] where both
        1/4 and 3/4 were."""
        out = {"count": self.counts(), "lower": self.lower(), "higher": self.higher(), "linear": self.linear()}
        if Fraction(1, 2) in self.q:
            out["median"] = self.median()
        if Fraction(1, 4) in self.q and Fraction(3, 4) in self.q:
            out["iqr"] = self.iqr()
        return out


class Histograms:
    """counts = host int64 [n, C, 256], one histogram per instance (or job) and channel; shift = the right shift the values were binned
    under (bin b holds the values b << shift .. ((b + 1) << shift) - 1; bin 255 everything above as well)."""
    __slots__ = ("counts", "shift")

    def __init__(self, counts, shift=0):
        c = np.ascontiguousarray(counts, np.int64)
        if c.ndim != 3 or c.shape[2] != 256 or not 0 <= int(shift) <= 8:
            raise KGLibraryError(f"Histograms: counts must be integers [n, C, 256], not {c.shape}, and 0 <= shift <= 8")
        self.counts, self.shift = c, int(shift)

    def __len__(self):
        return len(self.counts)

    def totals(self):
        """int64 [n, C]: the pixels counted"""
        return self.counts.sum(-1)

    def mode(self):
        """int64 [n, C]: the fullest bin, the smallest on a tie (0 for an empty histogram)"""
        return self.counts.argmax(-1).astype(np.int64)

    def entropy(self):
        """float64 [n, C]: -sum p log2 p over the occupied bins, in bits; NaN for an empty histogram"""
        tot = self.totals().astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            p = self.counts / tot[..., None]
            return np.where(tot > 0, -(np.where(p > 0, p * np.log2(np.where(p > 0, p, 1.0)), 0.0)).sum(-1), np.nan)

    def otsu(self):
        """int64 [n, C]: the threshold bin t in 0 .. 254 -- class 0 = the bins <= t, class 1 = the bins > t -- that maximises the
        between-class variance w0 w1 (mu0 - mu1)^2 = (N S0 - S N0)^2 / (N^2 N0 N1), with N0, S0 the count and the bin-weighted sum of
        class 0 and N, S of everything; a threshold with an empty class has variance 0; the smallest t on a tie (so 0 for an empty or a
        one-bin histogram).  Compared exactly, by cross-multiplication in Python integers: the squares pass 2^64."""
        c = self.counts.astype(object)
        bins = np.arange(256).astype(object)
        N0, S0 = np.cumsum(c, -1)[..., :255], np.cumsum(c * bins, -1)[..., :255]
        N, S = c.sum(-1)[..., None], (c * bins).sum(-1)[..., None]
        num, den = (N * S0 - S * N0) ** 2, N0 * (N - N0)
        best = np.zeros(c.shape[:2], np.int64)
        bnum, bden = np.zeros(c.shape[:2], object), np.ones(c.shape[:2], object)
        for t in range(255):
            nt, dt = num[..., t], den[..., t]
            better = np.asarray((dt > 0) & (nt * bden > bnum * np.where(dt > 0, dt, 1)), bool)
            best[better] = t
            bnum, bden = np.where(better, nt, bnum), np.where(better, dt, bden)
        return best

    def quantile(self, num, den):
        """int64 [n, C, 2]: the bins of the order statistics k_lo, k_hi of num / den, by the rank rule read off the cumulative counts; zeros
        for an empty histogram.  On uint8 with shift 0 these are the lo and hi of Quantiles."""
        f = as_fractions([(num, den)])
        tot = self.totals()
        k_lo, k_hi, _ = ranks(tot.reshape(-1), f)
        k = np.stack([k_lo[:, 0], k_hi[:, 0]], -1).reshape(tot.shape + (2,))
        b = _select(np.cumsum(self.counts, -1)[:, :, None, :], k)[0]
        return np.where(tot[..., None] > 0, b, 0)


# ---- host statement of the semantics ----------------------------------------------------------------------------------------------------

def _pixels(maps, img, job):
    """the values [|P|, C] of one job (img, id, y1, x1, y2, x2), or None for a bad job"""
    nimg, H, W = maps.shape
    i, v, y1, x1, y2, x2 = job
    y1, x1, y2, x2 = max(y1, 0), max(x1, 0), min(y2, H), min(x2, W)
    if not 0 <= i < nimg or y2 <= y1 or x2 <= x1:
        return None
    me = maps[i, y1:y2, x1:x2] == v
    return img[i, y1:y2, x1:x2][me].astype(np.int64) if me.any() else None


def quantiles_host(labels, jobs_or_n, image, q=None):
    """labels: integers [H, W] or [nimg, H, W]; jobs_or_n: jobs [m, 6] = (img, id, y1, x1, y2, x2), or the instance count n (one per map
    for a stack): the ids 1 .. n inside their own boxes (labelmetrics.label_stats_host); image: uint8 / uint16 [H, W, C] /
    [nimg, H, W, C]; q: as_fractions' -> int64 [m, C, 1 + 2 Q].  Per job and channel: sort, index by the integer rule.  Nothing split."""
    maps, img = host_args("quantiles_host", labels, image)
    qs = as_fractions(q)
    j = _labelmaps.host_job_table("quantiles_host", maps, jobs_or_n, labelmetrics.label_stats_host)
    C = img.shape[3]
    out = np.zeros((len(j), C, 1 + 2 * len(qs)), np.int64)
    for a, job in enumerate(j.tolist()):
        px = _pixels(maps, img, job)
        if px is None:
            continue
        v = np.sort(px, 0)                                             # [n, C]
        k_lo, k_hi, _ = ranks([len(v)], qs)
        out[a, :, 0] = len(v)
        out[a, :, 1::2], out[a, :, 2::2] = v[k_lo[0]].T, v[k_hi[0]].T
    return out


def histograms_host(labels, jobs, image):
    """labels, image as quantiles_host; jobs: integers [m, 9] = (img, id, y1, x1, y2, x2, channel, shift, prefix) -> int64 [m, 256]"""
    maps, img = host_args("histograms_host", labels, image)
    j = _labelmaps.host_jobs("histograms_host", jobs, 9, _HIST_JOB_COLUMNS).astype(np.int64)
    C = img.shape[3]
    out = np.zeros((len(j), 256), np.int64)
    for a, (*job, ch, shift, prefix) in enumerate(j.tolist()):
        if not 0 <= ch < C or not 0 <= shift <= 8:
            continue
        px = _pixels(maps, img, job)
        if px is None:
            continue
        w = px[:, ch] >> shift
        w = np.minimum(w, 255) if prefix < 0 else (w[(w >> 8) == prefix] & 255)
        out[a] = np.bincount(w, minlength=256)
    return out


# ---- the large-job route: selection from added piece histograms ---------------------------------------------------------------------------

def _hist_jobs(pieces, channels, shift, prefix):
    """pieces [mp, 6] -> [mp * len(channels), 9], piece-major; channels / prefix: one value per output row, or scalars"""
    p = np.asarray(pieces, np.int64).reshape(-1, 6)
    out = np.empty((len(p), 9), np.int64)
    out[:, :6], out[:, 6], out[:, 7], out[:, 8] = p, channels, shift, prefix
    return out


def quantiles_from_histograms(jobs, C, wide, q, max_job_pixels, hist_rows):
    """The route of the jobs too large for one workgroup.  jobs: clamped [m, 6]; C channels; wide: 16-bit values; hist_rows: a function
    from histogram jobs [k, 9] to their rows int [k, 256] (histogram_rows on the device, histograms_host on the host) -> int64
    [m, C, 1 + 2 Q].  hist_rows is called once, and once more for 16-bit values."""
    qs = as_fractions(q)
    j = np.asarray(jobs, np.int64).reshape(-1, 6)
    m, R = len(j), 2 * len(qs)
    out = np.zeros((m, C, 1 + R), np.int64)
    if m == 0:
        return out
    pieces, owner = split_jobs(j, max_job_pixels)
    mp = len(pieces)
    rows = np.asarray(hist_rows(_hist_jobs(np.repeat(pieces, C, 0), np.tile(np.arange(C), mp), 8 if wide else 0, -1)), np.int64)
    h1 = np.zeros((m, C, 256), np.int64)
    np.add.at(h1, owner, rows.reshape(mp, C, 256))
    n = h1[:, 0].sum(-1)
    k_lo, k_hi, _ = ranks(n, qs)
    k = np.stack([k_lo, k_hi], -1).reshape(m, R)                       # lo_0, hi_0, lo_1, ...
    kk = np.broadcast_to(k[:, None, :], (m, C, R))
    sel, resid = _select(np.cumsum(h1, -1)[:, :, None, :], kk)
    live = np.broadcast_to((n > 0)[:, None, None], sel.shape)
    if wide:
        key = (np.arange(m)[:, None, None] * C + np.arange(C)[None, :, None]) * 256 + sel
        uniq, inv = np.unique(key[live], return_inverse=True)          # the distinct (job, channel, selected high byte)
        uj, uc, ub = uniq // (256 * C), uniq // 256 % C, uniq % 256
        start = np.searchsorted(owner, np.arange(m + 1))
        cnt = start[uj + 1] - start[uj]
        which = np.repeat(np.arange(len(uniq)), cnt)
        at = np.arange(len(which)) - np.repeat(np.cumsum(cnt) - cnt, cnt) + start[uj][which]
        rows2 = np.asarray(hist_rows(_hist_jobs(pieces[at], uc[which], 0, ub[which])), np.int64)
        h2 = np.zeros((len(uniq), 256), np.int64)
        np.add.at(h2, which, rows2)
        low = _select(np.cumsum(h2, -1)[inv], resid[live])[0]
        val = np.zeros(sel.shape, np.int64)
        val[live] = (sel[live] << 8) | low
        sel = val
    out[:, :, 0] = n[:, None]
    out[:, :, 1:] = np.where(live, sel, 0)
    return out


# ---- device -----------------------------------------------------------------------------------------------------------------------------

def quantile_rows(labels, jobs, image, q=None):
    """kg_label_quantiles as it is: labels device int32 [H, W] or [nimg, H, W]; jobs host integers [m, 6] (uploaded once) or a device int32
    tensor; image a host array (uploaded once) or a device tensor; q: as_fractions' (the table is uploaded), or a device int32 [Q, 2]
    tensor of (num, den) rows, taken as it is -> device int32 [m, C, 1 + 2 Q].  One launch, no copy back, no synchronisation, nothing
    split."""
    import torch
    from . import ops
    lab, img = device_args("quantile_rows", labels, image)
    if torch.is_tensor(q):
        if q.dtype != torch.int32 or q.dim() != 2 or q.shape[1] != 2 or not 1 <= q.shape[0] <= MAX_Q or q.device != lab.device:
            raise KGLibraryError(f"quantile_rows: a device quantile table must be int32 [Q, 2], 1 <= Q <= {MAX_Q}, on the maps' device")
        qd = q.contiguous()
    else:
        qd = ops.h2d(q_table(q), lab.device)
    jd = _labelmaps.device_jobs("quantile_rows", jobs, 6, _JOB_COLUMNS, lab.device)
    Q = qd.shape[0]
    return job_rows("kg_label_quantiles", lab, img, jd, (_lib.ptr(qd), Q), (img.shape[3], 1 + 2 * Q))


def histogram_rows(labels, jobs, image):
    """kg_label_histograms as it is: labels, image as quantile_rows; jobs host integers [m, 9] = (img, id, y1, x1, y2, x2, channel, shift,
    prefix) (uploaded once) or a device int32 tensor -> device int32 [m, 256].  One launch, no copy back, no synchronisation."""
    lab, img = device_args("histogram_rows", labels, image)
    jd = _labelmaps.device_jobs("histogram_rows", jobs, 9, _HIST_JOB_COLUMNS, lab.device)
    return job_rows("kg_label_histograms", lab, img, jd, (), (256,))


def _device_quantiles(lab, img, j, qs, max_job_pixels):
    """lab, img: device tensors; j: clamped host jobs [m, 6] -> Quantiles"""
    from . import ops
    cap = check_cap("quantiles", max_job_pixels)
    C, Q = img.shape[3], len(qs)
    raw = np.zeros((len(j), C, 1 + 2 * Q), np.int64)
    large = (j[:, 4] - j[:, 2]) * (j[:, 5] - j[:, 3]) > cap
    small = np.flatnonzero(~large)
    if len(small):                                                     # the table and the jobs travel in one upload
        both = ops.h2d(np.concatenate([q_table(qs).reshape(-1), j[small].reshape(-1)]).astype(np.int32), lab.device)
        raw[small] = quantile_rows(lab, both[2 * Q:].view(-1, 6), img, both[:2 * Q].view(Q, 2)).cpu().numpy()
    if large.any():
        raw[large] = quantiles_from_histograms(j[large], C, img.element_size() == 2, qs, cap,
                                               lambda j9: histogram_rows(lab, j9, img).cpu().numpy())
    return Quantiles(raw, qs)


def quantiles(labels, n=None, jobs=None, image=None, q=None, stats=None, max_job_pixels=65536):
    """quantiles_host on the device -> Quantiles (host).  labels: device int32 [H, W] or [nimg, H, W].  What is taken:
      jobs   host integers [m, 6] = (img, id, y1, x1, y2, x2): one row per job; or
      n      the instance count (one per map for a stack): the ids 1 .. n inside their own boxes.  The boxes come from stats -- host
             integers [n, 5] = (area, y1, x1, y2, x2), one array per map for a stack -- or, without stats, from labelmetrics.label_stats.
    image: a host uint8 / uint16 array [H, W, C] / [nimg, H, W, C] (uploaded once) or a device tensor; q: as_fractions'.
    ONE kg_label_quantiles launch, one upload (the quantile table and the jobs) and one copy back when no job holds more than
    max_job_pixels pixels; such jobs take the histogram route (one more launch and copy back, two for uint16)."""
    lab, img = device_args("quantiles", labels, image)
    return _device_quantiles(lab, img, job_table("quantiles", lab, n, jobs, stats, labelmetrics.label_stats), as_fractions(q), max_job_pixels)


def histograms(labels, n=None, jobs=None, image=None, shift=None, stats=None, max_job_pixels=65536):
    """Per job and channel the 256-bin histogram of value >> shift (the last bin collects what lies above) -> Histograms (host int64
    [m, C, 256]).  labels, n / jobs / stats, image as quantiles; shift: None (0 for uint8, 8 for uint16) or 0 .. 8.  A job of more than
    max_job_pixels pixels is cut into pieces (labelmetrics.split_jobs) whose rows are added on the host.  ONE kg_label_histograms launch,
    one upload and one copy back."""
    lab, img = device_args("histograms", labels, image)
    j = job_table("histograms", lab, n, jobs, stats, labelmetrics.label_stats)
    shift = (8 if img.element_size() == 2 else 0) if shift is None else int(shift)
    if not 0 <= shift <= 8:
        raise KGLibraryError(f"histograms: shift {shift} (0 .. 8)")
    C = img.shape[3]
    pieces, owner = split_jobs(j, check_cap("histograms", max_job_pixels))
    rows = histogram_rows(lab, _hist_jobs(np.repeat(pieces, C, 0), np.tile(np.arange(C), len(pieces)), shift, -1), img).cpu().numpy()
    counts = np.zeros((len(j), C, 256), np.int64)
    np.add.at(counts, owner, rows.reshape(len(pieces), C, 256).astype(np.int64))
    return Histograms(counts, shift)


# ---- Instances ----------------------------------------------------------------------------------------------------------------------------

def quantiles_instances(inst, image, q=None, max_job_pixels=65536):
    """quantiles for an Instances / TiledInstances -> Quantiles with len(inst) rows: ids 1 .. n, boxes from table[:, 2:6]; an instance with
    no visible pixel gets zeros (NaN once derived).  image: uint8 / uint16 [H, W, C] at the label map's size (host array or device
    tensor).  A host label map (assemble_host's result) goes through quantiles_host."""
    stats = _labelmaps.instance_stats("quantiles_instances", inst)
    if is_device(inst.labels):
        return quantiles(inst.labels, len(inst), image=image, q=q, stats=stats, max_job_pixels=max_job_pixels)
    qs = as_fractions(q)
    return Quantiles(quantiles_host(_labelmaps.host_labels(inst), _labelmaps.jobs_from_stats(stats), _labelmaps.host_pixels(image), qs), qs)


def quantiles_instances_batch(insts, images, q=None, max_job_pixels=65536):
    """quantiles_instances for predict_instances' list (entries may be None), in place: every entry's `quantiles` is set.  ONE launch for
    all images of one output size.  images: uint8 / uint16 [N, h, w, C] (host array or device tensor), one image per entry, at the label
    maps' size."""
    qs = as_fractions(q)
    if images is None or len(images) != len(insts):
        raise KGLibraryError(f"quantiles: {0 if images is None else len(images)} images for {len(insts)} entries")
    for idx, stack, _, _ in _labelmaps.size_batches("quantiles_instances_batch", insts):
        got = quantiles(stack, [len(insts[i]) for i in idx], image=images[idx] if len(idx) != len(insts) else images, q=qs,
                        stats=[_labelmaps.instance_stats("quantiles_instances_batch", insts[i]) for i in idx], max_job_pixels=max_job_pixels)
        for i, a, b in _labelmaps.deal(insts, idx):
            insts[i].quantiles = Quantiles(got.raw[a:b], qs)
    return insts
