"""Instance midlines on the device: exact thinning of every instance of a label map, and the length, tips and branch points of what remains.

Every other label-map module describes a compact blob (area, moments, hull, Feret diameters, inscribed circle, texture, quantiles).  A
neural cell has processes and a rosette leaf has a blade on a petiole: such objects are measured by their topological skeleton -- the
length along the midline, the number of tips, the number of branch points (CellProfiler's MorphologicalSkeleton / MeasureObjectSkeleton,
skimage's thin, OpenCV's ximgproc.thinning).  None of these is a function of measure.py's sums, of the hull or of the distance transform.
Here the device thins every instance inside its box (kg_label_thin, csrc/thinning.hip) and the midline map and nine integers per
instance come back instead of the label map.  The feature is called thinning / midlines everywhere: "skeleton" already means the keypoint
skeleton of the post-processing.

    thin_host            the rule on one boolean array (or a stack) by shifted comparisons: the yardstick
    midlines_host        the statement below over jobs, in NumPy, never size-limited
    thin_rows            kg_label_thin as it is: ONE launch, everything stays on the device
    thin                 midlines_host from a device map: one upload, ONE launch, one copy back; a box that does not fit is thinned on the host
    Midlines             rows + skel: pixels(), ends(), junctions(), isolated(), passes(), lengths(), props()
    thin_instances       thin for an Instances / TiledInstances (ids 1 .. n, boxes from its table); predict_instances and predict_tiled
                         take thin=

Thinning stopped after k passes (max_passes=k) is an erosion that never deletes a component and never opens or closes a hole, which
distance.shrink_labels cannot promise for a thin object.

Semantics (include/kgnet_hip.h is the normative text)
  job         {img, id, y1, x1, y2, x2}: a half-open box, clamped to the map.  P = the pixels of the box in image img with labels == id.
              Everything outside the clamped box is background: a box that cuts an object thins the cut part.  Any int32 is an id.
  neighbours  clockwise from north, y growing downward: P2 = N, P3 = NE, P4 = E, P5 = SE, P6 = S, P7 = SW, P8 = W, P9 = NW.
  pass        two sub-iterations, each fully synchronous.  A set pixel is deleted iff C == 1 and 2 <= N <= 3 and m == 0, where
                C  = (!P2 & (P3|P4)) + (!P4 & (P5|P6)) + (!P6 & (P7|P8)) + (!P8 & (P9|P2))
                N1 = (P9|P2) + (P3|P4) + (P5|P6) + (P7|P8),  N2 = (P2|P3) + (P4|P5) + (P6|P7) + (P8|P9),  N = min(N1, N2)
                m  = (P6 | P7 | !P9) & P8 in the first sub-iteration, (P2 | P3 | !P5) & P4 in the second
              (Guo-Hall's parallel thinning with OpenCV's sub-iteration order).  Passes repeat until one deletes nothing, or max_passes
              have run; passes = the number of passes that deleted something; S = what remains.
  row         int [9] = ROW_COLUMNS, counted on S with 8-neighbourhoods inside S: members = |P|, pixels = |S|; isolated: no neighbour;
              ends: exactly one; junctions: at least three 0 -> 1 transitions in the cyclic sequence P2 .. P9; ortho: unordered pairs of S
              pixels that share a side; diag: unordered diagonal pairs neither of whose two common side-neighbours is in S (a diagonal
              that an L already bridges is no edge); status 0.  A bad job (image index, empty box) gets a row of zeros.
  map         skel int32 of the labels' shape: id on the pixels of S of every job, 0 elsewhere -- a label map like any other.
  size        a job is thinned on the device when fits(h, w) of its clamped box: (h + 2) * ceil((w + 2) / 32) <= 4096, one bit per pixel
              with a one-pixel halo in 16 KiB of LDS.  The entry gives any other job status 1, zeros and no pixels; thin thins such a box
              on the host from that box copied back and writes it in (split.py and contours.py do the same for their large boxes): its
              row then holds the host's counts and keeps status 1."""
import numpy as np

from . import _lib, _labelmaps, labelmetrics
from ._labelmaps import JOB_COLUMNS as _JOB_COLUMNS

KGLibraryError = _lib.KGLibraryError
MAX_WORDS = 4096                        # KG_TH_WORDS of csrc/thinning.hip
ROW_COLUMNS = ("members", "pixels", "isolated", "ends", "junctions", "ortho", "diag", "passes", "status")


def fits(h, w):
    """True when a clamped box of h x w pixels is thinned on the device: (h + 2) * ceil((w + 2) / 32) <= 4096."""
    return (int(h) + 2) * ((int(w) + 2 + 31) // 32) <= MAX_WORDS


def _passes(fn, max_passes):
    """None or 0: no limit -> 0; else an integer >= 1"""
    if max_passes is None:
        return 0
    if isinstance(max_passes, (bool, np.bool_)) or not isinstance(max_passes, (int, np.integer)) or not 0 <= max_passes <= 2 ** 31 - 1:
        raise KGLibraryError(f"{fn}: max_passes {max_passes!r} must be None, 0 (no limit) or an integer >= 1")
    return int(max_passes)


class Midlines:
    """rows = host int64 [m, 9] (ROW_COLUMNS), one row per job or instance; skel = the midline map the rows were counted on (a device
    int32 tensor from the device route, an array from the host route, or None)."""
    __slots__ = ("rows", "skel")

    def __init__(self, rows, skel=None):
        self.rows = np.ascontiguousarray(rows, np.int64).reshape(-1, 9)
        self.skel = skel

    def __len__(self):
        return len(self.rows)

    def __eq__(self, other):
        return isinstance(other, Midlines) and np.array_equal(self.rows, other.rows)

    __hash__ = None

    def members(self):
        """int64 [m]: the pixels of every object"""
        return self.rows[:, 0].copy()

    def pixels(self):
        """int64 [m]: the pixels of every midline"""
        return self.rows[:, 1].copy()

    def isolated(self):
        """int64 [m]: midline pixels without a neighbour (an object thinned to a point)"""
        return self.rows[:, 2].copy()

    def ends(self):
        """int64 [m]: the tips, midline pixels with exactly one neighbour"""
        return self.rows[:, 3].copy()

    def junctions(self):
        """int64 [m]: the branch points, midline pixels with at least three 0 -> 1 transitions around them"""
        return self.rows[:, 4].copy()

    def passes(self):
        """int64 [m]: the passes that deleted something, about half the object's largest width"""
        return self.rows[:, 7].copy()

    def lengths(self):
        """float64 [m]: ortho + sqrt(2) * diag, the length along the midline; 0 for an empty row"""
        return self.rows[:, 5].astype(np.float64) + np.sqrt(2.0) * self.rows[:, 6].astype(np.float64)

    def props(self):
        """dict of float64 arrays [m], from the integers only: members, pixels, isolated, ends, junctions, passes, length, and thinness =
        pixels / members (NaN for an empty row)."""
        r = self.rows.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            thin_ = np.where(r[:, 0] > 0, r[:, 1] / r[:, 0], np.nan)
        return {"members": r[:, 0], "pixels": r[:, 1], "isolated": r[:, 2], "ends": r[:, 3], "junctions": r[:, 4], "passes": r[:, 7],
                "length": self.lengths(), "thinness": thin_}


# ---- host statements of the semantics ---------------------------------------------------------------------------------------------------

def _planes(pad):
    """pad bool [n, h + 2, w + 2] -> (the centre, [P2 .. P9]) as views [n, h, w]"""
    return pad[:, 1:-1, 1:-1], [pad[:, :-2, 1:-1], pad[:, :-2, 2:], pad[:, 1:-1, 2:], pad[:, 2:, 2:], pad[:, 2:, 1:-1], pad[:, 2:, :-2],
                                pad[:, 1:-1, :-2], pad[:, :-2, :-2]]


def deletable(mask, second):
    """The pixels of a boolean stack [n, h, w] that sub-iteration `second` (False: the first) deletes: the rule as it is written, with
    integer sums and a minimum."""
    n, h, w = mask.shape
    pad = np.zeros((n, h + 2, w + 2), bool)
    pad[:, 1:-1, 1:-1] = mask
    c, (P2, P3, P4, P5, P6, P7, P8, P9) = _planes(pad)
    i8 = np.int8
    C = (~P2 & (P3 | P4)).astype(i8) + (~P4 & (P5 | P6)) + (~P6 & (P7 | P8)) + (~P8 & (P9 | P2))
    N1 = (P9 | P2).astype(i8) + (P3 | P4) + (P5 | P6) + (P7 | P8)
    N2 = (P2 | P3).astype(i8) + (P4 | P5) + (P6 | P7) + (P8 | P9)
    N = np.minimum(N1, N2)
    m = ((P2 | P3 | ~P5) & P4) if second else ((P6 | P7 | ~P9) & P8)
    return c & (C == 1) & (N >= 2) & (N <= 3) & ~m


def thin_host(mask, max_passes=None):
    """The rule on one boolean array [h, w] -> (S bool [h, w], passes); or on a stack [n, h, w], every array on its own -> (S bool
    [n, h, w], passes int64 [n]).  max_passes: None or 0 for no limit, else the passes to run at most."""
    limit = _passes("thin_host", max_passes)
    a = np.asarray(mask)
    if a.ndim not in (2, 3) or a.dtype.kind not in "biu":
        raise KGLibraryError("thin_host: a boolean array [h, w] or [n, h, w]")
    s = (a != 0).reshape((-1,) + a.shape[-2:]).copy()
    passes = np.zeros(len(s), np.int64)
    done = 0
    while s.size and (limit == 0 or done < limit):
        before = s.copy()
        s &= ~deletable(s, False)
        s &= ~deletable(s, True)
        changed = (s != before).reshape(len(s), -1).any(1)
        if not changed.any():
            break
        passes += changed                                                # a fixed point stays one: the deleting passes come first
        done += 1
    return (s[0], int(passes[0])) if a.ndim == 2 else (s, passes)


def count_host(S):
    """S bool [h, w] -> int64 [6] = (pixels, isolated, ends, junctions, ortho, diag) of ROW_COLUMNS"""
    S = np.asarray(S, bool)
    pad = np.zeros((1, S.shape[0] + 2, S.shape[1] + 2), bool)
    pad[0, 1:-1, 1:-1] = S
    c, nb = _planes(pad)
    P2, P3, P4, P5, P6, P7, P8, P9 = nb
    deg = sum(p.astype(np.int8) for p in nb)
    trans = sum((~nb[q] & nb[(q + 1) % 8]).astype(np.int8) for q in range(8))
    return np.array([c.sum(), (c & (deg == 0)).sum(), (c & (deg == 1)).sum(), (c & (trans >= 3)).sum(), (c & P4).sum() + (c & P6).sum(),
                     (c & P5 & ~P4 & ~P6).sum() + (c & P7 & ~P8 & ~P6).sum()], np.int64)


def _box_row(P, limit):
    """P bool [h, w] -> (S, the row int64 [9] with status 0)"""
    S, passes = thin_host(P, limit)
    return S, np.concatenate([[P.sum()], count_host(S), [passes, 0]]).astype(np.int64)


def midlines_host(labels, jobs_or_n, max_passes=None):
    """kg_label_thin in NumPy: labels integers [H, W] or [nimg, H, W]; jobs_or_n: jobs [m, 6] = (img, id, y1, x1, y2, x2), or the instance
    count n (one per map for a stack): the ids 1 .. n inside their own boxes (labelmetrics.label_stats_host) -> (skel int32 of the
    labels' shape, Midlines with one row per job, which keeps skel).  Never size-limited: status is 0."""
    limit = _passes("midlines_host", max_passes)
    maps, single = _labelmaps.host_maps("midlines_host", labels, True)
    _labelmaps.side("midlines_host", maps)
    nimg, H, W = maps.shape
    j = _labelmaps.host_job_table("midlines_host", maps, jobs_or_n, labelmetrics.label_stats_host)
    skel = np.zeros(maps.shape, np.int32)
    rows = np.zeros((len(j), 9), np.int64)
    for k, (i, v, y1, x1, y2, x2) in enumerate(j.tolist()):
        if not 0 <= i < nimg or y2 <= y1 or x2 <= x1:
            continue
        S, rows[k] = _box_row(maps[i, y1:y2, x1:x2] == v, limit)
        skel[i, y1:y2, x1:x2][S] = v                                     # a view: the assignment writes skel
    skel = skel[0] if single else skel
    return skel, Midlines(rows, skel)


# ---- device -----------------------------------------------------------------------------------------------------------------------------

def thin_rows(labels, jobs, max_passes=None, out=None):
    """kg_label_thin as it is: labels device int32 [H, W] or [nimg, H, W]; jobs host integers [m, 6] = (img, id, y1, x1, y2, x2) (uploaded
    once) or a device int32 tensor -> (skel device int32 of the labels' shape, rows device int32 [m, 9] = ROW_COLUMNS).  out: None, or a
    contiguous device int32 tensor of the labels' shape that becomes skel (every element is written).  A job that does not fit has
    status 1 and leaves no pixels.  One clear and one launch, no copy back, no synchronisation."""
    import torch
    from ._lib import ptr, stream_ptr
    limit = _passes("thin_rows", max_passes)
    lab, shape = _labelmaps.device_stack("thin_rows", labels)
    nimg, H, W = lab.shape
    jd = _labelmaps.device_jobs("thin_rows", jobs, 6, _JOB_COLUMNS, lab.device)
    m = jd.shape[0]
    skel = torch.empty_like(lab) if out is None else _labelmaps.out_tensor("thin_rows", "out", out, shape, torch.int32, lab.device)
    rows = torch.empty(m, 9, dtype=torch.int32, device=lab.device)
    with torch.cuda.device(lab.device):
        _lib.call("kg_label_thin", ptr(lab), nimg, H, W, ptr(jd) if m else None, m, limit, ptr(skel), ptr(rows) if m else None, stream_ptr())
    return skel.view(shape), rows


def _device_thin(lab, j, limit, out=None):
    """lab: device int32 [nimg, H, W], j: host jobs int64 [m, 6], clamped -> (skel device [nimg, H, W], rows host int64 [m, 9])"""
    from . import ops
    skel, rows = thin_rows(lab, j, limit, out)
    skel = skel.view(lab.shape)
    rows = rows.cpu().numpy().astype(np.int64) if len(j) else np.zeros((0, 9), np.int64)
    h, w = j[:, 4] - j[:, 2], j[:, 5] - j[:, 3]
    large = (j[:, 0] >= 0) & (j[:, 0] < lab.shape[0]) & (h > 0) & (w > 0) & ((h + 2) * ((w + 2 + 31) // 32) > MAX_WORDS)     # not fits(h, w)
    if (rows < 0).any() or not np.array_equal(rows[:, 8], large.astype(np.int64)):
        raise KGLibraryError("thin: rows that are no rows")
    for k in np.flatnonzero(large).tolist():                              # thinning cannot be banded: the box comes back
        i, v, y1, x1, y2, x2 = j[k].tolist()
        S, row = _box_row(lab[i, y1:y2, x1:x2].cpu().numpy() == v, limit)
        rows[k, :8] = row[:8]
        if S.any():
            box = skel[i, y1:y2, x1:x2].cpu().numpy()
            box[S] = v
            skel[i, y1:y2, x1:x2].copy_(ops.h2d(np.ascontiguousarray(box), lab.device))
    return skel, rows


def thin(labels, n=None, jobs=None, stats=None, max_passes=None, out=None):
    """midlines_host on the device -> (skel device int32 of the labels' shape, Midlines with host rows, which keeps skel).  labels: device
    int32 [H, W] or [nimg, H, W].  What is taken:
      jobs   host integers [m, 6] = (img, id, y1, x1, y2, x2): one row per job; or
      n      the instance count (one per map for a stack): the ids 1 .. n inside their own boxes.  The boxes come from stats -- host
             integers [n, 5] = (area, y1, x1, y2, x2), one array per map for a stack -- or, without stats, from labelmetrics.label_stats.
    One upload (the jobs), ONE kg_label_thin launch behind its clear, one copy back (the rows).  Only a job whose clamped box does not
    fit (fits, decided from the boxes) costs more: it is thinned by thin_host from that box copied back and its pixels are written into
    skel; its row holds the host's counts and keeps status 1.  out: as thin_rows'."""
    limit = _passes("thin", max_passes)
    lab, shape = _labelmaps.device_stack("thin", labels)
    j = _labelmaps.job_table("thin", lab, n, jobs, stats, labelmetrics.label_stats)
    skel, rows = _device_thin(lab, j, limit, None if out is None else _labelmaps.out_tensor("thin", "out", out, shape, lab.dtype, lab.device).view(lab.shape))
    skel = skel.view(shape)
    return skel, Midlines(rows, skel)


# ---- Instances ----------------------------------------------------------------------------------------------------------------------------

def _instance_midlines(insts, max_passes=None):
    """-> one Midlines per entry (None for a None entry); the entries themselves are not touched"""
    limit = _passes("thin_instances", max_passes)
    res = [None] * len(insts)

    def host_one(i, inst, lab):
        res[i] = midlines_host(lab, _labelmaps.instance_jobs(inst, 0, 0, *lab.shape), limit)[1]
    for idx, stack, H, W in _labelmaps.size_batches("thin_instances", insts, host_one):
        lab = _labelmaps.device_stack("thin_instances", stack)[0]
        skel, rows = _device_thin(lab, _labelmaps.batch_jobs(insts, idx, 0, H, W), limit)
        for k, (i, a, b) in enumerate(_labelmaps.deal(insts, idx)):
            res[i] = Midlines(rows[a:b], skel[k])
    return res


def thin_instances(inst, max_passes=None):
    """thin for an Instances / TiledInstances -> Midlines with len(inst) rows: ids 1 .. n, boxes from table[:, 2:6]; an instance with no
    visible pixel gets a row of zeros; `skel` is the midline map of inst.labels.  A host label map (assemble_host's result) goes through
    midlines_host."""
    return _instance_midlines([inst], max_passes)[0]


def thin_instances_batch(insts, max_passes=None):
    """thin_instances for predict_instances' list (entries may be None), in place: every entry's `midlines` is set.  ONE launch per
    output size."""
    for v, g in zip(insts, _instance_midlines(insts, max_passes)):
        if v is not None:
            v.midlines = g
    return insts
