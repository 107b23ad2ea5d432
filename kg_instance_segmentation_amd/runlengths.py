"""Run-length lists of a label map on the device: Kaggle rows, COCO counts, and the way back to a label map.

The label map is what this project produces; the run-length list is what its data set is submitted in and what its ground truth arrives
in.  instances.rle_encode / rle_decode state the format on the host, over a label map copied back (they stay as they are: the yardstick).
Here the device lists the runs of every instance (kg_label_run_counts, kg_label_runs, csrc/runlengths.hip), some ten to thirty thousand
integers come back instead of the map, and the host builds a CSR structure over them; kg_runs_paint turns run-length rows into a device
label map without a host map in between.

    run_counts_host   kg_label_run_counts in NumPy (the yardstick of the raw entry)
    run_rows_host     kg_label_runs in NumPy, offsets and the store predicate included
    runs_host         the runs of every job in NumPy, stated directly: nothing split
    run_counts        kg_label_run_counts as it is: ONE launch, rows stay on the device
    run_rows          kg_label_runs as it is: ONE launch, rows stay on the device
    runs              runs_host from a device map: column bands, one count launch, a host prefix, one write launch
    split_columns     the bands: full height, ascending x (labelmetrics.split_jobs cuts rows and would break the pixel order)
    RunLengths        host CSR over the jobs: indptr, first, last; of(k), string(k), coco(k), counts(), areas(), to_dict()
    runs_instances    runs for an Instances / TiledInstances (ids 1 .. n, boxes from its table)
    paint_host        run-length rows -> a label map, in NumPy
    paint             the same on the device (kg_runs_paint)
    parse_string      'start length start length ...' -> int64 [r, 2]
    submission_rows   the (ImageId, EncodedPixels) rows of a Kaggle submission

Semantics (include/kgnet_hip.h is the normative text)
  pixel order p = x * H + y: down the columns first, then left to right, 0-based; lab.T.reshape(-1)[p] is the pixel.
  job         {img, id, y1, x1, y2, x2}: a half-open box, clamped to the map.  P = the pixels of the box in image img with labels == id.
              Values are compared only: id may be any int32, 0 included.
  head        a pixel of P with p == 0 or flat[p - 1] != id;  tail: a pixel of P with p == H * W - 1 or flat[p + 1] != id.  The
              neighbours are read from the MAP, never from the box, so a run continues from the bottom of one column into the top of
              the next, exactly as instances.rle_encode merges it.
  runs        the k-th head and the k-th tail of a job in ascending p are its k-th run {first, last}, inclusive; Kaggle's pair is
              (first + 1, last - first + 1).
  bad jobs    an image index outside [0, nimg), an empty or inverted box, an id the box does not hold: nothing.
  boxes       heads and tails pair into the runs of the instance when the box holds every pixel of id (the boxes of label_stats and of an
              Instances table do).  A box that cuts a run is refused by runs_host and runs alike where it shows: unequal counts of
              heads and tails, first > last, or runs that do not ascend.
  bands       a box of more than max_job_pixels pixels is cut into column bands of the box's full height and max(max_job_pixels // h, 1)
              columns, in ascending x.  Heads and tails of the bands concatenate to the job's; a band can hold a head whose tail lies in
              a later band, so the two are counted and offset separately.
  sizes       H, W <= 32768 and nimg * H * W <= 2^31 - 1, so p fits int32."""
import numpy as np

from . import _lib, _labelmaps, labelmetrics
from ._labelmaps import JOB_COLUMNS as _JOB_COLUMNS, MAX_SIDE, device_stack, host_stack, is_device, out_tensor  # noqa: F401  (MAX_SIDE: public here)

KGLibraryError = _lib.KGLibraryError
_ROW_JOB_COLUMNS = "(img, id, y1, x1, y2, x2, head_at, tail_at)"


def _size(fn, H, W):
    if isinstance(H, (bool, np.bool_)) or isinstance(W, (bool, np.bool_)) or not 1 <= int(H) <= MAX_SIDE or not 1 <= int(W) <= MAX_SIDE \
            or int(H) * int(W) > 2 ** 31 - 1:
        raise KGLibraryError(f"{fn}: an image of {H} x {W} (1 .. {MAX_SIDE} each, at most 2^31 - 1 pixels)")
    return int(H), int(W)


class RunLengths:
    """Host CSR over the jobs (or the instances): row k owns the runs indptr[k] .. indptr[k + 1] of first and last (0-based, inclusive,
    ascending, in the pixel order p = x * H + y of an H x W image), all int64."""
    __slots__ = ("indptr", "first", "last", "H", "W")

    def __init__(self, indptr, first, last, H, W):
        self.indptr = np.ascontiguousarray(indptr, np.int64).reshape(-1)
        self.first, self.last = (np.ascontiguousarray(a, np.int64).reshape(-1) for a in (first, last))
        self.H, self.W = int(H), int(W)
        k = len(self.first)
        if len(self.indptr) < 1 or self.indptr[0] != 0 or self.indptr[-1] != k or (np.diff(self.indptr) < 0).any() or len(self.last) != k:
            raise KGLibraryError(f"RunLengths: indptr of {len(self.indptr)} entries ending at {self.indptr[-1] if len(self.indptr) else None} "
                                 f"for {k} first and {len(self.last)} last positions")

    def __len__(self):
        return len(self.indptr) - 1

    def __eq__(self, other):
        return isinstance(other, RunLengths) and (self.H, self.W) == (other.H, other.W) \
            and all(np.array_equal(getattr(self, k), getattr(other, k)) for k in ("indptr", "first", "last"))

    __hash__ = None

    def counts(self):
        """int64 [m]: the number of runs of every row"""
        return np.diff(self.indptr)

    def rows(self):
        """int64 [len(first)]: the row every run belongs to"""
        return np.repeat(np.arange(len(self), dtype=np.int64), self.counts())

    def areas(self):
        """int64 [m]: the pixels of every row"""
        out = np.zeros(len(self), np.int64)
        np.add.at(out, self.rows(), self.last - self.first + 1)
        return out

    def slice(self, r0, r1):
        """The RunLengths of rows r0 .. r1 - 1"""
        a, b = int(self.indptr[r0]), int(self.indptr[r1])
        return RunLengths(self.indptr[r0:r1 + 1] - a, self.first[a:b], self.last[a:b], self.H, self.W)

    def of(self, k):
        """int64 [r, 2] of (start, length), start counted from 1: instances.rle_encode's entry"""
        a, b = int(self.indptr[k]), int(self.indptr[k + 1])
        return np.stack([self.first[a:b] + 1, self.last[a:b] - self.first[a:b] + 1], 1).astype(np.int64).reshape(-1, 2)

    def string(self, k):
        """'start length start length ...': the EncodedPixels column of row k"""
        return " ".join(str(int(v)) for v in self.of(k).reshape(-1))

    def coco(self, k):
        """{"size": [H, W], "counts": [...]}: COCO's uncompressed form, alternating runs of zeros and ones in the same column-major
        order, beginning with the zeros (which may be 0); a trailing run of zeros is listed only when it is not empty."""
        a, b = int(self.indptr[k]), int(self.indptr[k + 1])
        f, l = self.first[a:b], self.last[a:b]
        edges = np.stack([f, l + 1], 1).reshape(-1)                  # where the value changes
        n = self.H * self.W
        if len(edges) == 0 or edges[-1] != n:
            edges = np.concatenate([edges, [n]])
        return {"size": [self.H, self.W], "counts": np.diff(np.concatenate([[0], edges])).astype(np.int64).tolist()}

    def to_dict(self, ids=None):
        """{id: of(k)} as instances.rle_encode returns it.  ids: the id of every row (default 1 .. m)."""
        own = _ids("to_dict", ids, len(self))
        return {int(i): self.of(k) for k, i in enumerate(own.tolist())}


def _ids(fn, ids, m):
    own = np.arange(1, m + 1, dtype=np.int64) if ids is None else np.asarray(ids, np.int64).reshape(-1)
    if len(own) != m:
        raise KGLibraryError(f"{fn}: {len(own)} ids for {m} rows")
    return own


# ---- host statements of the semantics ---------------------------------------------------------------------------------------------------

_NONE = (np.zeros(0, np.int64),) * 2


def _job_ends(lab, H, W, job):
    """One map [H, W], one job (id, y1, x1, y2, x2) -> (heads, tails): the positions p, ascending"""
    v, y1, x1, y2, x2 = job
    y1, x1, y2, x2 = max(y1, 0), max(x1, 0), min(y2, H), min(x2, W)
    if y2 <= y1 or x2 <= x1:
        return _NONE
    me = (lab[y1:y2, x1:x2] == v).T                                   # [w, h]: column-major, as p runs
    if not me.any():
        return _NONE
    xs = np.arange(x1, x2)
    prev, nxt = np.empty_like(me), np.empty_like(me)
    prev[:, 1:], nxt[:, :-1] = me[:, :-1], me[:, 1:]
    # the pixel before the top of a column and after its bottom, from the MAP: the row above / below, or the column beside at the wrap
    prev[:, 0] = (lab[y1 - 1, xs] == v) if y1 > 0 else np.where(xs > 0, lab[H - 1, np.maximum(xs - 1, 0)] == v, False)
    nxt[:, -1] = (lab[y2, xs] == v) if y2 < H else np.where(xs < W - 1, lab[0, np.minimum(xs + 1, W - 1)] == v, False)
    p = xs[:, None].astype(np.int64) * H + np.arange(y1, y2, dtype=np.int64)[None]
    return p[me & ~prev], p[me & ~nxt]


def run_counts_host(labels, jobs):
    """kg_label_run_counts in NumPy: labels integers [H, W] or [nimg, H, W]; jobs integers [m, 6] = (img, id, y1, x1, y2, x2)
    -> int32 [m, 2] = {heads, tails}, nothing split."""
    maps = host_stack("run_counts_host", labels)
    nimg, H, W = maps.shape
    j = _labelmaps.host_jobs("run_counts_host", jobs, 6, _JOB_COLUMNS).astype(np.int64)
    out = np.zeros((len(j), 2), np.int32)
    for k, (i, *rest) in enumerate(j.tolist()):
        if 0 <= i < nimg:
            out[k] = [len(a) for a in _job_ends(maps[i], H, W, rest)]
    return out


def run_rows_host(labels, jobs, R, fill=0):
    """kg_label_runs in NumPy: jobs integers [m, 8] = (img, id, y1, x1, y2, x2, head_at, tail_at) -> int32 [R, 2], which starts as `fill`
    everywhere: the k-th head of a job stores p into out[head_at + k][0], the k-th tail into out[tail_at + k][1], each only when the slot
    lies in [0, R)."""
    maps = host_stack("run_rows_host", labels)
    nimg, H, W = maps.shape
    j = _labelmaps.host_jobs("run_rows_host", jobs, 8, _ROW_JOB_COLUMNS).astype(np.int64)
    R = int(R)
    if R < 0:
        raise KGLibraryError(f"run_rows_host: R {R}")
    out = np.full((R, 2), fill, np.int32)
    for i, v, y1, x1, y2, x2, head_at, tail_at in j.tolist():
        if not 0 <= i < nimg:
            continue
        for col, (at, ps) in enumerate(zip((head_at, tail_at), _job_ends(maps[i], H, W, (v, y1, x1, y2, x2)))):
            slot = at + np.arange(len(ps), dtype=np.int64)
            keep = (slot >= 0) & (slot < R)
            out[slot[keep], col] = ps[keep]
    return out


def _paired(fn, per, first, last, H, W):
    """per: int64 [m, 2] = the heads and tails of every job; first / last: all heads / tails in job order -> RunLengths.  The k-th head and
    the k-th tail of a job are a run only when the box holds whole runs: a box that cuts a run of its id is refused where it shows."""
    if (per < 0).any() or (per[:, 0] != per[:, 1]).any() or len(first) != per[:, 0].sum() or len(last) != len(first):
        raise KGLibraryError(f"{fn}: a job whose heads and tails do not pair (its box cuts a run of its id)")
    indptr = np.zeros(len(per) + 1, np.int64)
    np.cumsum(per[:, 0], out=indptr[1:])
    R = len(first)
    inner = np.ones(R, bool)
    inner[indptr[:-1][indptr[:-1] < R]] = False                       # the first run of a job has no run before it
    if (first < 0).any() or (last >= H * W).any() or (first > last).any() or (first[1:] <= last[:-1])[inner[1:]].any():
        raise KGLibraryError(f"{fn}: rows that are no run-length list (first > last, or runs that do not ascend inside a job: a box that "
                             "cuts a run of its id)")
    return RunLengths(indptr, first, last, H, W)


def runs_host(labels, jobs_or_n):
    """labels: integers [H, W] or [nimg, H, W]; jobs_or_n: jobs [m, 6] = (img, id, y1, x1, y2, x2), or the instance count n (one per map
    for a stack): the ids 1 .. n inside their own boxes (labelmetrics.label_stats_host, which raises when a pixel lies outside [0, n])
    -> RunLengths, one row per job, not banded."""
    maps = host_stack("runs_host", labels)
    nimg, H, W = maps.shape
    j = _labelmaps.host_job_table("runs_host", maps, jobs_or_n, labelmetrics.label_stats_host)
    ends = [_job_ends(maps[i], H, W, rest) if 0 <= i < nimg else _NONE for i, *rest in j.tolist()]
    cat = [np.concatenate([e[c] for e in ends]) if ends else np.zeros(0, np.int64) for c in range(2)]
    return _paired("runs_host", np.array([[len(e[0]), len(e[1])] for e in ends], np.int64).reshape(-1, 2), cat[0], cat[1], H, W)


def split_columns(jobs, max_job_pixels=65536):
    """Jobs int [m, 6], clamped -> (pieces int32 [m2, 6], owner int64 [m2]): a job whose box holds more than max_job_pixels pixels becomes
    column bands of the box's full height and max(max_job_pixels // h, 1) columns, in ascending x; owner[k] is the job piece k belongs to,
    ascending."""
    j = np.asarray(jobs, np.int64).reshape(-1, 6)
    cap = int(max_job_pixels)
    if cap < 1:
        raise KGLibraryError(f"split_columns: max_job_pixels {max_job_pixels}")
    h, w = np.maximum(j[:, 4] - j[:, 2], 0), np.maximum(j[:, 5] - j[:, 3], 0)
    cols = np.where(h * w > cap, np.maximum(cap // np.maximum(h, 1), 1), np.maximum(w, 1))
    nb = (np.maximum(w, 1) + cols - 1) // cols                         # bands per job, 1 for a small or an empty box
    owner = np.repeat(np.arange(len(j), dtype=np.int64), nb)
    b = np.arange(len(owner), dtype=np.int64) - np.repeat(np.cumsum(nb) - nb, nb)
    pieces = j[owner]
    cut = nb[owner] > 1
    xa = pieces[:, 3] + b * cols[owner]
    pieces[cut, 5] = np.minimum(xa + cols[owner], pieces[:, 5])[cut]
    pieces[cut, 3] = xa[cut]
    return np.ascontiguousarray(pieces.astype(np.int32)).reshape(-1, 6), owner


# ---- device -----------------------------------------------------------------------------------------------------------------------------

def run_counts(labels, jobs):
    """kg_label_run_counts as it is: labels device int32 [H, W] or [nimg, H, W]; jobs host integers [m, 6] = (img, id, y1, x1, y2, x2)
    (uploaded once) or a device int32 tensor -> device int32 [m, 2] = {heads, tails}.  One launch, no copy back, no synchronisation,
    nothing split."""
    import torch
    from ._lib import ptr, stream_ptr
    lab = device_stack("run_counts", labels)[0]
    nimg, H, W = lab.shape
    jd = _labelmaps.device_jobs("run_counts", jobs, 6, _JOB_COLUMNS, lab.device)
    m = jd.shape[0]
    out = torch.empty(m, 2, dtype=torch.int32, device=lab.device)
    with torch.cuda.device(lab.device):
        _lib.call("kg_label_run_counts", ptr(lab), nimg, H, W, ptr(jd) if m else None, m, ptr(out) if m else None, stream_ptr())
    return out


def run_rows(labels, jobs, R, out=None):
    """kg_label_runs as it is: jobs host integers [m, 8] = (img, id, y1, x1, y2, x2, head_at, tail_at) (uploaded once) or a device int32
    tensor -> device int32 [R, 2] = {first, last}.  out: None (a tensor of zeros is made) or a contiguous device int32 [R, 2] that is
    written in place: only the slots the table names change.  One launch, no copy back, no synchronisation, nothing split."""
    import torch
    from ._lib import ptr, stream_ptr
    lab = device_stack("run_rows", labels)[0]
    nimg, H, W = lab.shape
    jd = _labelmaps.device_jobs("run_rows", jobs, 8, _ROW_JOB_COLUMNS, lab.device)
    m = jd.shape[0]
    R = int(R)
    if not 0 <= R <= 2 ** 31 - 1:
        raise KGLibraryError(f"run_rows: R {R}")
    out = torch.zeros(R, 2, dtype=torch.int32, device=lab.device) if out is None else out_tensor("run_rows", "out", out, (R, 2), torch.int32, lab.device)
    with torch.cuda.device(lab.device):
        _lib.call("kg_label_runs", ptr(lab), nimg, H, W, ptr(jd) if m else None, m, ptr(out) if R else None, R, stream_ptr())
    return out


def _device_runs(lab, j, max_job_pixels):
    """lab: device int32 [nimg, H, W], j: host jobs [m, 6], clamped -> RunLengths.  Two launches, two uploads and two copies back."""
    import torch
    nimg, H, W = lab.shape
    pieces, owner = split_columns(j, max_job_pixels)
    m = len(j)
    if len(pieces) == 0:
        return RunLengths(np.zeros(m + 1, np.int64), [], [], H, W)
    cnt = run_counts(lab, pieces).cpu().numpy().astype(np.int64)
    per = np.zeros((m, 2), np.int64)
    np.add.at(per, owner, cnt)
    none = np.zeros(0, np.int64)
    R = int(per[:, 0].sum())
    if (cnt < 0).any() or (per[:, 0] != per[:, 1]).any() or R == 0:
        return _paired("runs", per, none, none, H, W)                 # raises unless there is no run at all
    if R > 2 ** 31 - 1:
        raise KGLibraryError(f"runs: {R} runs exceed 2^31 - 1")
    table = np.concatenate([pieces.astype(np.int64), np.cumsum(cnt, 0) - cnt], 1)    # pieces are in job order, bands in ascending x
    rows = run_rows(lab, table, R, torch.empty(R, 2, dtype=torch.int32, device=lab.device)).cpu().numpy().astype(np.int64)
    return _paired("runs", per, rows[:, 0], rows[:, 1], H, W)


def runs(labels, n=None, jobs=None, stats=None, max_job_pixels=65536):
    """runs_host on the device -> RunLengths (host).  labels: device int32 [H, W] or [nimg, H, W].  What is listed:
      jobs   host integers [m, 6] = (img, id, y1, x1, y2, x2): one row per job; or
      n      the instance count (one per map for a stack): the ids 1 .. n inside their own boxes.  The boxes come from stats -- host
             integers [n, 5] = (area, y1, x1, y2, x2), one array per map for a stack; columns 1:6 of an Instances table are that -- or,
             without stats, from labelmetrics.label_stats (its launches and one copy per map).
    A job whose box holds more than max_job_pixels pixels is listed in column bands (split_columns).  ONE kg_label_run_counts launch and
    one small copy back, a host prefix over heads and tails, ONE kg_label_runs launch and one copy back: two launches and two copies
    whatever the map holds.  The rows that come back are checked (first <= last, ascending inside every job)."""
    lab = device_stack("runs", labels)[0]
    return _device_runs(lab, _labelmaps.job_table("runs", lab, n, jobs, stats, labelmetrics.label_stats), max_job_pixels)


# ---- Instances ----------------------------------------------------------------------------------------------------------------------------

def _instance_runs(insts, max_job_pixels):
    """-> one RunLengths per entry (None for a None entry); the entries themselves are not touched"""
    out = [None] * len(insts)

    def host_one(i, inst, lab):
        out[i] = runs_host(lab, _labelmaps.instance_jobs(inst, 0, 0, *lab.shape))
    for idx, stack, H, W in _labelmaps.size_batches("runs_instances", insts, host_one):
        got = _device_runs(device_stack("runs_instances", stack)[0], _labelmaps.batch_jobs(insts, idx, 0, H, W), max_job_pixels)
        for i, a, b in _labelmaps.deal(insts, idx):
            out[i] = got.slice(a, b)
    return out


def runs_instances(inst, max_job_pixels=65536):
    """runs for an Instances / TiledInstances -> RunLengths with len(inst) rows: ids 1 .. n, boxes from table[:, 2:6]; an instance with
    no visible pixel gets an empty row.  A host label map (assemble_host's result) goes through runs_host."""
    return _instance_runs([inst], max_job_pixels)[0]


def runs_instances_batch(insts, max_job_pixels=65536):
    """runs_instances for predict_instances' list (entries may be None), in place: every entry's `runs` is set.  ONE pair of launches per
    output size."""
    for v, g in zip(insts, _instance_runs(insts, max_job_pixels)):
        if v is not None:
            v.runs = g
    return insts


# ---- from run-length rows to a label map -------------------------------------------------------------------------------------------------

def _paint_rows(fn, runs, H, W, ids):
    """A RunLengths (with the id of every row, default 1 .. m) or a dict {id: [r, 2] of (start, length)} -> int64 [R, 3] = (first, last,
    value), sorted by first; raises on a run outside the image and on two runs that overlap."""
    H, W = _size(fn, H, W)
    if isinstance(runs, RunLengths):
        if (runs.H, runs.W) != (H, W):
            raise KGLibraryError(f"{fn}: run lengths of a {runs.H} x {runs.W} image for one of {H} x {W}")
        rows = np.stack([runs.first, runs.last, _ids(fn, ids, len(runs))[runs.rows()]], 1)
    elif isinstance(runs, dict):
        if ids is not None:
            raise KGLibraryError(f"{fn}: a dict carries its own ids")
        parts = []
        for i, r in runs.items():
            r = np.asarray(r)
            if r.size and r.dtype.kind not in "iu":
                raise KGLibraryError(f"{fn}: the runs of id {i} must be integers [r, 2] = (start, length)")
            r = r.astype(np.int64).reshape(-1, 2)
            parts.append(np.stack([r[:, 0] - 1, r[:, 0] + r[:, 1] - 2, np.full(len(r), int(i), np.int64)], 1))
        rows = np.concatenate(parts) if parts else np.zeros((0, 3), np.int64)
    else:
        raise KGLibraryError(f"{fn}: a RunLengths or a dict {{id: [r, 2]}}")
    rows = rows.astype(np.int64).reshape(-1, 3)
    if len(rows) and (rows[:, 2].min() < -2 ** 31 or rows[:, 2].max() > 2 ** 31 - 1):
        raise KGLibraryError(f"{fn}: ids must fit int32")
    if ((rows[:, 0] < 0) | (rows[:, 1] < rows[:, 0]) | (rows[:, 1] >= H * W)).any():
        raise KGLibraryError(f"{fn}: a run outside a {H} x {W} image (or of length below 1)")
    rows = rows[np.argsort(rows[:, 0], kind="stable")]
    if (rows[1:, 0] <= rows[:-1, 1]).any():
        raise KGLibraryError(f"{fn}: two runs overlap")
    return rows, H, W


def paint_host(runs, H, W, background=0, ids=None):
    """Run-length rows -> int32 [H, W]: the value of the run that holds the pixel, else background.  runs: a RunLengths (ids: the value of
    every row, default 1 .. m) or a dict {id: [r, 2] of (start, length)} as instances.rle_encode returns.  Raises on a run outside the
    image and on two runs that overlap (Kaggle forbids overlaps)."""
    rows, H, W = _paint_rows("paint_host", runs, H, W, ids)
    flat = np.full(H * W, int(background), np.int32)
    length = rows[:, 1] - rows[:, 0] + 1
    at = np.repeat(rows[:, 0] - (np.cumsum(length) - length), length) + np.arange(int(length.sum()), dtype=np.int64)
    flat[at] = np.repeat(rows[:, 2], length)
    return np.ascontiguousarray(flat.reshape(W, H).T)


def paint(runs, H, W, device, background=0, ids=None):
    """paint_host on the device -> device int32 [H, W].  The host sorts and checks the rows; one upload, ONE kg_runs_paint launch, no copy
    back: ground truth or a submission reaches labelmetrics.LabelEvaluator without a host label map."""
    import torch
    from ._lib import ptr, stream_ptr
    rows, H, W = _paint_rows("paint", runs, H, W, ids)
    if isinstance(background, (bool, np.bool_)) or not -2 ** 31 <= int(background) <= 2 ** 31 - 1:
        raise KGLibraryError(f"paint: background {background!r} must fit int32")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise KGLibraryError("paint (MI355X build) needs a GPU device; the host route is paint_host")
    rd = _labelmaps.upload_jobs(rows, dev)
    out = torch.empty(H, W, dtype=torch.int32, device=rd.device)
    with torch.cuda.device(rd.device):
        _lib.call("kg_runs_paint", ptr(rd) if len(rows) else None, len(rows), H, W, int(background), ptr(out), stream_ptr())
    return out


def parse_string(s):
    """'start length start length ...' -> int64 [r, 2]: the inverse of RunLengths.string and instances.rle_string"""
    tok = str(s).split()
    try:
        v = np.array([int(t) for t in tok], np.int64)
    except ValueError:
        raise KGLibraryError(f"parse_string: {s!r} is not a list of integers") from None
    if len(v) % 2:
        raise KGLibraryError(f"parse_string: {len(v)} numbers do not pair into (start, length)")
    return v.reshape(-1, 2)


def submission_rows(image_id, runs):
    """The (ImageId, EncodedPixels) rows of a Kaggle submission for one image: one per non-empty row of a RunLengths, in row order."""
    if not isinstance(runs, RunLengths):
        raise KGLibraryError("submission_rows: a RunLengths")
    return [(image_id, runs.string(k)) for k in np.flatnonzero(runs.counts()).tolist()]
