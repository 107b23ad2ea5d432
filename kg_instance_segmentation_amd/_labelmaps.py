"""The argument and batch layer of the label-map modules (instances, tiling, labelmetrics, polygons, components, measure, distance,
neighbours, runlengths, contours, hulls, intensity, split, texture, thinning, boundaries, crops, linking), one owner per rule.  fn is the public function the message names.

    maps       host_maps, device_maps; with the side bound: MAX_SIDE, side, host_stack, device_stack
    job tables host_jobs, upload_jobs, device_jobs, instance_jobs, batch_jobs; counts, jobs_from_stats, and the n / jobs / stats arguments
               of every per-job function: job_table (device entries), host_job_table (the *_host entries)
    images     host_image, device_image, host_pixels; maps and image together: host_args, device_args; job_rows, the launcher of the
               entries that take (labels, image, jobs); check_cap
    outputs    out_tensor
    Instances  check_instances, instance_stats, host_labels
    batches    size_groups, size_batches (the walk over predict_instances' list, one stack per output size), deal"""
import numpy as np

from . import _lib
from .instances import Instances

KGLibraryError = _lib.KGLibraryError
MAX_SIDE = 32768
MAX_CHANNELS = 4
JOB_COLUMNS = "(img, id, y1, x1, y2, x2)"
SUMS_FIT = "the bound that keeps every sum inside int64"           # why measure, and what reads an image like it, bounds the sides


def is_device(t):
    import torch
    return torch.is_tensor(t) and t.device.type == "cuda"


def _words(stack):
    return ("label maps", "[H, W] or [nimg, H, W]", (2, 3)) if stack else ("a label map", "[H, W]", (2,))


def host_maps(fn, labels, stack):
    """stack=False: one map [H, W] -> the array.  stack=True: [H, W] or [nimg, H, W] of at most 2^31 - 1 elements ->
    ([nimg, H, W], was_2d)."""
    what, shape, ndims = _words(stack)
    lab = np.asarray(labels)
    if lab.ndim not in ndims or lab.dtype.kind not in "iu" or lab.size == 0:
        raise KGLibraryError(f"{fn}: {what} must be a non-empty integer array {shape}")
    if not stack:
        return lab
    if lab.size > 2 ** 31 - 1:
        raise KGLibraryError(f"{fn}: nimg * H * W exceeds 2^31 - 1")
    return lab.reshape((-1,) + lab.shape[-2:]), lab.ndim == 2


def device_maps(fn, t, stack, like=None):
    """The same for a device int32 tensor -> the tensor, contiguous, in its own shape; like: a tensor whose shape and device it must
    share."""
    import torch
    what, shape, ndims = _words(stack)
    if not is_device(t):
        raise KGLibraryError(f"{fn} (MI355X build) needs the label map{'s' if stack else ''} on a GPU device; the host route is {fn}_host")
    if t.dtype != torch.int32 or t.dim() not in ndims or t.numel() == 0:
        raise KGLibraryError(f"{fn}: {what} must be a non-empty int32 tensor {shape}")
    if stack and t.numel() > 2 ** 31 - 1:
        raise KGLibraryError(f"{fn}: nimg * H * W exceeds 2^31 - 1")
    if like is not None and (t.shape != like.shape or t.device != like.device):
        raise KGLibraryError(f"{fn}: tensors of {tuple(t.shape)} and {tuple(like.shape)} must have one shape and one device")
    return t.contiguous()


def side(fn, maps, why=""):
    """[..., H, W] maps (host or device) as they came, once their sides are known to fit; why: what the caller's bound protects"""
    H, W = maps.shape[-2:]
    if H > MAX_SIDE or W > MAX_SIDE:
        raise KGLibraryError(f"{fn}: a map of {H} x {W} exceeds {MAX_SIDE}{' (' + why + ')' if why else ''}")
    return maps


def host_stack(fn, labels, why=""):
    """host_maps of a stack within the side bound -> [nimg, H, W]"""
    return side(fn, host_maps(fn, labels, True)[0], why)


def device_stack(fn, t, why="", bound=True):
    """device_maps of a stack -> (the tensor as [nimg, H, W], the caller's shape); bound=False: the entry has no side bound"""
    t = device_maps(fn, t, True)
    lab = t.view((-1,) + t.shape[-2:])
    return (side(fn, lab, why) if bound else lab), t.shape


def host_jobs(fn, jobs, ncol, names, rows="m"):
    """A host job table: integers [rows, ncol] that fit int32 -> the array as it came."""
    j = np.asarray(jobs)
    if j.ndim != 2 or j.shape[1] != ncol or j.dtype.kind not in "iu" or (j.size and (j.min() < -2 ** 31 or j.max() > 2 ** 31 - 1)):
        raise KGLibraryError(f"{fn}: jobs must be integers [{rows}, {ncol}] = {names} that fit int32")
    return j


def upload_jobs(j, dev):
    """A validated host job table [m, ncol] -> device int32 [m, ncol]: one ops.h2d, or an empty tensor when m == 0."""
    import torch
    from . import ops
    if len(j) == 0:
        return torch.empty(0, j.shape[1], dtype=torch.int32, device=dev)
    return ops.h2d(np.ascontiguousarray(j, np.int32), dev)


def device_jobs(fn, jobs, ncol, names, dev, rows="m", owner="maps'"):
    """A job table, host integers (validated by host_jobs, uploaded once) or a device int32 tensor -> device int32 [rows, ncol] on dev."""
    import torch
    if torch.is_tensor(jobs):
        if jobs.dtype != torch.int32 or jobs.dim() != 2 or jobs.shape[1] != ncol or jobs.device != dev:
            raise KGLibraryError(f"{fn}: device jobs must be int32 [{rows}, {ncol}] on the {owner} device")
        return jobs.contiguous()
    return upload_jobs(host_jobs(fn, jobs, ncol, names, rows), dev)


def instance_jobs(inst, img, grow, H, W):
    """int64 [n, 6]: ids 1 .. n of image img, boxes from the table grown by `grow` and clamped; an instance with no visible pixel gets an
    empty box, hence an empty row."""
    t = np.asarray(inst.table, np.int64).reshape(-1, 8)
    n = len(t)
    box = t[:, 2:6] + [-grow, -grow, grow, grow]
    box[:, :2] = np.clip(box[:, :2], 0, [H, W]); box[:, 2:] = np.clip(box[:, 2:], 0, [H, W])
    box = np.where(t[:, 1:2] > 0, box, 0)
    return np.concatenate([np.full((n, 1), int(img)), np.arange(1, n + 1)[:, None], box], 1).astype(np.int64).reshape(-1, 6)


def batch_jobs(insts, idx, grow, H, W):
    """instance_jobs of the entries idx of one stack: entry idx[k] is image k"""
    return np.concatenate([instance_jobs(insts[i], k, grow, H, W) for k, i in enumerate(idx)])


def jobs_from_stats(stats, img=0):
    """stats: integers [n, 5] = (area, y1, x1, y2, x2) of the ids 1 .. n of image `img` (labelmetrics.STATS_COLUMNS; columns 1:6 of an
    Instances table) -> int32 [n, 6] jobs.  An id with area 0 gets an empty box, hence a row of zeros."""
    s = np.asarray(stats)
    if s.ndim != 2 or s.shape[1] != 5 or s.dtype.kind not in "iu":
        raise KGLibraryError("jobs_from_stats: stats must be integers [n, 5] = (area, y1, x1, y2, x2)")
    s = s.astype(np.int64)
    box = np.where(s[:, :1] > 0, s[:, 1:], 0)
    n = len(s)
    return np.ascontiguousarray(np.concatenate([np.full((n, 1), int(img)), np.arange(1, n + 1)[:, None], box], 1).astype(np.int32)).reshape(-1, 6)


def counts(fn, n, nimg):
    """the instance count n, one per map for a stack -> a list of nimg counts"""
    ns = [int(n)] if np.ndim(n) == 0 else [int(v) for v in n]
    if len(ns) != nimg or any(v < 0 for v in ns):
        raise KGLibraryError(f"{fn}: {len(ns)} instance count(s) for {nimg} label map(s)")
    return ns


def job_table(fn, maps, n, jobs, stats, stats_of):
    """The n / jobs / stats arguments of a per-job function over maps [nimg, H, W] -> int64 [m, 6] jobs, clamped to the map (so that a
    band rule sees the pixels a job really holds; a job of a bad image keeps its index and gets its empty row).  jobs: integers [m, 6];
    or n, the instance count (one per map for a stack), with the boxes from stats -- [n, 5], one array per map for a stack -- or, without
    stats, from stats_of(map, n) (labelmetrics.label_stats or label_stats_host)."""
    nimg, H, W = maps.shape
    if jobs is not None:
        if n is not None or stats is not None:
            raise KGLibraryError(f"{fn}: jobs cannot be given together with n / stats")
        j = host_jobs(fn, jobs, 6, JOB_COLUMNS).astype(np.int64)
    else:
        if n is None:
            raise KGLibraryError(f"{fn}: the instance count n or a job table is needed")
        ns = counts(fn, n, nimg)
        if stats is None:
            per = [stats_of(maps[i], ns[i]) for i in range(nimg)]
        else:
            per = [stats] if nimg == 1 and np.ndim(stats) == 2 else list(stats)
            if len(per) != nimg or any(len(np.asarray(s)) != k for s, k in zip(per, ns)):
                raise KGLibraryError(f"{fn}: stats must be [n, 5] per label map ({nimg} map(s), counts {ns})")
        j = np.concatenate([jobs_from_stats(s, i) for i, s in enumerate(per)]).astype(np.int64).reshape(-1, 6)
    j = j.copy()
    j[:, 2:4] = np.clip(j[:, 2:4], 0, [H, W]); j[:, 4:6] = np.clip(j[:, 4:6], 0, [H, W])
    return j


def host_job_table(fn, maps, jobs_or_n, stats_of):
    """The jobs_or_n argument of a *_host function -> job_table's result.  jobs [m, 6] or the instance count(s); an empty list is no
    jobs, as jobs=[] of the device functions."""
    if np.ndim(jobs_or_n) == 2 or (np.ndim(jobs_or_n) == 1 and np.size(jobs_or_n) == 0):
        return job_table(fn, maps, None, jobs_or_n if np.size(jobs_or_n) else np.zeros((0, 6), np.int64), None, None)
    return job_table(fn, maps, jobs_or_n, None, None, stats_of)


# ---- images ---------------------------------------------------------------------------------------------------------------------------

def host_image(fn, image, shape):
    """-> [nimg, H, W, C] or None"""
    if image is None:
        return None
    a = np.asarray(image)
    if a.dtype not in (np.uint8, np.uint16):
        raise KGLibraryError(f"{fn}: the image must be uint8 or uint16, not {a.dtype}")
    if a.ndim == 3 and shape[0] == 1:
        a = a[None]
    if a.ndim != 4 or a.shape[:3] != tuple(shape) or not 1 <= a.shape[3] <= MAX_CHANNELS:
        raise KGLibraryError(f"{fn}: an image of {a.shape} for label maps of {tuple(shape)}: [nimg, H, W, C] with 1 <= C <= {MAX_CHANNELS}")
    return a


def device_image(fn, image, shape, dev):
    """host array (uploaded once) or device tensor -> device tensor [nimg, H, W, C], or None"""
    import torch
    from . import ops
    if image is None:
        return None
    if not torch.is_tensor(image):
        a = host_image(fn, image, shape)
        if a.dtype == np.uint16:                                       # the bytes travel as int16; the kernel reads them unsigned
            return ops.h2d(np.ascontiguousarray(a).view(np.int16), dev)
        return ops.h2d(np.ascontiguousarray(a), dev)
    t = image
    if t.dtype not in (torch.uint8, torch.int16, getattr(torch, "uint16", torch.int16)) or t.device != dev:
        raise KGLibraryError(f"{fn}: a device image must be uint8 or uint16 (int16 storage is read as uint16) on the maps' device")
    if t.dim() == 3 and shape[0] == 1:
        t = t[None]
    if t.dim() != 4 or tuple(t.shape[:3]) != tuple(shape) or not 1 <= t.shape[3] <= MAX_CHANNELS:
        raise KGLibraryError(f"{fn}: an image of {tuple(t.shape)} for label maps of {tuple(shape)}: [nimg, H, W, C] with 1 <= C <= {MAX_CHANNELS}")
    return t.contiguous()


def host_pixels(image):
    """An image that may be a tensor -> what host_image takes: a tensor comes back to the host, int16 storage read as uint16"""
    import torch
    if torch.is_tensor(image):
        image = image.cpu().numpy()
        image = image.view(np.uint16) if image.dtype == np.int16 else image
    return image


def host_args(fn, labels, image):
    """-> (maps [nimg, H, W], image [nimg, H, W, C]) of a *_host function that needs an image"""
    maps = host_stack(fn, labels, SUMS_FIT)
    img = host_image(fn, image, maps.shape)
    if img is None:
        raise KGLibraryError(f"{fn}: an image is needed")
    return maps, img


def device_args(fn, labels, image):
    """the same on the device: a host image is uploaded once"""
    lab = device_stack(fn, labels, SUMS_FIT)[0]
    if image is None:
        raise KGLibraryError(f"{fn}: an image is needed")
    return lab, device_image(fn, image, lab.shape, lab.device)


def job_rows(entry, lab, img, jd, extra, shape):
    """One launch of an entry (labels, nimg, H, W, image, channels, elem_bytes, jobs, m, *extra, out, stream) -> device int32 [m, *shape]"""
    import torch
    from ._lib import ptr, stream_ptr
    nimg, H, W = lab.shape
    m = jd.shape[0]
    out = torch.empty((m,) + shape, dtype=torch.int32, device=lab.device)
    with torch.cuda.device(lab.device):
        _lib.call(entry, ptr(lab), nimg, H, W, ptr(img), img.shape[3], img.element_size(), ptr(jd) if m else None, m, *extra,
                  ptr(out) if m else None, stream_ptr())
    return out


def check_cap(fn, max_job_pixels):
    if int(max_job_pixels) < 1:
        raise KGLibraryError(f"{fn}: max_job_pixels {max_job_pixels}")
    return int(max_job_pixels)


def out_tensor(fn, what, t, shape, dtype, dev):
    """An output the caller passes in: a contiguous device tensor of exactly this shape and dtype on dev -> the tensor"""
    if not is_device(t) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != dev or not t.is_contiguous():
        raise KGLibraryError(f"{fn}: {what} must be a contiguous {str(dtype).replace('torch.', '')} {list(shape)} tensor on the maps' device")
    return t


# ---- Instances --------------------------------------------------------------------------------------------------------------------------

def check_instances(fn, inst):
    if not isinstance(inst, Instances):
        raise KGLibraryError(f"{fn}: an Instances or a TiledInstances")
    if np.asarray(inst.table).shape != (len(inst), 8):
        raise KGLibraryError(f"{fn}: a table of {np.asarray(inst.table).shape} for {len(inst)} instances")


def instance_stats(fn, inst):
    """-> int64 [n, 5] = (area, y1, x1, y2, x2): columns 1:6 of the table, job_table's stats"""
    if not isinstance(inst, Instances):
        raise KGLibraryError(f"{fn}: an Instances or a TiledInstances")
    stats = np.asarray(inst.table, np.int64).reshape(-1, 8)[:, 1:6]
    if len(stats) != len(inst):
        raise KGLibraryError(f"{fn}: a table of {len(stats)} rows for {len(inst)} instances")
    return stats


def host_labels(inst):
    """the label map of an Instances that is not on a GPU device, as an array"""
    import torch
    return inst.labels.numpy() if torch.is_tensor(inst.labels) else np.asarray(inst.labels)


# ---- batches: predict_instances' list, one stack per output size ------------------------------------------------------------------------

def size_groups(image_sizes):
    """Images grouped by output size, in order of first appearance: [((h, w), [image indices])]."""
    groups = {}
    for i, hw in enumerate(image_sizes):
        groups.setdefault((int(hw[0]), int(hw[1])), []).append(i)
    return list(groups.items())


def size_batches(fn, insts, host_one=None):
    """The walk over predict_instances' list (entries may be None).  Every entry is checked first; an entry whose label map is not on
    a GPU device goes to host_one(i, inst, its label map as an array), once each and in order (without host_one it is refused); then, per
    output size in order of first appearance, comes (idx, stack, H, W): the entries of that size and their label maps as ONE device
    tensor [len(idx), H, W], so that a caller launches once per size."""
    import torch
    todo = [i for i, v in enumerate(insts) if v is not None]
    for i in todo:
        check_instances(fn, insts[i])
    host = [i for i in todo if not is_device(insts[i].labels)]
    if host and host_one is None:
        raise KGLibraryError(f"{fn} (MI355X build) needs the label maps on a GPU device")
    for i in host:
        host_one(i, insts[i], host_labels(insts[i]))
    todo = [i for i in todo if i not in host]
    for (H, W), members in size_groups([tuple(insts[i].labels.shape) for i in todo]):
        idx = [todo[k] for k in members]
        yield idx, (insts[idx[0]].labels[None] if len(idx) == 1 else torch.stack([insts[i].labels for i in idx])), H, W


def deal(insts, idx, rows=None):
    """(i, r, r + k) for every entry i of idx: the rows of a stacked result that are entry i's, k = len(insts[i]) or rows[position]"""
    r = 0
    for p, i in enumerate(idx):
        k = len(insts[i]) if rows is None else int(rows[p])
        yield i, r, r + k
        r += k
