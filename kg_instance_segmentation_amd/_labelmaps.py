"""The argument layer the label-map modules share (instances, tiling, labelmetrics, components, measure, neighbours, runlengths, contours, split, texture): label maps
and job tables, host or device.  fn is the public function the message names."""
import numpy as np

from . import _lib

KGLibraryError = _lib.KGLibraryError


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
