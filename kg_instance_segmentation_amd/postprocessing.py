"""Drop-in `postprocessing` module (reference postprocessing.py) on the float64 HIP pipeline.

Hough vote -> Gaussian -> peaks -> greedy keypoint-graph grouping run on the GPU with the
reference's exact float64 arithmetic and summation order; only the (tiny) skeleton list is copied to
the host, where the reference's list-of-ndarray return types are rebuilt."""
import numpy as np
import torch

from . import _lib, ops
from ._lib import ptr, stream_ptr, c_double, c_long

PEAK_THRESH = 0.004   # postprocessing.py:145
_STREAMS = {}


class _Workspace:
    cache = {}

    @classmethod
    def get(cls, H, W, dev, peak_cap, skel_cap):
        key = (H, W, str(dev), peak_cap, skel_cap)
        ws = cls.cache.get(key)
        if ws is None:
            nbytes = _lib.load().kg_postproc_workspace_bytes(H, W, peak_cap, skel_cap)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            cls.cache[key] = ws
        return ws


def caps(H, W):
    """(peak_cap, skel_cap) of an H x W map.  Beyond 65 536 peaks per map the later peaks in scan order (channel, row, column) are dropped
    without an error."""
    peak_cap = min(5 * H * W, 1 << 16)
    return peak_cap, peak_cap


def skeletons_device(kp, short, mid, debug=False):
    """kp [.,5,H,W], short [.,10,H,W], mid [.,40,H,W] device fp32 (batch element 0 is used,
    postprocessing.py:138-140).  Returns (skel [cap,5,3] f64 device, nskel int32[1] device[, debug dict])."""
    if not kp.is_cuda:
        raise _lib.KGLibraryError("postprocessing (MI355X build) needs GPU tensors")
    kp0 = kp.detach()[0].contiguous().float(); sh0 = short.detach()[0].contiguous().float(); md0 = mid.detach()[0].contiguous().float()
    _, H, W = kp0.shape
    dev = kp0.device
    peak_cap, skel_cap = caps(H, W)
    ws = _Workspace.get(H, W, dev, peak_cap, skel_cap)
    skel = torch.empty(skel_cap, 5, 3, dtype=torch.float64, device=dev)
    nsk = torch.zeros(1, dtype=torch.int32, device=dev)
    dbg = None
    args = [None] * 5
    if debug:
        dbg = {"heat": torch.empty(5, H, W, dtype=torch.float64, device=dev), "blur": torch.empty(5, H, W, dtype=torch.float64, device=dev),
               "peaks": torch.empty(3, peak_cap, dtype=torch.int32, device=dev), "conf": torch.empty(peak_cap, dtype=torch.float64, device=dev),
               "npeaks": torch.zeros(1, dtype=torch.int32, device=dev)}
        args = [ptr(dbg["heat"]), ptr(dbg["blur"]), ptr(dbg["peaks"]), ptr(dbg["conf"]), ptr(dbg["npeaks"])]
    with torch.cuda.device(dev):      # (launch on the tensors' device, whatever the "current" one is)
        _lib.call("kg_postproc_scale", ptr(kp0), ptr(sh0), ptr(md0), H, W, c_double(PEAK_THRESH), ptr(ws), c_long(ws.numel()), peak_cap,
                  skel_cap, ptr(skel), ptr(nsk), *args, stream_ptr())
    return (skel, nsk, dbg) if debug else (skel, nsk)


def get_skeletons_and_masks(kp_maps, short_offsets, mid_offsets):
    """== postprocessing.get_skeletons_and_masks (postprocessing.py:129-147): list of 5x3 float64 arrays."""
    skel, nsk = skeletons_device(kp_maps, short_offsets, mid_offsets)
    n = int(nsk.item())
    if n > skel.shape[0]:
        raise _lib.KGLibraryError(f"skeleton capacity exceeded ({n} > {skel.shape[0]})")
    host = skel[:n].cpu().numpy()
    return [host[i].copy() for i in range(n)]


def refine_skeleton(skeletons):
    """postprocessing.py:150-159 (host: a few hundred 5x3 arrays)."""
    out = []
    for s in skeletons:
        mask = s[:, 0] > 0.
        if mask.sum() >= 3 or mask[[0, 3]].sum() == 2 or mask[[1, 2]].sum() == 2:
            out.append(s)
    return out


def _boxes_device(skel_list, scale, boxes, nbox, cap, dev):
    n = len(skel_list)
    if n == 0:
        return
    sk = torch.from_numpy(np.ascontiguousarray(np.asarray(skel_list, np.float64).reshape(n, 15))).to(dev)
    ns = torch.tensor([n], dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.call("kg_skeleton_boxes", ptr(sk), ptr(ns), n, c_double(scale), 0, ptr(boxes), ptr(nbox), cap, stream_ptr())


def skeleton_to_box(skeletons, scale):
    """postprocessing.py:164-242 -> list of [y1,x1,y2,x2,conf]; scales the skeletons in place like the reference."""
    if len(skeletons) == 0:
        return []
    dev = torch.device("cuda", torch.cuda.current_device())
    cap = len(skeletons)
    boxes = torch.empty(cap, 5, dtype=torch.float64, device=dev)
    nbox = torch.zeros(1, dtype=torch.int32, device=dev)
    _boxes_device(skeletons, scale, boxes, nbox, cap, dev)
    k = int(nbox.item())
    for s in skeletons:
        s[:, :2] *= scale
    return [list(r) for r in boxes[:k].cpu().numpy()]


def gather_skeleton(skeleton0, skeleton1, skeleton2, skeleton3):
    """postprocessing.py:255-261: boxes of the four scales concatenated (N x 5 float64, or shape (0,))."""
    b = skeleton_to_box(skeleton0, 1) + skeleton_to_box(skeleton1, 2) + skeleton_to_box(skeleton2, 4) + skeleton_to_box(skeleton3, 8)
    return np.asarray(b)


def gather_skeleton_single(skeleton0, skeleton1, skeleton2, skeleton3):
    return (np.asarray(skeleton_to_box(skeleton0, 1)), np.asarray(skeleton_to_box(skeleton1, 2)),
            np.asarray(skeleton_to_box(skeleton2, 4)), np.asarray(skeleton_to_box(skeleton3, 8)))


def detect(dec, nms_thresh=0.5, timing=None):
    """Fused test.py:105-116: four scales -> refine -> boxes -> NMS with a single device->host copy.
    dec = ([kp,short,mid] x 4).  Returns N x 5 float64 ndarray or None.  timing (dict, measurement hook of bench.py): receives
    "boxes_nms_ms", the GPU time of the box assembly + NMS launches."""
    from . import nms as _nms
    dev = dec[0][0].device
    # the scales are independent and the greedy grouping of a scale is ONE workgroup: run them on separate streams -- the caller's
    # stream for the first (largest) scale + 3 side streams = 4, the number of hardware queues a process gets by default (a fifth
    # stream shares a queue with another one and its scale runs after that one's grouping instead of beside it)
    main = torch.cuda.current_stream(dev)
    pool = _STREAMS.setdefault(str(dev), [torch.cuda.Stream(dev) for _ in range(3)])
    ready = main.record_event()            # the head maps are complete here; the side streams start from this point
    sks, by_key, used = [], {}, []
    for i, d in enumerate(dec):
        key = tuple(d[0].shape[-2:])
        if key not in by_key:              # equal sizes share one cached workspace: they stay on one stream, in order
            by_key[key] = None if not by_key else pool[(len(by_key) - 1) % 3]
        st = by_key[key]
        if st is None:
            sks.append(skeletons_device(*d))
            continue
        if st not in used:
            st.wait_event(ready)
            used.append(st)
        with torch.cuda.stream(st):
            r = skeletons_device(*d)
        for t in r:
            t.record_stream(main)
        sks.append(r)
    for st in used:
        main.wait_stream(st)
    cap = sum(s[0].shape[0] for s in sks)
    cap = min(cap, 1 << 15)
    boxes = torch.empty(cap, 5, dtype=torch.float64, device=dev)
    nbox = torch.zeros(1, dtype=torch.int32, device=dev)
    if timing is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    for (skel, nsk), scale in zip(sks, (1, 2, 4, 8)):
        with torch.cuda.device(dev):
            _lib.call("kg_skeleton_boxes", ptr(skel), ptr(nsk), skel.shape[0], c_double(scale), 1, ptr(boxes), ptr(nbox), cap, stream_ptr())
    out, nk = _nms.nms_device(boxes, nbox, cap, float(nms_thresh))
    if timing is not None:
        e1.record()
    k = int(nk.item())
    if timing is not None:
        timing["boxes_nms_ms"] = e0.elapsed_time(e1)
    if k == 0:
        return None
    return out[:k].cpu().numpy()


# ---- batched detection (test.py:105-116 for a batch of images) -------------------------------------------------------------------------
BATCH_WORKSPACE_BYTES = 8 << 30   # default budget of detect_batch: post-processing workspace (all scales) of the images processed together


class _BatchWorkspace:
    """One workspace per (H, W, device) for kg_postproc_batch, grown to the largest image count seen."""
    cache = {}

    @classmethod
    def get(cls, H, W, dev, n):
        need = _lib.load().kg_postproc_batch_workspace_bytes(n, H, W, *caps(H, W))
        if need < 0:
            raise _lib.KGLibraryError(_lib.load().kg_last_error().decode())
        key = (H, W, str(dev))
        ws = cls.cache.get(key)
        if ws is None or ws.numel() < need:
            if ws is not None:
                torch.cuda.synchronize(dev)     # (the old one may still be in use on a side stream: let it finish before it is freed)
            cls.cache.pop(key, None)
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            cls.cache[key] = ws
        return ws


def image_workspace_bytes(sizes):
    """Post-processing workspace of ONE image over its scales of the given (H, W) sizes (equal sizes share a workspace)."""
    lib = _lib.load()
    return sum(lib.kg_postproc_workspace_bytes(H, W, *caps(H, W)) for H, W in dict.fromkeys(sizes))


def plan_chunks(n, per_image_bytes, budget):
    """Consecutive [start, stop) ranges covering n images, each of at most max(1, budget // per_image_bytes) images."""
    k = n if per_image_bytes <= 0 else max(1, min(n, int(budget) // int(per_image_bytes)))
    return [(a, min(n, a + k)) for a in range(0, n, max(k, 1))]


def skeletons_batch_device(kp, short, mid):
    """kp [n,5,H,W], short [n,10,H,W], mid [n,40,H,W] contiguous fp32 device -> (skel [n,cap,5,3] f64, nskel int32 [n]), all on device."""
    n, _, H, W = kp.shape
    dev = kp.device
    peak_cap, skel_cap = caps(H, W)
    ws = _BatchWorkspace.get(H, W, dev, n)
    skel = torch.empty(n, skel_cap, 5, 3, dtype=torch.float64, device=dev)
    nsk = torch.empty(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.call("kg_postproc_batch", ptr(kp), ptr(short), ptr(mid), n, H, W, c_double(PEAK_THRESH), ptr(ws), c_long(ws.numel()), peak_cap,
                  skel_cap, ptr(skel), ptr(nsk), stream_ptr())
    return skel, nsk


def _detect_chunk(dec, nms_thresh):
    """detect() for the n images of dec (four scales of [n,C,H,W] contiguous fp32): (kept rows [n*cap,5] f64, nkeep int32 [n]) on device,
    the kept rows of image i after those of images 0 .. i-1."""
    from ctypes import c_void_p, c_int
    n = dec[0][0].shape[0]
    dev = dec[0][0].device
    # the stream arrangement of detect(): the caller's stream for the first scale + 3 side streams, now each launch covering the n images
    main = torch.cuda.current_stream(dev)
    pool = _STREAMS.setdefault(str(dev), [torch.cuda.Stream(dev) for _ in range(3)])
    ready = main.record_event()
    sks, by_key, used = [], {}, []
    for d in dec:
        key = tuple(d[0].shape[-2:])
        if key not in by_key:
            by_key[key] = None if not by_key else pool[(len(by_key) - 1) % 3]
        st = by_key[key]
        if st is None:
            sks.append(skeletons_batch_device(*d))
            continue
        if st not in used:
            st.wait_event(ready)
            used.append(st)
        with torch.cuda.stream(st):
            r = skeletons_batch_device(*d)
        for t in r:
            t.record_stream(main)
        sks.append(r)
    for st in used:
        main.wait_stream(st)
    ns = len(sks)
    cap = min(sum(s[0].shape[1] for s in sks), 1 << 15)
    boxes = torch.empty(n, cap, 5, dtype=torch.float64, device=dev)
    nbox = torch.empty(n, dtype=torch.int32, device=dev)
    lib = _lib.load()
    nws = lib.kg_nms_batch_workspace_bytes(n, cap)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    out = torch.empty(n * cap, 5, dtype=torch.float64, device=dev)
    nk = torch.empty(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.call("kg_skeleton_boxes_batch", n, ns, (c_void_p * ns)(*[s[0].data_ptr() for s in sks]), (c_void_p * ns)(*[s[1].data_ptr() for s in sks]),
                  (c_int * ns)(*[s[0].shape[1] for s in sks]), (c_double * ns)(*(1, 2, 4, 8)[:ns]), 1, ptr(boxes), ptr(nbox), cap, stream_ptr())
        _lib.call("kg_nms_batch", n, ptr(boxes), ptr(nbox), cap, c_double(float(nms_thresh)), ptr(ws), c_long(nws), ptr(out), ptr(nk), stream_ptr())
    return out, nk


def detect_batch(dec, nms_thresh=0.5, max_workspace_bytes=None):
    """detect() for every image of a batch: dec = ([kp, short, mid] x 4) with a leading image dimension N (forward_dec's outputs).
    Returns a list of N entries, entry i == detect() on image i alone (N x 5 float64 ndarray, or None).  One launch per stage and scale
    covers all images of a chunk; chunks hold at most max_workspace_bytes (default BATCH_WORKSPACE_BYTES) of workspace, at least one image.
    The host reads the kept-box counts and the kept rows of the whole batch in two copies."""
    if not dec[0][0].is_cuda:
        raise _lib.KGLibraryError("postprocessing (MI355X build) needs GPU tensors")
    if len(dec) > 4:
        raise _lib.KGLibraryError("detect_batch: at most four scales")
    dec = [[t.detach().contiguous().float() for t in d] for d in dec]
    N = dec[0][0].shape[0]
    if any(t.shape[0] != N for d in dec for t in d):
        raise _lib.KGLibraryError("detect_batch: every head map needs the same number of images")
    if N == 0:
        return []
    budget = BATCH_WORKSPACE_BYTES if max_workspace_bytes is None else max_workspace_bytes
    chunks = plan_chunks(N, image_workspace_bytes([tuple(d[0].shape[-2:]) for d in dec]), budget)
    res = [_detect_chunk([[t[a:b] for t in d] for d in dec], nms_thresh) for a, b in chunks]
    nk = torch.cat([r[1] for r in res]).cpu().numpy().astype(np.int64)                  # copy 1: kept boxes per image
    tot = [int(nk[a:b].sum()) for a, b in chunks]
    rows = torch.cat([r[0][:t] for r, t in zip(res, tot)]).cpu().numpy() if sum(tot) else np.zeros((0, 5))   # copy 2: the kept rows
    starts = np.concatenate([[0], np.cumsum(nk)])
    return [rows[starts[i]:starts[i + 1]].copy() if nk[i] else None for i in range(N)]


def paste_masks(predictions, input_h, input_w, image_w, image_h, seg_thresh, device_u8=False, packed=False):
    """== the reference driver's `post_processing` (test.py:127-157) for the predictions of `model.forward_seg`: every mask patch is
    resized to its (rounded, clamped) box, pasted into an (input_h, input_w) canvas, resized to the image and thresholded -- in one
    kernel launch for all detections (kg_mask_paste) instead of two cv2.resize calls and a full-size host array per detection.
    Returns [masks float32 [n, image_h, image_w] in {0, 1}, dets float32 [n, 5] = (y1, x1, y2, x2, conf) in image pixels] like the
    reference, or None; device_u8=True keeps the masks on the GPU as bytes (what eval_parts.seg_evaluation consumes), packed=True as a
    bitmasks.BitMasks (one bit per pixel, kg_mask_paste_bits: the same pixels in 1/8 of the bytes)."""
    if predictions is None:
        return None
    meta = getattr(predictions, "kg_meta", None)
    if meta is None:
        raise _lib.KGLibraryError("paste_masks needs the predictions object returned by this package's forward_seg")
    return paste_rows(meta["flat"], meta["off"], meta["h"], meta["w"], meta["boxes"], input_h, input_w, image_w, image_h, seg_thresh, device_u8,
                      packed)


def paste_rows(flat, off, h, w, boxes, input_h, input_w, image_w, image_h, seg_thresh, device_u8=False, packed=False):
    """paste_masks over an explicit list of mask rows (patch offsets / sizes in the flat probability buffer and their boxes, as in
    forward_seg's kg_meta): one kg_mask_paste (packed=True: kg_mask_paste_bits) launch.  Returns [masks, dets] as paste_masks does."""
    n = len(off)
    dev = flat.device
    b = np.asarray(boxes, np.float32).reshape(-1, 5)
    y1 = np.maximum(0, np.round(b[:, 0]).astype(np.int32)); x1 = np.maximum(0, np.round(b[:, 1]).astype(np.int32))
    y2 = np.minimum(np.round(b[:, 2]).astype(np.int32), input_h - 1); x2 = np.minimum(np.round(b[:, 3]).astype(np.int32), input_w - 1)
    tab = np.stack([np.asarray(off, np.int64), np.asarray(h, np.int64), np.asarray(w, np.int64), y1, x1, y2, x2,
                    np.zeros(n, np.int64)], 1).astype(np.int32)
    dets = np.stack([y1.astype(np.float64) / input_h * image_h, x1.astype(np.float64) / input_w * image_w,
                     y2.astype(np.float64) / input_h * image_h, x2.astype(np.float64) / input_w * image_w, b[:, 4].astype(np.float64)], 1).astype(np.float32)
    if packed:
        from .bitmasks import BitMasks
        bm = BitMasks.empty(int(image_h), int(image_w), dev, n)
        if n:
            with torch.cuda.device(dev):
                _lib.call("kg_mask_paste_bits", ptr(flat), ptr(ops.h2d(tab.reshape(-1), dev)), n, int(input_h), int(input_w), int(image_h),
                          int(image_w), _lib.c_float(float(seg_thresh)), ptr(bm.words), c_long(bm.words.shape[1]), stream_ptr())
        return [bm, dets]
    out = torch.empty(n, int(image_h), int(image_w), dtype=torch.uint8 if device_u8 else torch.float32, device=dev)
    if n:
        with torch.cuda.device(dev):
            _lib.call("kg_mask_paste", ptr(flat), ptr(ops.h2d(tab.reshape(-1), dev)), n, int(input_h), int(input_w), int(image_h), int(image_w),
                      _lib.c_float(float(seg_thresh)), ptr(out), 1 if device_u8 else 0, stream_ptr())
    return [out if device_u8 else out.cpu().numpy(), dets]
