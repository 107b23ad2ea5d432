"""Batched inference: the reference driver's per-image evaluation path (test.py:88-157, test_inference + post_processing) for a whole
batch of images in one call.

    forward_dec over the batch -> detect_batch -> ONE forward_seg with every image's boxes -> one kg_mask_paste launch per output size.

predict() is an opt-in API for a caller's own evaluation loop; the reference drivers (dropin/) are unchanged.  Resizing the source images
to the network input stays with the caller."""
import numpy as np
import torch

from . import _lib, postprocessing
from ._labelmaps import size_groups  # (its owner is the label-map batch walk; it stays importable here)


def image_row_ranges(img, nimg):
    """[start, stop) of every image's rows in a flat list of rows sorted by image index (forward_seg's kg_meta["img"])."""
    img = np.asarray(img, np.int64).reshape(-1)
    if len(img) and np.any(np.diff(img) < 0):
        raise _lib.KGLibraryError("image_row_ranges: rows are not sorted by image")
    starts = np.searchsorted(img, np.arange(nimg + 1), side="left")
    return [(int(starts[i]), int(starts[i + 1])) for i in range(nimg)]


def predict(model, x, nms_thresh=0.5, seg_thresh=0.5, image_sizes=None, device_u8=False, max_workspace_bytes=None, packed=False):
    """test_inference + post_processing (test.py:88-157) for the batch x [N,3,H,W] (already resized and normalised as test.py:91-92 does).
    The model's mode is left as it is.  image_sizes: (h, w) of every source image (default: the input size).
    Returns N entries: None (no detection) or [masks float32 [n, h, w] in {0, 1}, dets float32 [n, 5] (y1, x1, y2, x2, conf) in image pixels],
    the masks as uint8 device tensors with device_u8=True, as a bitmasks.BitMasks (device words, one bit per pixel) with packed=True."""
    with torch.no_grad():
        d0, d1, d2, d3, feat_seg = model.forward_dec(x)
    return predict_from_heads(model, [d0, d1, d2, d3], feat_seg, x.shape[2], x.shape[3], nms_thresh, seg_thresh, image_sizes, device_u8,
                              max_workspace_bytes, packed)


def predict_from_heads(model, dec, feat_seg, input_h, input_w, nms_thresh=0.5, seg_thresh=0.5, image_sizes=None, device_u8=False,
                       max_workspace_bytes=None, packed=False, dets=None):
    """The part of predict() after forward_dec: dec = ([kp, short, mid] x 4) and feat_seg of a batch, as forward_dec returns them.
    dets: what postprocessing.detect_batch(dec, nms_thresh) returned, for a caller that already ran it (evaluation.evaluate)."""
    N = dec[0][0].shape[0]
    sizes = [(int(input_h), int(input_w))] * N if image_sizes is None else [(int(h), int(w)) for h, w in image_sizes]
    if len(sizes) != N:
        raise _lib.KGLibraryError(f"predict: {len(sizes)} image sizes for {N} images")
    if dets is None:
        dets = postprocessing.detect_batch(dec, nms_thresh, max_workspace_bytes=max_workspace_bytes)
    elif len(dets) != N:
        raise _lib.KGLibraryError(f"predict: {len(dets)} detection entries for {N} images")
    if all(d is None for d in dets):
        return [None] * N
    boxes = [d if d is not None else np.zeros((0, 5), np.float64) for d in dets]   # (one array per image, as test.py:119 passes [bboxes])
    with torch.no_grad():
        pred = model.forward_seg(feat_seg, boxes)
    meta = getattr(pred, "kg_meta", None)
    out = [None] * N
    if meta is None:                     # every box fell outside the feature maps: no mask rows at all
        for i in range(N):
            if dets[i] is not None:
                out[i] = _empty(sizes[i], device_u8, feat_seg[0].device, packed)
        return out
    rng = image_row_ranges(meta["img"], N)
    off, hh, ww, bx = np.asarray(meta["off"]), np.asarray(meta["h"]), np.asarray(meta["w"]), np.asarray(meta["boxes"])
    for (h, w), imgs in size_groups(sizes):
        imgs = [i for i in imgs if dets[i] is not None]
        if not imgs:
            continue
        sel = np.concatenate([np.arange(*rng[i]) for i in imgs]).astype(np.int64)
        masks, d = postprocessing.paste_rows(meta["flat"], off[sel], hh[sel], ww[sel], bx[sel], input_h, input_w, w, h, seg_thresh, device_u8,
                                              packed)
        r = 0
        for i in imgs:
            k = rng[i][1] - rng[i][0]
            out[i] = [masks[r:r + k], d[r:r + k]]
            r += k
    return out


def _empty(hw, device_u8, dev, packed=False):
    h, w = hw
    if packed:
        from .bitmasks import BitMasks
        return [BitMasks.empty(h, w, dev), np.zeros((0, 5), np.float32)]
    m = torch.empty(0, h, w, dtype=torch.uint8, device=dev) if device_u8 else np.zeros((0, h, w), np.float32)
    return [m, np.zeros((0, 5), np.float32)]


def instances_from_predictions(preds):
    """predict(packed=True)'s list -> per image None or an instances.Instances (labels: device int32 [h, w], dets: predict's, table: host
    int64 [n, 8], masks: the BitMasks).  One kg_instance_labels call per distinct output size, with all images of that size in it, and one
    device -> host copy of all tables."""
    from . import instances
    out = [None] * len(preds)
    todo = [i for i, p in enumerate(preds) if p is not None]
    if not todo:
        return out
    tables, where = [], []
    for _, imgs in size_groups([preds[i][0].shape[1:] for i in todo]):
        imgs = [todo[j] for j in imgs]
        parts = [preds[i][0] for i in imgs]
        if parts[0].device.type != "cuda":
            raise _lib.KGLibraryError("predict_instances (MI355X build) needs masks on a GPU device")
        row_start = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
        labels, table = instances.label_map(instances.join_masks(parts), row_start)
        tables.append(table)
        for k, i in enumerate(imgs):
            out[i] = instances.Instances(labels[k], preds[i][1], None, preds[i][0])
            where.append(i)
    host = torch.cat(tables).cpu().numpy() if len(tables) > 1 else tables[0].cpu().numpy()
    r = 0
    for i in where:
        out[i].table = host[r:r + len(out[i].masks)]
        r += len(out[i].masks)
    return out


def predict_instances(model, x, nms_thresh=0.5, seg_thresh=0.5, image_sizes=None, max_workspace_bytes=None, clean=None, measure=None,
                      expand=None, neighbours=None, runs=None, contours=None, hulls=None, quantiles=None, split=None, texture=None, thin=None, crops=None):
    """predict(packed=True) followed by the instance label map and the per-instance table of every image (instances.py), on the device:
    the label map (4 bytes per pixel) and the table (64 bytes per instance) replace n full-size masks as what crosses to the host.
    clean: None, or a dict of components.clean's policy arguments: every label map is then cleaned on the device (one components pass
    over all images of one output size) and the tables are refreshed.
    expand: None, or a distance in pixels (a number, at most 64): every instance is then grown by that much without two instances
    merging (distance.expand_instances_batch), after the clean-up and before the measurements, which then measure the expanded regions.
    measure: None; True: every result's `measurements` holds the geometry of its instances (measure.py), measured on the final label
    map; or a uint8 / uint16 [N, h, w, C] array or device tensor at the label maps' size: the intensity columns too.  One launch for
    all images of one output size.
    neighbours: None; True, or a dict of neighbours.neighbours_instances' keyword arguments (connectivity, expand, slots,
    max_job_pixels): every result's `neighbours` holds the touching-neighbour graph of its final label map (neighbours.py), one launch
    for all images of one output size.  None adds no launch and no import.
    runs: None; True, or a dict of runlengths.runs_instances' keyword arguments (max_job_pixels): every result's `runs` holds the
    run-length lists of its instances (runlengths.py: Kaggle rows, COCO counts), taken last, on the final label map -- two launches and
    two copies back for all images of one output size.  None adds no launch and no import.
    contours: None; True, or a dict (contours.contours_instances takes no keyword arguments yet, so an empty one): every result's
    `contours` holds the polygon rings of its instances (contours.py: COCO polygons, GeoJSON), taken last, next to runs, on the final
    label map -- two launches and two copies back for all images of one output size.  None adds no launch and no import.
    hulls: None; True, or a dict of hulls.hulls_instances' keyword arguments (max_job_pixels): every result's `hulls` holds the convex
    hull of its instances (hulls.py: solidity, Feret diameters, hull rings), taken last, next to contours, on the final label map -- one
    launch and one copy back for all images of one output size.  None adds no launch and no import.
    quantiles: None; a uint8 / uint16 [N, h, w, C] array or device tensor at the label maps' size, or a dict {"image": that, "q": ...,
    "max_job_pixels": ...} of intensity.quantiles_instances_batch's arguments: every result's `quantiles` holds the intensity order
    statistics of its instances (intensity.py: median, quartiles, a 5 % / 95 % range), taken next to measure on the final label map -- one
    launch, one upload and one copy back for all images of one output size.  None adds no launch and no import.
    texture: None; a uint8 / uint16 [N, h, w, C] array or device tensor at the label maps' size, or a dict {"image": that, "levels": ...,
    "distance": ..., "channels": ..., "range": ..., "max_job_pixels": ...} of texture.texture_instances_batch's arguments: every result's
    `texture` holds the co-occurrence matrices of its instances (texture.py: Haralick's features), taken next to quantiles on the final
    label map -- one launch, one upload and one copy back for all images of one output size (range="object" measures first unless
    measure= already gave the intensity columns).  None adds no launch and no import.
    split: None; a distance in pixels (a number, 1 .. 64), or a dict of split.split_instances_batch's arguments (distance, connectivity,
    min_seed_area, frame, only): merged instances are then split into their core seeds' regions (split.py), after the clean-up and
    before the expansion and everything else; every result has `parent` set, dets extended by a copy of the parent's row per new id and
    masks unchanged.  One seeds pass and one kg_label_split launch for all images of one output size.  None adds no launch and no
    import.
    thin: None; True, or a dict of thinning.thin_instances_batch's keyword arguments (max_passes): every result's `midlines` holds the
    midline of its instances (thinning.py: length, tips, branch points, and the midline map `skel`), taken next to the other
    measurements on the final label map -- one upload, one launch and one copy back for all images of one output size.  None adds no
    launch and no import.
    crops: None; a uint8 / uint16 [N, h, w, C] array or device tensor at the label maps' size, or a dict {"image": that (None: masks only),
    "size": ..., "window": ..., "margin": ..., "angle": ..., "side": ..., "flip": ..., "mode": ..., "masked": ..., "fill": ..., "masks": ...}
    of crops.crops_instances_batch's arguments: every result's `crops` holds one fixed-size patch and mask per instance, on the device
    (crops.py: what a second network takes), taken last, next to hulls, on the final label map -- one upload (the table) and one launch
    for all images of one output size, nothing copied back.  None adds no launch and no import."""
    if not torch.is_tensor(x) or x.device.type != "cuda":
        raise _lib.KGLibraryError("predict_instances (MI355X build) needs the input batch on a GPU device")
    out = instances_from_predictions(predict(model, x, nms_thresh, seg_thresh, image_sizes, max_workspace_bytes=max_workspace_bytes, packed=True))
    if clean is not None:
        from . import components
        out = components.clean_instances_batch(out, **dict(clean))
    if split is not None:
        from . import split as _split
        out = _split.split_instances_batch(out, **(dict(split) if isinstance(split, dict) else {"distance": split}))
    if expand is not None:
        from . import distance
        out = distance.expand_instances_batch(out, expand)
    if measure is not None and measure is not False:
        from . import measure as _measure
        _measure.measure_instances_batch(out, None if measure is True else measure)
    if quantiles is not None and quantiles is not False:
        from . import intensity
        kw = dict(quantiles) if isinstance(quantiles, dict) else {"image": quantiles}
        intensity.quantiles_instances_batch(out, kw.pop("image", None), **kw)
    if texture is not None and texture is not False:
        from . import texture as _texture
        kw = dict(texture) if isinstance(texture, dict) else {"image": texture}
        _texture.texture_instances_batch(out, kw.pop("image", None), **kw)
    if thin is not None and thin is not False:
        from . import thinning
        thinning.thin_instances_batch(out, **({} if thin is True else dict(thin)))
    if neighbours is not None and neighbours is not False:
        from . import neighbours as _neighbours
        _neighbours.neighbours_instances_batch(out, **({} if neighbours is True else dict(neighbours)))
    if runs is not None and runs is not False:
        from . import runlengths
        runlengths.runs_instances_batch(out, **({} if runs is True else dict(runs)))
    if contours is not None and contours is not False:
        from . import contours as _contours
        _contours.contours_instances_batch(out, **({} if contours is True else dict(contours)))
    if hulls is not None and hulls is not False:
        from . import hulls as _hulls
        _hulls.hulls_instances_batch(out, **({} if hulls is True else dict(hulls)))
    if crops is not None and crops is not False:
        from . import crops as _crops
        kw = dict(crops) if isinstance(crops, dict) else {"image": crops}
        _crops.crops_instances_batch(out, kw.pop("image", None), **kw)
    return out


from .tiling import predict_tiled  # noqa: E402,F401  (whole images of any size at native resolution: tiling.py)
