"""Per-instance measurements: shape, contact and intensity of every instance of a label map, without copying the map back.

predict_instances and predict_tiled end in ONE int32 label map per image; components.py cleans it and labelmetrics.py scores it.  This
module measures the objects.  Every such measurement -- centroid, second moments, axes, orientation, boundary length, "touches the
frame", "touches a neighbour", mean and spread of the intensity -- is a function of a few exact integers per instance; the device counts
them (kg_label_measure, csrc/measure.hip), a few thousand integers come back, and the host derives the floats in float64.

    measure_host       the semantics in NumPy (the CPU route, and the yardstick of the GPU tests)
    measure            the same rows from device tensors, ONE launch
    measure_instances  measure for an Instances / TiledInstances (ids 1 .. n, boxes from its table)
    Measurements       raw int64 [n, 10 + 4 C]; props() = the derived float64 quantities, shared by both routes

Semantics (include/kgnet_hip.h is the normative text)
  job         {img, id, y1, x1, y2, x2}: a half-open box, clamped to the map.  P = the pixels of the box in image img with labels == id.
  row         int64 [10 + 4 C] (columns(C)), C = the number of image channels, 0 without an image:
                area                                   |P|
                sum_y, sum_x, sum_yy, sum_yx, sum_xx   over P, of the pixel coordinates in the image
                edges                                  the (pixel of P, direction up / down / left / right) pairs whose neighbour lies
                                                       outside the map or holds a value != id
                edges_border                           those whose neighbour lies outside the map
                edges_contact                          those whose neighbour lies inside the map and holds a non-zero value != id
                boundary_pixels                        the pixels of P with at least one such edge
                sum_c, sumsq_c, min_c, max_c           per channel over P; min and max are 0 when area == 0
  neighbours  are read from the MAP, never from the box: a box edge or band edge inside the map is not an object edge.
  values      are compared only: INT_MIN, -1 and INT_MAX in the map are "another non-zero value".
  bad jobs    an image index outside [0, nimg), an empty or inverted box, an id the box does not hold: a row of zeros.
  sizes       H, W <= 32768, so area <= 2^30, a coordinate product < 2^30, a coordinate sum < 2^60 and a uint16 sum of squares < 2^62:
              every column fits int64 and nothing else needs checking; larger maps are refused.
  images      uint8 or uint16 [nimg, H, W, C] ([H, W, C] for one map), 1 <= C <= 4.
  bands       a job whose clamped box holds more than max_job_pixels pixels is split as labelmetrics.split_jobs does; the band rows are
              combined on the host (combine_bands): everything is added, min / max are taken over the bands with area > 0."""
import math

import numpy as np

from . import _lib, _labelmaps, labelmetrics
from ._labelmaps import JOB_COLUMNS, MAX_CHANNELS, MAX_SIDE, SUMS_FIT, is_device, jobs_from_stats  # noqa: F401  (MAX_SIDE, jobs_from_stats: public here)
from .labelmetrics import split_jobs  # noqa: F401  (the band rule is labelmetrics': columns 0 and 1 of a job pass through it untouched)

KGLibraryError = _lib.KGLibraryError
GEOMETRY_COLUMNS = ("area", "sum_y", "sum_x", "sum_yy", "sum_yx", "sum_xx", "edges", "edges_border", "edges_contact", "boundary_pixels")
CHANNEL_COLUMNS = ("sum", "sumsq", "min", "max")


def columns(C):
    """The column names of a row with C image channels: GEOMETRY_COLUMNS, then sum_c, sumsq_c, min_c, max_c for c = 0 .. C - 1."""
    C = int(C)
    if not 0 <= C <= MAX_CHANNELS:
        raise KGLibraryError(f"columns: {C} channels (0 .. {MAX_CHANNELS})")
    return GEOMETRY_COLUMNS + tuple(f"{k}_{c}" for c in range(C) for k in CHANNEL_COLUMNS)


# ---- the derived quantities -----------------------------------------------------------------------------------------------------------

def _exact(num):
    """an object array of Python integers -> float64, every element rounded once"""
    return np.array([float(v) for v in num], np.float64)


class Measurements:
    """raw = host int64 [n, 10 + 4 C] (columns(C)), one row per instance (or per job); props() derives the float64 quantities."""
    __slots__ = ("raw",)

    def __init__(self, raw):
        r = np.ascontiguousarray(raw, np.int64)
        if r.ndim != 2 or r.shape[1] < len(GEOMETRY_COLUMNS) or (r.shape[1] - len(GEOMETRY_COLUMNS)) % 4 \
                or (r.shape[1] - len(GEOMETRY_COLUMNS)) // 4 > MAX_CHANNELS:
            raise KGLibraryError(f"Measurements: raw must be integers [n, 10 + 4 C] with 0 <= C <= {MAX_CHANNELS}, not {r.shape}")
        self.raw = r

    def __len__(self):
        return len(self.raw)

    @property
    def channels(self):
        return (self.raw.shape[1] - len(GEOMETRY_COLUMNS)) // 4

    @property
    def columns(self):
        return columns(self.channels)

    def column(self, name):
        return self.raw[:, self.columns.index(name)]

    def props(self):
        """dict of float64 arrays [n] ([n, 2] for centroid, [n, C] for mean / std, bool for touches_border), from the integers only:

          area
          centroid             (sum_y, sum_x) / area
          mu_yy, mu_yx, mu_xx  the central second moments per pixel: (area * sum_yy - sum_y^2) / area^2 and so on.  The numerators are
                               formed in Python integers -- they exceed 64 bits, and the float64 difference cancels for an object far
                               from the origin -- and then divided once, in float64, by area^2.
          axis_major, axis_minor   4 sqrt(l1), 4 sqrt(max(l2, 0)) with l1 >= l2 the eigenvalues of [[mu_yy, mu_yx], [mu_yx, mu_xx]]: the
                               axes of the ellipse with the same second moments.
          eccentricity         sqrt(1 - max(l2, 0) / l1), 0 when l1 == 0
          orientation          0.5 atan2(2 mu_yx, mu_yy - mu_xx): the angle of the major axis measured FROM the y (row) axis TOWARDS the
                               x (column) axis, in (-pi/2, pi/2]; 0 for an object elongated along y, pi/2 along x, pi/4 along y == x.
          equivalent_diameter  sqrt(4 area / pi)
          perimeter            edges: the crack length, the number of pixel sides between the object and anything else.  It
                               overestimates the length of a smooth outline by up to 4 / pi (a circle of radius r has about 8 r cracks).
          touches_border       edges_border > 0
          contact_fraction     edges_contact / edges
          mean, std            per channel, the population standard deviation; the variance numerator area * sumsq - sum^2 is formed
                               in Python integers as above.
        An instance with area == 0 gets NaN wherever a division by zero would occur."""
        r = self.raw
        n, C = len(r), self.channels
        o = r.astype(object)                                           # Python integers: the products below exceed 64 bits
        area = o[:, 0]
        af = r[:, 0].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            a2 = _exact(area * area)
            mu_yy = _exact(area * o[:, 3] - o[:, 1] * o[:, 1]) / a2
            mu_yx = _exact(area * o[:, 4] - o[:, 1] * o[:, 2]) / a2
            mu_xx = _exact(area * o[:, 5] - o[:, 2] * o[:, 2]) / a2
            half, root = (mu_yy + mu_xx) / 2, np.sqrt(((mu_yy - mu_xx) / 2) ** 2 + mu_yx ** 2)
            l1, l2 = half + root, np.maximum(half - root, 0)            # (NaN stays NaN through np.maximum)
            ecc = np.where(l1 == 0, 0.0, np.sqrt(np.maximum(1 - l2 / np.where(l1 == 0, 1.0, l1), 0)))
            out = {"area": af,
                   "centroid": r[:, 1:3].astype(np.float64) / af[:, None],
                   "mu_yy": mu_yy, "mu_yx": mu_yx, "mu_xx": mu_xx,
                   "axis_major": 4 * np.sqrt(l1), "axis_minor": 4 * np.sqrt(l2),
                   "eccentricity": ecc,
                   "orientation": 0.5 * np.arctan2(2 * mu_yx, mu_yy - mu_xx),
                   "equivalent_diameter": np.where(af > 0, np.sqrt(4 * af / math.pi), np.nan),
                   "perimeter": r[:, 6].astype(np.float64),
                   "touches_border": r[:, 7] > 0,
                   "contact_fraction": r[:, 8].astype(np.float64) / r[:, 6].astype(np.float64)}
            mean, std = np.zeros((n, C), np.float64), np.zeros((n, C), np.float64)
            for c in range(C):
                s, q = o[:, 10 + 4 * c], o[:, 11 + 4 * c]
                mean[:, c] = r[:, 10 + 4 * c].astype(np.float64) / af
                std[:, c] = np.sqrt(_exact(area * q - s * s) / a2)
            out["mean"], out["std"] = mean, std
        return out


# ---- host statement of the semantics ----------------------------------------------------------------------------------------------------

def measure_host(labels, jobs_or_n, image=None):
    """labels: integers [H, W] or [nimg, H, W]; jobs_or_n: jobs [m, 6] = (img, id, y1, x1, y2, x2), or the instance count n (one per map
    for a stack): the ids 1 .. n are then measured inside their own boxes (labelmetrics.label_stats_host, which raises when a pixel lies
    outside [0, n]); image: None, or uint8 / uint16 [H, W, C] / [nimg, H, W, C] -> int64 [m, 10 + 4 C], one row per job, nothing split."""
    maps = _labelmaps.host_stack("measure_host", labels, SUMS_FIT)
    nimg, H, W = maps.shape
    img = _labelmaps.host_image("measure_host", image, maps.shape)
    C = 0 if img is None else img.shape[3]
    jobs = _labelmaps.host_job_table("measure_host", maps, jobs_or_n, labelmetrics.label_stats_host)
    out = np.zeros((len(jobs), 10 + 4 * C), np.int64)
    for k, (i, v, y1, x1, y2, x2) in enumerate(jobs.tolist()):
        y1, x1, y2, x2 = max(y1, 0), max(x1, 0), min(y2, H), min(x2, W)
        if not 0 <= i < nimg or y2 <= y1 or x2 <= x1:
            continue
        lab = maps[i]
        ys, xs = np.nonzero(lab[y1:y2, x1:x2] == v)
        if len(ys) == 0:
            continue
        ys, xs = ys.astype(np.int64) + y1, xs.astype(np.int64) + x1
        edge = np.zeros(len(ys), np.int64)
        border = contact = 0
        for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            ny, nx = ys + dy, xs + dx
            inside = (ny >= 0) & (ny < H) & (nx >= 0) & (nx < W)
            nb = lab[np.clip(ny, 0, H - 1), np.clip(nx, 0, W - 1)]
            differs = inside & (nb != v)
            edge += ~inside | differs
            border += int(np.count_nonzero(~inside))
            contact += int(np.count_nonzero(differs & (nb != 0)))
        out[k, :10] = (len(ys), ys.sum(), xs.sum(), (ys * ys).sum(), (ys * xs).sum(), (xs * xs).sum(), edge.sum(), border, contact,
                       np.count_nonzero(edge))
        if C:
            px = img[i, ys, xs].astype(np.int64)                       # [|P|, C]
            out[k, 10::4], out[k, 11::4], out[k, 12::4], out[k, 13::4] = px.sum(0), (px * px).sum(0), px.min(0), px.max(0)
    return out


def combine_bands(rows, owner, n_jobs):
    """rows int64 [m2, 10 + 4 C] of the pieces split_jobs made, owner int [m2] -> int64 [n_jobs, 10 + 4 C]: everything is added, min / max
    are taken over the pieces with area > 0 (0 if there is none)."""
    rows = np.asarray(rows, np.int64)
    owner = np.asarray(owner, np.int64).reshape(-1)
    if rows.ndim != 2 or len(rows) != len(owner) or (len(owner) and (owner.min() < 0 or owner.max() >= n_jobs)):
        raise KGLibraryError(f"combine_bands: rows {rows.shape}, {len(owner)} owners, {n_jobs} jobs")
    ncol = rows.shape[1]
    out = np.zeros((int(n_jobs), ncol), np.int64)
    is_min = np.zeros(ncol, bool); is_min[12::4] = True
    is_max = np.zeros(ncol, bool); is_max[13::4] = True
    add = ~(is_min | is_max)
    np.add.at(out, (owner[:, None], np.flatnonzero(add)[None]), rows[:, add])
    live = rows[:, 0] > 0
    if is_min.any() and live.any():
        lo = np.full((int(n_jobs), int(is_min.sum())), np.iinfo(np.int64).max)
        np.minimum.at(lo, owner[live], rows[live][:, is_min])
        np.maximum.at(out, (owner[live][:, None], np.flatnonzero(is_max)[None]), rows[live][:, is_max])
        out[:, is_min] = np.where(out[:, :1] > 0, lo, 0)
    return out


# ---- device -----------------------------------------------------------------------------------------------------------------------------

def measure_rows(labels, jobs, image=None):
    """kg_label_measure as it is: labels device int32 [H, W] or [nimg, H, W]; jobs host int [m, 6] (uploaded once) or a device int32
    tensor; image None, a host array (uploaded once) or a device tensor -> device int64 [m, 10 + 4 C].  One launch, no copy back, no
    synchronisation, nothing split."""
    import torch
    from ._lib import ptr, stream_ptr
    lab = _labelmaps.device_stack("measure", labels, SUMS_FIT)[0]
    dev = lab.device
    nimg, H, W = lab.shape
    img = _labelmaps.device_image("measure", image, lab.shape, dev)
    C = 0 if img is None else img.shape[3]
    jd = _labelmaps.device_jobs("measure", jobs, 6, JOB_COLUMNS, dev)
    m = jd.shape[0]
    out = torch.empty(m, 10 + 4 * C, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.call("kg_label_measure", ptr(lab), nimg, H, W, ptr(img), C, img.element_size() if C else 1, ptr(jd) if m else None, m,
                  ptr(out) if m else None, stream_ptr())
    return out


def measure(labels, n=None, jobs=None, image=None, stats=None, max_job_pixels=65536):
    """measure_host on the device -> Measurements (host).  labels: device int32 [H, W] or [nimg, H, W].  What is measured:
      jobs   host integers [m, 6] = (img, id, y1, x1, y2, x2): one row per job; or
      n      the instance count (one per map for a stack): the ids 1 .. n inside their own boxes.  The boxes come from stats -- host
             integers [n, 5] = (area, y1, x1, y2, x2), one array per map for a stack; columns 1:6 of an Instances table are that -- or,
             without stats, from labelmetrics.label_stats (its launches and one copy per map; it raises when a pixel lies outside [0, n]):
             ground-truth maps and cleaned maps are served this way.
    image: None, a host uint8 / uint16 array [H, W, C] / [nimg, H, W, C] (uploaded once) or a device tensor.
    A job whose box holds more than max_job_pixels pixels is measured in bands (split_jobs, combine_bands).
    ONE kg_label_measure launch, one upload (the jobs) and one device -> host copy (the rows)."""
    lab = _labelmaps.device_stack("measure", labels, SUMS_FIT)[0]
    j = _labelmaps.job_table("measure", lab, n, jobs, stats, labelmetrics.label_stats)
    pieces, owner = split_jobs(j, max_job_pixels)
    rows = measure_rows(lab, pieces, image).cpu().numpy()
    return Measurements(combine_bands(rows, owner, len(j)))


def measure_instances(inst, image=None, max_job_pixels=65536):
    """measure for an Instances / TiledInstances -> Measurements with len(inst) rows: ids 1 .. n, boxes from table[:, 2:6]; an instance
    with area_visible == 0 gets a row of zeros.  image: None, or uint8 / uint16 [H, W, C] at the label map's size (host array or device
    tensor).  A host label map (assemble_host's result) goes through measure_host."""
    import torch
    stats = _labelmaps.instance_stats("measure_instances", inst)
    if is_device(inst.labels):
        return measure(inst.labels, len(inst), image=image, stats=stats, max_job_pixels=max_job_pixels)
    if torch.is_tensor(image):
        image = image.cpu().numpy()
    return Measurements(measure_host(_labelmaps.host_labels(inst), jobs_from_stats(stats), image))


def measure_instances_batch(insts, images=None, max_job_pixels=65536):
    """measure_instances for predict_instances' list (entries may be None), in place: every entry's `measurements` is set.  ONE launch for
    all images of one output size.  images: None (geometry only), or uint8 / uint16 [N, h, w, C] (host array or device tensor) with one
    image per entry, at the label maps' size."""
    if images is not None and len(images) != len(insts):
        raise KGLibraryError(f"measure: {len(images)} images for {len(insts)} entries")
    for idx, stack, _, _ in _labelmaps.size_batches("measure_instances_batch", insts):
        img = None
        if images is not None:
            img = images[idx] if len(idx) != len(insts) else images
        got = measure(stack, [len(insts[i]) for i in idx], image=img, stats=[np.asarray(insts[i].table, np.int64)[:, 1:6] for i in idx],
                      max_job_pixels=max_job_pixels)
        for i, a, b in _labelmaps.deal(insts, idx):
            insts[i].measurements = Measurements(got.raw[a:b])
    return insts
