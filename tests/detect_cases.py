"""Seeded inputs and case tables the CPU and GPU tests of the detection stage share (tests/test_detect_cases_cpu.py asserts from the oracle
alone that the tables contain what they claim; tests/test_gpu_detect.py compares the library with the oracle on them, bit for bit).

The stage is csrc/postproc.hip behind postprocessing.py and nms.py: Hough vote, Gaussian, peaks, ranking, greedy grouping (part A), box assembly
(part B), NMS and the gather of the kept rows (part C), and what the entry points return when a capacity is smaller than what the input produces
(part D).  Every builder is a pure function of its arguments; the oracle results are computed once per process and must not be written to."""
import functools

import numpy as np

from oracle import postproc as op
from oracle import synth

# ---- part A: map sizes ------------------------------------------------------------------------------------------------------------------------
# ragged: no multiple of the 32 x 32 Hough tile, of the 8 / 16 / 32 px grouping cell or of the 1024-element peak chunk (25 x 17 is the coarsest
# head map of a 200 x 136 image); one pixel wide or high: the Gaussian's 'reflect' border folds its 8-tap reach over and over
THIN = [(1, 1), (1, 70), (70, 1)]
RAGGED = THIN + [(25, 17), (33, 70), (31, 97), (65, 87)]
# seams of group_kernel, crossed in both orientations by thin maps: cell size 8 px up to 256, 16 px up to 512, 32 px up to 1024, beyond it the
# general (global-memory) path
SEAMS = [(24, 256), (24, 257), (257, 24), (24, 512), (24, 513), (513, 24), (24, 1024), (1024, 24), (24, 1025), (1025, 24)]
# a 24-pixel strip of 256 / 257 columns groups 70 .. 76 skeletons; 40 pixels give the 8 / 16 px seam 100 and more on either side as well
SEAMS += [(40, 256), (40, 257), (257, 40)]
# synth.head_maps arguments (H, W, objects, seed) of the ragged sizes that can hold objects, and of the general grouping path
SYNTH = [(25, 17, 2, 5), (33, 70, 5, 5), (31, 97, 6, 5), (65, 87, 10, 5), (24, 1025, 20, 5)]
BATCH_SIZES = [(33, 70), (24, 513), (24, 1025)]
GK_NL = 8192      # postproc.hip: most keypoints the LDS path of group_kernel holds


def default_seed(H, W):
    return 1000 * H + W


def random_maps(H, W, seed=None):
    """Untrained-network-like head maps (kp [1,5,H,W], short [1,10,H,W], mid [1,40,H,W], float32): peaks everywhere, offsets of many pixels."""
    rng = np.random.default_rng(default_seed(H, W) if seed is None else seed)
    kp = (rng.random((1, 5, H, W)) ** 2).astype(np.float32)
    short = (rng.normal(size=(1, 10, H, W)) * 3).astype(np.float32)
    mid = (rng.normal(size=(1, 40, H, W)) * 8).astype(np.float32)
    return kp, short, mid


def stage_maps(H, W, seed=None):
    """random_maps; a one-pixel-wide map (which has no peak) gets kp = 0.9 everywhere, so that heat and blur carry values through the reflection
    (1 x 1: offsets of 1/16 the size as well -- nearly every vote of the full-size ones leaves the only cell)"""
    kp, short, mid = random_maps(H, W, seed)
    if min(H, W) == 1:
        kp = np.full_like(kp, 0.9)
    if H == W == 1:
        short = short / 16
    return kp, short, mid


def synth_maps(H, W, n, seed):
    return synth.head_maps(H, W, n, seed, smin=6, smax=16)[:3]


def oracle_stages(kp, short, mid, thresh=0.004, peak_cap=None):
    """every stage of the oracle; peak_cap: ranking and grouping see the first peak_cap peaks in scan order only (npeaks stays the full count)"""
    heat = op.hough(kp, short)
    blur = op.gauss(heat)
    ids, xs, ys, conf = op.peaks(blur, thresh)
    total = len(ids)
    if peak_cap is not None:
        ids, xs, ys, conf = ids[:peak_cap], xs[:peak_cap], ys[:peak_cap], conf[:peak_cap]
    skel = op.group(ids, xs, ys, conf, mid)
    return dict(heat=heat, blur=blur, peaks=np.stack([ids, xs, ys], 1).reshape(-1, 3), peak_conf=conf, skel=skel, npeaks=total)


@functools.lru_cache(maxsize=None)
def stage_reference(H, W, seed=None):
    return oracle_stages(*stage_maps(H, W, seed))


@functools.lru_cache(maxsize=None)
def synth_reference(H, W, n, seed):
    return oracle_stages(*synth_maps(H, W, n, seed))


def group_route(n, H, W):
    """the path group_kernel takes for n ranked keypoints of an H x W map: 'general', or the cell-size exponent CS of group_fast"""
    if not (n <= GK_NL and H <= 1024 and W <= 1024):
        return "general"
    return 3 if (H <= 256 and W <= 256) else 4 if (H <= 512 and W <= 512) else 5


def image_scales(H, W, n, seed):
    """synth.head_maps at the four scales of an H x W image, object sizes scaled as tests/test_gpu_batch_inference.py::four_scales scales them"""
    out = []
    for sc in (1, 2, 4, 8):
        kp, short, mid, _ = synth.head_maps(H // sc, W // sc, max(1, n // sc), seed * 10 + sc, smin=max(3, 14 // sc), smax=max(6, 40 // sc))
        out.append([kp, short, mid])
    return out


@functools.lru_cache(maxsize=None)
def end_to_end():
    """three 200 x 136 images (head maps 200 x 136, 100 x 68, 50 x 34, 25 x 17), the middle one all zero -> (maps per image, op.detect per image)"""
    decs = [image_scales(200, 136, 16 + 8 * i, 300 + i) for i in range(3)]
    decs[1] = [[np.zeros_like(a) for a in d] for d in decs[1]]
    return decs, [op.detect(d, 0.5) for d in decs]


# ---- part B: skeleton tables ----------------------------------------------------------------------------------------------------------------------
BOX_BRANCHES = ["nc4", "nc3 no tl", "nc3 no tr", "nc3 no bl", "nc3 no br", "tl-br", "tr-bl", "tl tr c", "tl bl c", "tr br c", "bl br c", "nc2 rest", "nc<2"]
REJECTING = ("nc2 rest", "nc<2")


def skeleton_table(n, seed):
    """[n, 5, 3] float64 rows of (x, y, conf) for tl, tr, bl, br, centre.  Row i has the mask pattern i % 32 (keypoint j present iff bit j), so all
    32 patterns recur through every 1024-row chunk and accepted and rejected rows alternate.  Present keypoints have independent random positive
    coordinates (so min / max pick either corner); a missing one is (0, 0, 0) as the grouping writes it, in every fifth row a peak of column 0
    instead (x = 0 with a row and a confidence: still missing).  Every seventh row has five equal confidences."""
    rng = np.random.default_rng(seed)
    t = np.zeros((n, 5, 3), np.float64)
    t[:, :, 0] = rng.uniform(1., 500., (n, 5))
    t[:, :, 1] = rng.uniform(1., 500., (n, 5))
    t[:, :, 2] = rng.random((n, 5))
    t[6::7, :, 2] = 0.5
    present = ((np.arange(n)[:, None] % 32) >> np.arange(5)[None, :]) & 1 == 1
    col0 = np.zeros((n, 1), bool); col0[4::5] = True
    t[~present & ~col0] = 0.
    t[:, :, 0][~present] = 0.
    return t


def refine_keeps(row):
    m = row[:, 0] > 0.
    return bool(m.sum() >= 3 or (m[0] and m[3]) or (m[1] and m[2]))


def box_branch(row):
    """the branch of skeleton_box (postproc.hip; postprocessing.py:164-242 of the reference) a [5, 3] row takes, as a name of BOX_BRANCHES"""
    m = [bool(v) for v in row[:, 0] > 0.]
    nc = sum(m[:4])
    if nc == 4:
        return "nc4"
    if nc == 3:
        return "nc3 no " + ("tl", "tr", "bl", "br")[m[:4].index(False)]
    if nc == 2:
        if m[0] and m[3]: return "tl-br"
        if m[1] and m[2]: return "tr-bl"
        if m[0] and m[1] and m[4]: return "tl tr c"
        if m[0] and m[2] and m[4]: return "tl bl c"
        if m[1] and m[3] and m[4]: return "tr br c"
        if m[2] and m[3] and m[4]: return "bl br c"
        return "nc2 rest"
    return "nc<2"


def table_branches(table, do_refine):
    """per row: 'refined out' (do_refine and refine_skeleton drops it) or its box_branch"""
    return ["refined out" if (do_refine and not refine_keeps(r)) else box_branch(r) for r in table]


def boxes_reference(table, scale, do_refine):
    return op.boxes(op.refine(table) if do_refine else table, scale)


# ---- part C: box populations --------------------------------------------------------------------------------------------------------------------
NMS_NL = 2048     # postproc.hip: most boxes the LDS path of nms_kernel holds
NMS_SIZES = [1, 2, 300, 2047, 2048, 2049, 5000]
NMS_THRESHOLDS = [0.0, 0.1, 0.5, 1.0]


def box_population(n, seed, extent=600):
    """[n, 5] float64 (y1, x1, y2, x2, conf): centres uniform in [0, extent)^2, sides uniform in [8, 40], confidences rounded to two digits --
    101 values, so equal confidences are the rule"""
    rng = np.random.default_rng(seed)
    cy, cx = rng.uniform(0, extent, n), rng.uniform(0, extent, n)
    h, w = rng.uniform(8, 40, n), rng.uniform(8, 40, n)
    conf = np.round(rng.random(n), 2)
    return np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2, conf], 1)


def special_rows(pop, seed):
    """40 rows for splicing into pop: 20 exact duplicates of rows of pop (IoU 1: the later index loses the tie), 10 zero-area boxes of which five
    are identical (inter / union = 0 / 0, and NaN is 'not <= thresh': suppressed, as by the reference's np.where(ovr <= thresh)), 5 boxes with
    negative coordinates, 5 inverted boxes (y2 < y1: a negative area)"""
    rng = np.random.default_rng(seed)
    dup = pop[rng.choice(len(pop), 20, replace=len(pop) < 20)]
    p = rng.uniform(50, 550, (10, 2)); p[5:] = p[5]
    zero = np.concatenate([p, p, np.round(rng.random((10, 1)), 2)], 1)
    zero[5:, 4] = [0.3, 0.9, 0.9, 0.5, 0.7]
    neg = box_population(5, seed + 1, extent=60); neg[:, :4] -= 85.
    inv = box_population(5, seed + 2); inv[:, [0, 2]] = inv[:, [2, 0]]
    return np.concatenate([dup, zero, neg, inv], 0)


def spliced_population(n, seed):
    """box_population(n, seed) with special_rows inserted at seeded positions -> (boxes [n + 40, 5], positions of the 40 rows)"""
    pop = box_population(n, seed)
    sp = special_rows(pop, seed + 100)
    rng = np.random.default_rng(seed + 200)
    where = np.sort(rng.choice(n + len(sp), len(sp), replace=False))
    out = np.empty((n + len(sp), 5), np.float64)
    mask = np.zeros(len(out), bool); mask[where] = True
    out[mask] = sp; out[~mask] = pop
    return out, where


def grid_population():
    """9 x 9 identical 20 x 20 boxes 10 apart (IoU 1/3 with the four neighbours, 1/7 diagonally), confidences falling along the raster: every kept
    box suppresses its right and lower neighbours at 0.3, whose own neighbours then survive -- the kept set depends on the whole chain"""
    y, x = np.mgrid[0:9, 0:9]
    y, x = y.ravel() * 10., x.ravel() * 10.
    return np.stack([y, x, y + 20., x + 20., 1. - np.arange(81) * 0.01], 1)


def nms_pick(boxes, thresh):
    """indices the oracle keeps, in pick order"""
    b = np.ascontiguousarray(boxes, np.float64).reshape(-1, 5)
    keep = np.empty(max(len(b), 1), np.int32)
    import ctypes
    nk = op.lib().kgo_nms(ctypes.c_int(len(b)), b.ctypes.data_as(ctypes.c_void_p), ctypes.c_double(thresh), keep.ctypes.data_as(ctypes.c_void_p))
    return keep[:nk].copy()


def tied(boxes):
    """boxes whose confidence some other box shares"""
    _, inv, cnt = np.unique(boxes[:, 4], return_inverse=True, return_counts=True)
    return int((cnt[inv] > 1).sum())


@functools.lru_cache(maxsize=None)
def nms_case(name):
    """named populations of the NMS tests -> boxes [n, 5] (read only)"""
    if name == "grid":
        b = grid_population()
    elif name.endswith("+specials"):
        b = spliced_population(int(name[:-9]), 1)[0]
    else:
        b = box_population(int(name), 1)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def nms_reference(name, thresh):
    b = nms_case(name)
    return nms_pick(b, thresh)


# ---- part D: capacities ---------------------------------------------------------------------------------------------------------------------------
# (H, W, peak_cap, skel_cap) on random_maps(H, W): 65 x 87 has 373 peaks and 56 skeletons, 24 x 1025 (general grouping path) 1541 peaks
CAP_CASES = [(65, 87, 373, 373), (65, 87, 372, 372), (65, 87, 100, 100), (65, 87, 1, 1), (65, 87, 373, 10), (65, 87, 100, 5),
             (24, 1025, 500, 500), (24, 1025, 1541, 20)]
SKEL_OVERFLOW = [(65, 87, 373, 10), (65, 87, 100, 5), (24, 1025, 1541, 20)]


@functools.lru_cache(maxsize=None)
def cap_reference(H, W, peak_cap):
    return oracle_stages(*random_maps(H, W), peak_cap=peak_cap)


CAP_BATCH_PEAK_CAP = 200
CAP_BATCH_SEEDS = (71, 72, 73)


@functools.lru_cache(maxsize=None)
def cap_batch():
    """three 65 x 87 random maps for one kg_postproc_batch call with peak_cap = 200 and ONE threshold: the threshold lies between the 200th and the
    201st largest peak confidence of the middle image (exactly 200 peaks); the first image lost the kp of its lower rows (fewer), the last is
    whole (more, at that threshold: its confidences are the same distribution, and the CPU test asserts it).
    -> (maps per image, threshold, oracle_stages per image truncated to 200 peaks)"""
    H, W = 65, 87
    maps = [random_maps(H, W, s) for s in CAP_BATCH_SEEDS]
    conf = np.sort(op.peaks(op.gauss(op.hough(maps[1][0], maps[1][1])), 0.004)[3])[::-1]
    thresh = float((conf[CAP_BATCH_PEAK_CAP - 1] + conf[CAP_BATCH_PEAK_CAP]) / 2)
    maps[0][0][:, :, 40:, :] = 0.
    return maps, thresh, [oracle_stages(*m, thresh=thresh, peak_cap=CAP_BATCH_PEAK_CAP) for m in maps]
