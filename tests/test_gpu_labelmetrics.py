"""GPU: label-map evaluation (csrc/labelmetrics.hip, labelmetrics.py) against the host statements of the same semantics
(labelmetrics.*_host), and LabelEvaluator on a predict_tiled result end to end.  Every comparison is exact equality of integers (and of the
float64 metrics computed from them by the same host code).  Shapes are the smallest at which the kernels can go wrong: one pixel, one
short row, a row of exactly one wave segment, widths that are no multiple of 64 (runs cross segments and row ends), more than one block,
boxes wider than a workgroup."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from kg_instance_segmentation_amd import KGnet, bitmasks, instances, tiling  # noqa: E402
from kg_instance_segmentation_amd import labelmetrics as lm  # noqa: E402
from kg_instance_segmentation_amd.bitmasks import BitMasks  # noqa: E402

DEV = "cuda"
SHAPES = [(1, 1), (1, 67), (5, 64), (37, 130), (64, 256)]


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def seeded_map(H, W, n, seed):
    """Seeded blocky map with ids 1 .. n: rectangles painted over each other, id n - 1 without a pixel (n >= 3), the id n itself, single
    pixels in the four corners, one run over a whole row (longer than 64 pixels where the map is wide enough)."""
    rng = np.random.default_rng(1000 * H + 10 * W + 7 * n + seed)
    lab = np.zeros((H, W), np.int32)
    for i in range(1, n + 1):
        y, x = rng.integers(0, H), rng.integers(0, W)
        lab[y:y + rng.integers(1, H // 3 + 2), x:x + rng.integers(1, W // 2 + 2)] = i
    if n >= 1:
        lab[H // 2, :] = 1
        lab[0, 0], lab[0, W - 1], lab[H - 1, 0], lab[H - 1, W - 1] = 1, n, 1, n
    if n >= 3:
        lab[lab == n - 1] = 0
    lab.setflags(write=False)
    return lab


# ---- stats ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 3, 200])
@pytest.mark.parametrize("H,W", SHAPES)
def test_label_stats(H, W, n):
    maps = [seeded_map(H, W, n, 0), np.zeros((H, W), np.int32)]
    if n:
        maps += [np.full((H, W), n, np.int32), np.full((H, W), 1, np.int32)]                  # one id fills the whole map
    for k, lab in enumerate(maps):
        want = lm.label_stats_host(lab, n)
        got = lm.label_stats(up(lab), n)
        assert got.dtype == np.int64 and got.shape == (n, 5) and np.array_equal(got, want), (k, got[:4], want[:4])
    if n:
        assert lm.label_stats(up(maps[2]), n)[n - 1].tolist() == [H * W, 0, 0, H, W]
    if n >= 3:
        want = lm.label_stats_host(maps[0], n)
        assert not want[n - 2].any() and want[n - 1, 0] > 0                                   # an id with no pixel, and the id n itself
    stats, invalid = lm.label_stats_device(up(maps[0]), n)
    assert stats.is_cuda and stats.dtype == torch.int32 and tuple(stats.shape) == (n, 5) and tuple(invalid.shape) == (1,) and int(invalid) == 0


@pytest.mark.parametrize("n", [0, 3, 200])
def test_label_stats_invalid_values(n):
    H, W = 37, 130
    lab = seeded_map(H, W, n, 1).copy()
    where = [(0, 0), (0, 63), (0, 64), (5, 129), (36, 129), (20, 1), (20, 2), (20, 3)]
    vals = [n + 1, -3, n + 1, -3, -2 ** 31, 2 ** 31 - 1, -1, n + 1]
    for (y, x), v in zip(where, vals):
        lab[y, x] = v
    want, count = lm.label_stats_counts_host(lab, n)
    assert count == len(where)
    stats, invalid = lm.label_stats_device(up(lab), n)                                        # the raw entry: the count, and exact valid ids
    assert int(invalid) == count and np.array_equal(stats.cpu().numpy(), want)
    with pytest.raises(lm.KGLibraryError, match=f"{count} pixel"):
        lm.label_stats(up(lab), n)
    with pytest.raises(lm.KGLibraryError):
        lm.contingency(up(lab), up(seeded_map(H, W, n, 2)), n, n)
    if n:
        assert want[:, 0].sum() > 0


# ---- intersections ------------------------------------------------------------------------------------------------------------------------

def test_inter_jobs():
    H, W, n = 37, 130, 40
    a, b = seeded_map(H, W, n, 3), seeded_map(H, W, n, 4)
    ad, bd = up(a), up(b)
    none = lm.inter_jobs(ad, bd, np.zeros((0, 6), np.int32))                                  # m = 0
    assert none.is_cuda and none.dtype == torch.int64 and tuple(none.shape) == (0,)
    ia, ib = int(a[H // 2, 5]), int(b[H // 2, 5])
    special = [[ia, ib, 4, 9, 4, 40], [ia, ib, 4, 9, 30, 9],                                  # empty boxes
               [ia, ib, 30, 100, 4, 9], [ia, ib, 10, 9, 4, 40],                               # inverted boxes
               [ia, ib, -5, -7, H + 3, W + 9], [ia, ib, -2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1],      # reaching outside on every side
               [ia, ib, H, W, H + 5, W + 5], [ia, ib, -9, -9, 0, 0],                          # wholly outside
               [1000, ib, 0, 0, H, W], [ia, n - 1, 0, 0, H, W], [-1, -1, 0, 0, H, W], [0, 0, 0, 0, H, W],        # ids absent from a map; background
               [ia, ib, 0, 0, H, W]]                                                          # the whole map
    want = lm.inter_jobs_host(a, b, special)
    got = lm.inter_jobs(ad, bd, np.array(special)).cpu().numpy()
    assert np.array_equal(got, want), (got, want)
    assert not want[:4].any() and want[4] == want[5] == want[-1] > 0 and not want[6:11].any()
    rng = np.random.default_rng(5)
    m = 300
    y1, x1 = rng.integers(-3, H, m), rng.integers(-3, W, m)
    jobs = np.stack([rng.integers(0, n + 1, m), rng.integers(0, n + 1, m), y1, x1, y1 + rng.integers(0, H, m), x1 + rng.integers(0, W, m)], 1)
    jobs[:40, :2] = np.stack([a[jobs[:40, 2].clip(0, H - 1), jobs[:40, 3].clip(0, W - 1)], b[jobs[:40, 2].clip(0, H - 1), jobs[:40, 3].clip(0, W - 1)]], 1)
    want = lm.inter_jobs_host(a, b, jobs)
    assert np.array_equal(lm.inter_jobs(ad, bd, jobs).cpu().numpy(), want) and (want > 0).sum() > 30
    assert np.array_equal(lm.inter_jobs(ad, bd, up(jobs.astype(np.int32))).cpu().numpy(), want)      # device jobs
    # a box wider than the workgroup: every thread keeps its column offset from row to row
    wide_a, wide_b = seeded_map(3, 700, 5, 6), seeded_map(3, 700, 5, 7)
    jobs = [[1, 1, 0, 0, 3, 700], [1, 1, 1, 100, 3, 611], [5, 1, 0, 0, 3, 700]]
    want = lm.inter_jobs_host(wide_a, wide_b, jobs)
    assert np.array_equal(lm.inter_jobs(up(wide_a), up(wide_b), np.array(jobs)).cpu().numpy(), want) and want[0] >= 700


def test_inter_jobs_box_widths_around_the_walk():
    H, W = 40, 300
    a, b = np.full((H, W), 1, np.int32), np.full((H, W), 2, np.int32)
    jobs = np.array([[1, 2, 3, 7, 40, 7 + w] for w in (1, 2, 255, 256, 257)] + [[1, 2, H - 1, 0, H, W], [1, 2, 0, W - 1, H, W]], np.int32)
    want = lm.inter_jobs_host(a, b, jobs)
    assert want.tolist() == [37, 74, 37 * 255, 37 * 256, 37 * 257, W, H]
    assert np.array_equal(lm.inter_jobs(up(a), up(b), jobs).cpu().numpy(), want)


def test_inter_jobs_grid_stride():
    """More jobs than the grid cap of 2^20 blocks: the blocks stride, and every copy of one small job gives the single job's count."""
    from kg_instance_segmentation_amd import _lib
    from kg_instance_segmentation_amd._lib import ptr, stream_ptr
    H, W, m = 9, 70, 2 ** 20 + 3
    a, b = np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)
    a[3:5, 10:13], b[3:5, 11:14] = 4, 3
    job = np.array([[4, 3, 3, 10, 5, 14]], np.int32)                                          # 8 pixels, 4 of them counted
    want = lm.inter_jobs_host(a, b, job)
    assert want.tolist() == [4]
    ad, bd = up(a), up(b)
    assert np.array_equal(lm.inter_jobs(ad, bd, job).cpu().numpy(), want)
    guard = torch.full((m + 2,), -7, dtype=torch.int64, device=DEV)                           # a cell in front of and behind the output
    jd = up(job).repeat(m, 1)
    _lib.call("kg_label_inter_jobs", ptr(ad), ptr(bd), H, W, ptr(jd), m, ptr(guard[1:]), stream_ptr())
    assert bool((guard[1:-1] == int(want[0])).all()) and int(guard[0]) == -7 and int(guard[-1]) == -7


# ---- contingency ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", SHAPES)
def test_contingency(H, W):
    pairs_seen = 0
    for n_pred in (0, 1, 40):
        for n_gt in (0, 1, 40):
            p, g = seeded_map(H, W, n_pred, 8), seeded_map(H, W, n_gt, 9)
            want = lm.contingency_host(p, g, n_pred, n_gt)
            pd, gd = up(p), up(g)
            sp, sg = lm.label_stats_host(p, n_pred), lm.label_stats_host(g, n_gt)
            for cap in (7, 65536):
                for given in (False, True):
                    got = lm.contingency(pd, gd, n_pred, n_gt, pred_stats=sp if given else None, gt_stats=sg if given else None, max_job_pixels=cap)
                    assert got == want, (n_pred, n_gt, cap, given)
            pairs_seen += len(want.pairs)
            if H * W > 7 and n_pred and n_gt:                                                 # the split path did run
                assert len(lm.split_jobs(lm.candidate_pairs(sp, sg), 7)[0]) > len(lm.candidate_pairs(sp, sg))
    assert pairs_seen > (20 if H * W > 100 else 0)


@functools.lru_cache(maxsize=None)
def overlapping_masks(H, W, n, seed):
    rng = np.random.default_rng(seed)
    m = np.zeros((n, H, W), np.uint8)
    for k in range(n):
        y, x = rng.integers(0, H), rng.integers(0, W)
        m[k, y:y + rng.integers(1, H // 2 + 2), x:x + rng.integers(1, W // 3 + 2)] = 1
    if n > 3:
        m[3] = m[1]                                                                           # wholly hidden under an earlier row
    return m


@pytest.mark.parametrize("H,W", SHAPES)
def test_ground_truth_forms(H, W):
    for n_pred, ng in ((40, 25), (1, 1), (0, 25), (40, 0)):
        p = seeded_map(H, W, n_pred, 10)
        dense = overlapping_masks(H, W, ng, 11)
        glab = instances.label_map_host(dense)                                                # the first row wins an overlap
        want = lm.contingency_host(p, glab, n_pred, ng)
        conf = np.linspace(0.9, 0.1, n_pred)
        pd = up(p)
        forms = {"device map": (up(glab), ng), "host map": (glab, ng), "bits": BitMasks.from_words(bitmasks.pack_host(dense), H, W, pd.device),
                 "dense host": dense, "dense device": up(dense)}
        ref = lm.LabelEvaluator()
        ref.add((p, n_pred), (glab, ng), conf)
        for name, gt in forms.items():
            ev = lm.LabelEvaluator()
            assert ev.add((pd, n_pred), gt, conf) == want, (name, n_pred, ng)
            a, b = ev.summary(), ref.summary()
            assert all(same(a[k], b[k]) for k in a), name
        if ng > 3 and H * W > 100:
            assert (dense.sum(0) > 1).any() and want.area_gt[3] == 0
    with pytest.raises(lm.KGLibraryError):
        lm.LabelEvaluator().add((up(seeded_map(H, W, 1, 10)), 1), (np.zeros((H + 1, W), np.int32), 0))


def same(a, b):
    if a is None or b is None:
        return a is b
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cal_model():
    from oracle import weightgen
    m = KGnet.resnet50(pretrained=False)
    m.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    return m.to(DEV).eval()


def test_tiled_result_scored_on_the_device_equals_the_host_route(cal_model):
    H, W, S = 400, 600, 256
    img = np.random.default_rng(8).integers(0, 256, (H, W, 3), dtype=np.uint8)
    r = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4)
    n = len(r)
    assert n > 10 and tuple(r.labels.shape) == (H, W)
    lab = r.labels.cpu().numpy()
    # a seeded ground truth of about as many instances: half of them the prediction's own ids moved by a pixel, the rest rectangles
    rng = np.random.default_rng(9)
    n_gt = n
    gt = np.zeros((H, W), np.int32)
    for i in range(1, n_gt + 1):
        y, x = rng.integers(0, H), rng.integers(0, W)
        gt[y:y + rng.integers(4, 30), x:x + rng.integers(4, 30)] = i
    moved = np.roll(lab, (1, 1), (0, 1))
    keep = (moved > 0) & (moved % 2 == 0)
    gt[keep] = moved[keep]
    ev = lm.LabelEvaluator()
    c = ev.add(r, (up(gt), n_gt))
    host = lm.LabelEvaluator()
    ch = host.add((lab, n), (gt, n_gt), r.dets[:, 4])
    assert c == ch and len(c.pairs) > n // 2
    got, want = ev.summary(), host.summary()
    print({k: got[k] for k in ("kaggle", "pq", "sq", "dq", "aji", "dice")}, "pairs", len(c.pairs), "instances", n)
    assert set(got) == set(want) and all(same(got[k], want[k]) for k in got), (got, want)
    assert got["images"] == 1 and 0 < got["kaggle"] < 1 and 0 < got["aji"] < 1 and got["seg_ap"][0] > 0
    # the table's columns are the stats of the label map: no stats launch was needed for the prediction
    assert np.array_equal(lm.label_stats(r.labels, n), r.table[:, 1:6])
    # against its own label map
    own = lm.LabelEvaluator()
    own.add(r, (r.labels, n))
    s = own.summary()
    assert s["kaggle"] == 1.0 and s["pq"] == 1.0 and s["aji"] == 1.0 and s["dice"] == 1.0
    # evaluate_tiled: the same image through the public entry
    s2 = lm.evaluate_tiled(cal_model, [(img, (gt, n_gt))], tile=S, overlap=64, batch=4)
    assert all(same(s2[k], got[k]) for k in got)
