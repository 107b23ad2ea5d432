"""GPU: exact thinning on the device (csrc/thinning.hip, thinning.py) against the host statement of the same semantics
(thinning.midlines_host: the rule by shifted comparisons with integer sums and a minimum; the device evaluates a Boolean circuit on 32
pixels per word).  Every comparison is exact integer equality.  Shapes are the smallest at which the kernel can go wrong: one-pixel,
one-row and one-column maps, box widths on and either side of the 32-bit word pitch, objects and bars that cross the word boundaries
(the carry), boxes at the four map edges, both sides of the size rule, the deepest square that fits, rings, a comb, a checkerboard, a
serpentine, noise, pass limits, ids of any int32, boxes that cut or overhang, hostile job tables between guards, several images in one
launch, more jobs than the grid cap, out= reuse, and the predict routes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import thinning_cases as tc  # noqa: E402
from kg_instance_segmentation_amd import KGnet, _lib, inference, instances, tiling  # noqa: E402
from kg_instance_segmentation_amd import components as cc  # noqa: E402
from kg_instance_segmentation_amd import distance as dt  # noqa: E402
from kg_instance_segmentation_amd import measure as ms  # noqa: E402
from kg_instance_segmentation_amd import runlengths as rl  # noqa: E402
from kg_instance_segmentation_amd import split as sp  # noqa: E402
from kg_instance_segmentation_amd import thinning as th  # noqa: E402

DEV = "cuda"
I32 = np.iinfo(np.int32)
E = _lib.KGLibraryError


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def job_fits(jobs, nimg, H, W):
    j = np.asarray(jobs, np.int64).reshape(-1, 6)
    h = np.maximum(np.minimum(j[:, 4], H) - np.maximum(j[:, 2], 0), 0)
    w = np.maximum(np.minimum(j[:, 5], W) - np.maximum(j[:, 3], 0), 0)
    live = (j[:, 0] >= 0) & (j[:, 0] < nimg) & (h > 0) & (w > 0)
    return ~live | np.array([th.fits(a, b) for a, b in zip(h, w)], bool)


def same_as_host(lab, jobs, max_passes=None):
    """the raw entry and thin (with the host route of the boxes that do not fit) against midlines_host -> (skel, rows) of the host"""
    lab = np.asarray(lab, np.int32)
    jobs = np.asarray(jobs, np.int64).reshape(-1, 6)
    want, mid = th.midlines_host(lab, jobs, max_passes)
    wrows = mid.rows
    nimg = 1 if lab.ndim == 2 else lab.shape[0]
    fit = job_fits(jobs, nimg, *lab.shape[-2:])
    d = up(lab)
    skel, rows = th.thin_rows(d, jobs, max_passes)
    assert skel.is_cuda and skel.dtype == torch.int32 and skel.shape == d.shape and rows.dtype == torch.int32 and rows.shape == (len(jobs), 9)
    rows = rows.cpu().numpy()
    assert np.array_equal(rows[fit], wrows[fit]) and np.array_equal(rows[~fit], np.tile([0] * 8 + [1], ((~fit).sum(), 1)))
    if fit.all():
        assert np.array_equal(skel.cpu().numpy(), want)
    assert torch.equal(d, up(lab))                                      # the input is left alone
    skel2, mid2 = th.thin(d, jobs=jobs, max_passes=max_passes)
    assert np.array_equal(skel2.cpu().numpy(), want) and mid2.skel is skel2
    assert np.array_equal(mid2.rows[:, :8], wrows[:, :8]) and np.array_equal(mid2.rows[:, 8], (~fit).astype(np.int64))
    return want, wrows


def whole(lab, v=1):
    return [[0, v, 0, 0, *np.asarray(lab).shape]]


# ---- smallest maps, widths around the word pitch, the carry, the edges ----------------------------------------------------------------------

def test_one_pixel():
    skel, rows = same_as_host(np.ones((1, 1), np.int32), [[0, 1, 0, 0, 1, 1]])
    assert skel.tolist() == [[1]] and rows[0].tolist() == [1, 1, 1, 0, 0, 0, 0, 0, 0]
    skel, rows = same_as_host(np.ones((1, 1), np.int32), [[0, 2, 0, 0, 1, 1]])
    assert skel.tolist() == [[0]] and not rows.any()


@pytest.mark.parametrize("n", [2, 30, 31, 32, 62, 63, 64, 257])
@pytest.mark.parametrize("col", [False, True])
def test_one_row_and_one_column_maps(n, col):
    lab = np.ones((n, 1) if col else (1, n), np.int32)
    lab.reshape(-1)[n // 2] = 0 if n > 40 else 1                        # the long ones in two pieces
    skel, rows = same_as_host(lab, whole(lab))
    assert np.array_equal(skel, lab) and rows[0, 7] == 0 and rows[0, 3] == (2 if n <= 40 else 4)


@pytest.mark.parametrize("w", [30, 31, 62, 63, 94])
def test_box_widths_around_the_word_pitch(w):
    rng = np.random.default_rng(w)
    lab = (rng.random((19, w + 5)) < 0.7).astype(np.int32)
    lab[3:12, :] = 1                                                    # a thick band through every column, noise above and below
    for x1 in (0, 2, 5):
        skel, rows = same_as_host(lab, [[0, 1, 0, x1, 19, x1 + w]])
        assert rows[0, 7] >= 3 and rows[0, 1] > 0
    same_as_host(lab, [[0, 1, 1, 2, 18, 2 + w], [0, 1, 0, 0, 19, w + 5], [0, 0, 0, 1, 19, 1 + w]])


@pytest.mark.parametrize("edge", [30, 31, 32, 62, 63, 64])
def test_the_carry_between_words(edge):
    """Box column c sits at bit c + 1: the columns 30 .. 32 and 62 .. 64 lie around the word boundaries.  A disc's boundary, a vertical
    and a diagonal 3-pixel bar and a horizontal bar's end are put across column `edge`."""
    H, W = 64, 100
    yy, xx = np.mgrid[0:H, 0:W]
    lab = np.zeros((H, W), np.int32)
    lab[(yy - 14) ** 2 + (xx - edge + 9) ** 2 <= 100] = 1               # the disc's right boundary reaches column edge + 1
    lab[28:60, edge - 1:edge + 2] = 2                                   # a vertical bar centred on the column
    lab[(np.abs((xx - edge) - (yy - 40)) <= 1) & (yy >= 30) & (yy < 52) & (lab == 0)] = 3    # a diagonal bar through it
    lab[60:63, 3:edge + 1] = 4                                          # a horizontal bar that ends at the column
    jobs = [[0, v, 0, 0, H, W] for v in (1, 2, 3, 4)] + [[0, 2, 20, edge - 1, 64, edge + 2], [0, 4, 58, 0, 64, edge + 1]]
    skel, rows = same_as_host(lab, jobs)
    assert (rows[:4, 7] > 0).all() and (rows[:4, 1] > 0).all()
    same_as_host(np.ascontiguousarray(lab.T), [[0, v, 0, 0, W, H] for v in (1, 2, 3, 4)])


def test_boxes_at_the_four_map_edges():
    H, W = 45, 70
    lab = np.zeros((H, W), np.int32)
    lab[0:7, 5:60] = 1
    lab[H - 7:, 8:66] = 2
    lab[10:35, 0:5] = 3
    lab[9:36, W - 6:] = 4
    lab[0:4, 0:4] = 5
    lab[H - 3:, W - 3:] = 6
    jobs = [[0, 1, 0, 5, 7, 60], [0, 2, H - 7, 8, H, 66], [0, 3, 10, 0, 35, 5], [0, 4, 9, W - 6, 36, W], [0, 5, 0, 0, 4, 4], [0, 6, H - 3, W - 3, H, W],
            [0, 2, H - 7, 0, H, W], [0, 4, 0, W - 6, H, W]]
    skel, rows = same_as_host(lab, jobs)
    assert (rows[:, 1] > 0).all()


@pytest.mark.parametrize("h", [1, 2, 126])
def test_heights(h):
    rng = np.random.default_rng(h)
    lab = (rng.random((h, 77)) < 0.8).astype(np.int32)
    skel, rows = same_as_host(lab, whole(lab))
    assert rows[0, 0] == lab.sum() and rows[0, 1] > 0


@pytest.mark.parametrize("h,w", [(254, 510), (255, 510), (4094, 30), (4095, 30)])
def test_both_sides_of_the_size_rule(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    lab = ((yy // 9 + xx // 7) % 3 > 0).astype(np.int32)                 # a lattice of thick strokes: a few passes, many branch points
    lab[:, w - 2:] = 1
    lab[h - 2:, :] = 1
    skel, rows = same_as_host(lab, whole(lab))
    assert th.fits(h, w) == ((h + 2) * -(-(w + 2) // 32) <= 4096) == (h in (254, 4094)) and rows[0, 4] > 10 and rows[0, 7] >= 3
    assert skel[h // 2:].any() and skel[:, w // 2:].any()


# ---- object shapes ----------------------------------------------------------------------------------------------------------------------

def test_full_square_of_120():
    lab = np.ones((120, 120), np.int32)
    skel, rows = same_as_host(lab, whole(lab))
    assert rows[0, 0] == 14400 and rows[0, 7] == 60 and rows[0, 8] == 0


@pytest.mark.parametrize("shape", ["disc", "annulus", "nested", "comb", "checkerboard", "serpentine", "noise", "example"])
def test_shapes(shape):
    rng = np.random.default_rng(7)
    P = {"disc": tc.disc(18), "annulus": tc.annulus(), "nested": tc.nested_rings(), "comb": tc.comb(), "checkerboard": tc.checkerboard(41, 53),
         "serpentine": tc.serpentine(63), "noise": rng.random((64, 200)) < 0.6, "example": tc.pinned_example()[0] > 0}[shape]
    lab = P.astype(np.int32)
    skel, rows = same_as_host(lab, whole(lab))
    r = rows[0].tolist()
    if shape == "disc":
        assert r[1] == 3 and r[7] == 18
    if shape == "annulus":
        assert r[7] == 3 and r[2] == r[3] == r[4] == 0 and r[5] + r[6] == r[1]             # one closed ring
    if shape == "nested":
        assert r[2] == r[3] == r[4] == 0 and r[5] + r[6] == r[1]                           # two closed rings
    if shape == "comb":
        assert r[3] == 9 and r[4] == 7
    if shape == "checkerboard":
        assert r[7] == 0 and r[1] == r[0] and np.array_equal(skel, lab)
    if shape == "serpentine":
        assert r[3] == 2 and r[4] == 0 and r[5] + r[6] == r[1] - 1
    if shape == "example":
        assert r == tc.pinned_example()[2] and np.array_equal(skel > 0, tc.pinned_example()[1])
    same_as_host(np.ascontiguousarray(lab.T), whole(lab.T))


@pytest.mark.parametrize("limit", [1, 2, 0])
def test_max_passes(limit):
    lab = tc.blobs(90, 130, 7, 3, 5, 14)
    stats = tc.stats_of(lab, 7)
    jobs = np.concatenate([np.zeros((7, 1), np.int64), np.arange(1, 8)[:, None], stats[:, 1:]], 1)
    skel, rows = same_as_host(lab, jobs, limit)
    full, frows = th.midlines_host(lab, jobs)
    assert (rows[:, 7] <= limit).all() if limit else np.array_equal(rows, frows.rows)
    if limit:
        assert (rows[:, 1] > frows.rows[:, 1]).any() and not ((full > 0) & (skel == 0)).any()      # an erosion that keeps the midline inside


def test_any_int32_is_an_id():
    rng = np.random.default_rng(12)
    vals = np.array([0, -1, I32.min, I32.max, 5], np.int32)
    lab = vals[rng.integers(0, 5, (9, 11))].repeat(5, 0).repeat(5, 1)
    jobs = [[0, int(v), 0, 0, 45, 55] for v in vals]
    for k in range(5):
        skel, rows = same_as_host(lab, jobs[k:k + 1])
        assert rows[0, 0] == (lab == vals[k]).sum() and rows[0, 7] > 0
    same_as_host(lab, jobs)                                             # different ids never store the same pixel: all in one launch


def test_boxes_that_cut_or_overhang_and_a_duplicate():
    lab = tc.blobs(50, 64, 4, 7, 5, 12)
    jobs = [[0, 1, -5, -9, 30, 40], [0, 2, 10, 12, 80, 90], [0, 3, 20, 0, 21, 64], [0, 4, 0, 30, 50, 31], [0, 1, I32.min, I32.min, I32.max, I32.max],
            [0, 2, 10, 12, 80, 90]]
    for k in range(len(jobs)):
        same_as_host(lab, jobs[k:k + 1])
    same_as_host(lab, jobs)


def test_three_images_with_interleaved_jobs():
    labs = np.stack([tc.blobs(40, 75, 4, 30 + i, 3, 9) for i in range(3)])
    jobs = []
    for k in range(4):
        for i in (2, 0, 1):
            jobs.append([i, k + 1, *tc.stats_of(labs[i], 4)[k, 1:].tolist()])
    skel, rows = same_as_host(labs, jobs)
    assert (skel > 0).reshape(3, -1).any(1).all()
    skel2, mid = th.thin(up(labs), n=[4, 4, 4])                         # the boxes from the maps themselves
    assert np.array_equal(skel2.cpu().numpy(), skel) and len(mid) == 12
    skel3, mid3 = th.thin(up(labs), n=[4, 4, 4], stats=[tc.stats_of(labs[i], 4) for i in range(3)], max_passes=1)
    assert np.array_equal(skel3.cpu().numpy(), th.midlines_host(labs, [4, 4, 4], 1)[0])


def test_hostile_tables_between_guards():
    H, W, nimg = 24, 40, 2
    labs = np.stack([tc.blobs(H, W, 3, 50 + i, 3, 6) for i in range(nimg)])
    jobs = np.array([[-1, 1, 0, 0, H, W], [nimg, 1, 0, 0, H, W], [I32.max, 1, 0, 0, H, W], [I32.min, 1, 0, 0, H, W], [0, 1, H, W, 0, 0],
                     [1, 1, 5, 5, 5, 30], [0, 1, I32.max, I32.max, I32.min, I32.min], [1, 2, -I32.max, -I32.max, I32.max, I32.max],
                     [0, 2, 0, 0, H, W], [1, 3, H - 1, W - 1, I32.max, I32.max], [0, 77, 0, 0, H, W], [1, 1, I32.min, I32.min, I32.max, I32.max]], np.int64)
    want, mid = th.midlines_host(labs, jobs)
    wrows = mid.rows
    assert not wrows[:7].any() and wrows[7, 0] > 0 and not wrows[10].any()
    m = len(jobs)
    d = up(labs)
    jbuf = torch.full((m + 2, 6), I32.max, dtype=torch.int32, device=DEV)                 # guard rows a stray read would act on
    jbuf[1:-1] = up(jobs.astype(np.int32))
    sbuf = torch.full((nimg * H * W + 2 * W,), -5, dtype=torch.int32, device=DEV)
    rbuf = torch.full((m + 2, 9), 77, dtype=torch.int32, device=DEV)
    skel, rows = sbuf[W:-W], rbuf[1:-1]
    for limit in (0, 1):
        _lib.call("kg_label_thin", _lib.ptr(d), nimg, H, W, _lib.ptr(jbuf[1:-1]), m, limit, _lib.ptr(skel), _lib.ptr(rows), _lib.stream_ptr())
        torch.cuda.synchronize()
        want, mid = th.midlines_host(labs, jobs, limit)
        assert np.array_equal(skel.cpu().numpy().reshape(labs.shape), want) and np.array_equal(rows.cpu().numpy(), mid.rows)
        assert (sbuf[:W] == -5).all() and (sbuf[-W:] == -5).all() and (rbuf[0] == 77).all() and (rbuf[-1] == 77).all()
    same_as_host(labs, jobs)


def test_more_jobs_than_the_grid_cap():
    """1 048 584 jobs, more than the 2^20 workgroups of a launch: the first eight blocks take a second job and write their LDS bitmaps
    again.  Jobs 0 .. 3 and 2^20 + 4 .. 2^20 + 7 thin an object of id 7 in boxes of their own, the others are one-pixel jobs with a
    closed form: a pixel of value 1 is its own midline."""
    H, W, m = 1025, 1024, (1 << 20) + 8
    idx = np.arange(H * W, dtype=np.int64)
    lab = (1 + (idx % 3 == 0)).astype(np.int32).reshape(H, W)
    lab[100:136, 100:157] = 7 * tc.comb(6, 25, 5, 5, 9)                 # 36 x 57
    yy, xx = np.divmod(idx[:m], W)
    jobs = np.stack([np.zeros(m, np.int64), np.ones(m, np.int64), yy, xx, yy + 1, xx + 1], 1)
    special = [0, 1, 2, 3, (1 << 20) + 4, (1 << 20) + 5, (1 << 20) + 6, (1 << 20) + 7]
    for s, k in enumerate(special):
        jobs[k] = [0, 7, 100 + s, 100, 141, 161 - 3 * s]
    skel, rows = th.thin_rows(up(lab), jobs)
    skel, rows = skel.cpu().numpy(), rows.cpu().numpy()
    wskel, wmid = th.midlines_host(lab, jobs[special])
    assert (wmid.rows[:, 7] > 0).all() and np.array_equal(rows[special], wmid.rows)
    one = np.ones(m, bool)
    one[special] = False
    is1 = lab.reshape(-1)[:m] == 1
    want_rows = np.zeros((m, 9), np.int32)
    want_rows[is1, :3] = 1
    assert np.array_equal(rows[one], want_rows[one])
    want = wskel.reshape(-1).copy()
    want[:m][one & is1] = 1
    assert np.array_equal(skel.reshape(-1), want)


def test_out_reuse_no_jobs_and_refusals():
    lab = tc.blobs(40, 50, 3, 5)
    d = up(lab)
    buf = torch.full_like(d, 9)
    skel, mid = th.thin(d, 3, out=buf)
    assert skel.data_ptr() == buf.data_ptr() and np.array_equal(buf.cpu().numpy(), th.midlines_host(lab, 3)[0])
    skel, mid = th.thin(d, jobs=[[0, 2, 0, 0, 40, 50]], out=buf)       # every element is written: nothing of the first call is left
    assert np.array_equal(buf.cpu().numpy(), th.midlines_host(lab, [[0, 2, 0, 0, 40, 50]])[0]) and (buf == 1).sum() == 0
    skel, rows = th.thin_rows(d, np.zeros((0, 6), np.int64), out=buf)
    assert not buf.any() and rows.shape == (0, 9)
    skel, mid = th.thin(d, jobs=np.zeros((0, 6), np.int64))
    assert not skel.any() and len(mid) == 0
    for bad in (buf[:, 1:], buf.long(), buf.cpu(), buf[None]):
        with pytest.raises(E):
            th.thin_rows(d, np.zeros((0, 6), np.int64), out=bad)
    for maps, jobs in ((lab, np.zeros((0, 6), np.int64)), (d.long(), np.zeros((0, 6), np.int64)), (d, np.zeros((1, 8), np.int64))):
        with pytest.raises(E):
            th.thin_rows(maps, jobs)
    for bad in (-1, 1.5, True):
        with pytest.raises(E):
            th.thin_rows(d, np.zeros((0, 6), np.int64), bad)
    with pytest.raises(E):
        th.thin(d, 3, jobs=[[0, 1, 0, 0, 4, 4]])
    j = up(np.array([[0, 1, 0, 0, 5, 5]], np.int32))
    r = torch.zeros(1, 9, dtype=torch.int32, device=DEV)
    o = torch.empty_like(d)
    for sk, limit, rr in ((d, 0, r), (o, -1, r), (o, 0, d.view(-1)[:9]), (o, 0, o.view(-1)[:9])):     # skel aliases labels; a negative limit;
        with pytest.raises(E):                                                                        # rows alias a map
            _lib.call("kg_label_thin", _lib.ptr(d), 1, *lab.shape, _lib.ptr(j), 1, limit, _lib.ptr(sk), _lib.ptr(rr), _lib.stream_ptr())
    with pytest.raises(E):
        _lib.call("kg_label_thin", _lib.ptr(d), 1, *lab.shape, _lib.ptr(j), 1, 0, _lib.ptr(o), _lib.ptr(j), _lib.stream_ptr())   # rows alias jobs


# ---- the family works on skel ---------------------------------------------------------------------------------------------------------------

def test_measure_and_runs_on_skel():
    n = 6
    lab = tc.blobs(80, 110, n, 21, 4, 12)
    skel, mid = th.thin(up(lab), n)
    host = skel.cpu().numpy()
    assert np.array_equal(ms.measure(skel, n).raw, ms.measure_host(host, n)) and np.array_equal(ms.measure_host(host, n)[:, 0], mid.pixels())
    assert rl.runs(skel, n) == rl.runs_host(host, n)


# ---- Instances, end to end ------------------------------------------------------------------------------------------------------------------

def sheet_instances(device=True):
    n = 9
    lab = tc.blobs(120, 150, n, 33, 4, 11)
    lab[1, 0] = 3                                                      # a speck of id 3 for the clean-up to drop
    stats = tc.stats_of(lab, n)
    dets = np.concatenate([stats[:, 1:].astype(np.float32), np.linspace(0.9, 0.5, n, dtype=np.float32)[:, None]], 1)
    table = tiling.table_from_labels_host(lab, np.concatenate([np.arange(1, n + 1)[:, None], stats[:, 1:]], 1), stats[:, 0])
    return instances.Instances(up(lab) if device else lab, dets, table, "the masks"), lab, n


@pytest.mark.parametrize("clean", [None, dict(min_area=4, connectivity=4)])
def test_thin_instances(clean):
    inst, lab, n = sheet_instances()
    hinst = sheet_instances(False)[0]
    if clean is not None:
        inst, hinst = cc.clean_instances(inst, **clean), cc.clean_instances(hinst, **clean)
    for limit in (None, 2):
        got, want = th.thin_instances(inst, limit), th.thin_instances(hinst, limit)
        assert got == want and len(got) == n and got.skel.is_cuda and np.array_equal(got.skel.cpu().numpy(), want.skel)
    grown = dt.expand_instances(sp.split_instances(inst, 3), 2)         # after a split and an expansion: from labels and table alone
    hgrown = instances.Instances(grown.labels.cpu().numpy(), grown.dets, grown.table, grown.masks)
    got, want = th.thin_instances(grown), th.thin_instances(hgrown)
    assert got == want and len(got) == len(grown) and np.array_equal(got.skel.cpu().numpy(), want.skel)
    out = th.thin_instances_batch([inst, None, grown], max_passes=1)
    assert out[1] is None and inst.midlines == th.thin_instances(hinst, 1) and grown.midlines == th.thin_instances(hgrown, 1)


@pytest.fixture(scope="module")
def cal_model():
    from oracle import weightgen
    m = KGnet.resnet50(pretrained=False)
    m.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    return m.to(DEV).eval()


def same_instances(a, b):
    return (torch.equal(a.labels, b.labels) and np.array_equal(a.dets, b.dets) and np.array_equal(a.table, b.table) and type(a) is type(b))


def host_of(inst):
    if isinstance(inst, tiling.TiledInstances):
        return tiling.TiledInstances(inst.labels.cpu().numpy(), inst.dets, inst.table, inst.tile, inst.origin, inst.tile_masks)
    return instances.Instances(inst.labels.cpu().numpy(), inst.dets, inst.table, inst.masks)


def test_predict_tiled_with_thin(cal_model):
    H, W, S = 400, 600, 256
    img = np.random.default_rng(8).integers(0, 256, (H, W, 3), dtype=np.uint8)
    plain = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4)
    none = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4, thin=None)
    assert len(plain) > 0 and plain.midlines is None and none.midlines is None and same_instances(plain, none)   # the default path is untouched
    for kw in (True, dict(max_passes=1)):
        got = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4, thin=kw)
        want = th.thin_instances(host_of(plain), **({} if kw is True else kw))
        assert same_instances(got, plain) and got.midlines == want and np.array_equal(got.midlines.skel.cpu().numpy(), want.skel)
        assert len(got.midlines) == len(got) and (got.midlines.pixels() > 0).any()
    policy = dict(min_area=4)
    both = tiling.predict_tiled(cal_model, up(img), tile=S, overlap=64, batch=4, clean=policy, split=2, expand=3, thin=True, measure=True)
    final = dt.expand_instances(sp.split_instances(cc.clean_instances(plain, **policy), 2), 3)
    want = th.thin_instances(host_of(final))
    assert same_instances(both, final) and both.midlines == want and np.array_equal(both.midlines.skel.cpu().numpy(), want.skel)
    assert len(both.midlines) == len(both) == len(both.measurements.raw)


def test_predict_instances_with_thin(cal_model):
    S = 256
    src = np.random.default_rng(9).integers(0, 256, (2, S, S, 3), dtype=np.uint8)
    x = torch.cat([tiling.cut_tiles(src[i], tiling.plan(S, S, S, 64)) for i in range(2)])
    plain = inference.predict_instances(cal_model, x)
    none = inference.predict_instances(cal_model, x, thin=None)
    assert all(p is not None and len(p) > 0 and q.midlines is None and same_instances(p, q) for p, q in zip(plain, none))
    got = inference.predict_instances(cal_model, x, thin=True)
    full = inference.predict_instances(cal_model, x, clean=dict(min_area=4), split=2, expand=2, thin=dict(max_passes=2), runs=True)
    for p, g, f in zip(plain, got, full):
        want = th.thin_instances(host_of(p))
        assert same_instances(g, p) and g.midlines == want and np.array_equal(g.midlines.skel.cpu().numpy(), want.skel)
        ref = dt.expand_instances(sp.split_instances(cc.clean_instances(p, min_area=4), 2), 2)
        want = th.thin_instances(host_of(ref), 2)
        assert same_instances(f, ref) and f.midlines == want and np.array_equal(f.midlines.skel.cpu().numpy(), want.skel) and len(f.runs) == len(f)
