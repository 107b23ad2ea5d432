"""GPU: the nearest-other-label transform and its products (csrc/distance.hip, distance.py) against the host statement of the same semantics
(distance.*_host, a plain minimum over offsets).  Every comparison is exact integer equality.  Shapes are the smallest at which the kernel
can go wrong: one-pixel, one-row and one-column maps, the exact disc around one pixel, sources on both sides of every tile seam with a
window that spans three tiles, ragged blobs at every radius class, checkerboards, one value only, extreme values with ties, three images
in one launch, box widths on both sides of the 256-thread walk, hostile job tables, bands."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from kg_instance_segmentation_amd import KGnet, _lib, inference, tiling  # noqa: E402
from kg_instance_segmentation_amd import components as cc  # noqa: E402
from kg_instance_segmentation_amd import distance as dt  # noqa: E402
from kg_instance_segmentation_amd import measure as ms  # noqa: E402
from kg_instance_segmentation_amd._lib import ptr, stream_ptr  # noqa: E402

DEV = "cuda"
I32 = np.iinfo(np.int32)
BOTH = (("d2", "nearest"),)
EVERY = (("d2",), ("nearest",), ("d2", "nearest"))


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def blob_map(H, W, n, seed):
    """A seeded ragged map: ellipses and rectangles with ids 1 .. n painted over each other, some cut by the frame, some touching."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    lab = np.zeros((H, W), np.int32)
    for i in range(1, n + 1):
        cy, cx = rng.integers(0, H), rng.integers(0, W)
        ry, rx = rng.integers(1, max(H // 4, 2) + 1), rng.integers(1, max(W // 6, 2) + 1)
        sel = (np.abs(yy - cy) <= ry) & (np.abs(xx - cx) <= rx) if i % 2 else ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
        lab[sel & (rng.random((H, W)) < 0.93)] = i
    return lab


def check(lab, max_d2, frame=False, wants=BOTH):
    """distance on the device equals distance_host; -> the host pair"""
    lab = np.ascontiguousarray(lab, np.int32)
    wd, wn = dt.distance_host(lab, max_d2, frame)
    d = up(lab)
    for want in wants:
        gd, gn = dt.distance(d, max_d2, frame, want=want)
        assert (gd is None) == ("d2" not in want) and (gn is None) == ("nearest" not in want)
        if gd is not None:
            assert gd.dtype == torch.int32 and gd.shape == d.shape and np.array_equal(gd.cpu().numpy(), wd), (max_d2, frame, want)
        if gn is not None:
            assert gn.dtype == torch.int32 and gn.shape == d.shape and np.array_equal(gn.cpu().numpy(), wn), (max_d2, frame, want)
    return wd, wn


@pytest.mark.parametrize("max_d2", [1, 4096])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 130), (130, 1)])
def test_smallest_maps(H, W, max_d2):
    lab = np.full((1, 1), 7, np.int32) if H * W == 1 else blob_map(H, W, 9, 10 + H)
    for frame in (False, True):
        wd, wn = check(lab, max_d2, frame)
        if H * W == 1:
            assert wd.tolist() == [[1 if frame else max_d2 + 1]] and wn.tolist() == [[7]]
    assert H * W == 1 or (wd == 1).any()


@pytest.mark.parametrize("max_d2", [1, 2, 4095, 4096])
def test_exact_disc_around_one_pixel(max_d2):
    lab = np.zeros((140, 140), np.int32)
    lab[70, 70] = 5
    wd, wn = check(lab, max_d2)
    yy, xx = np.mgrid[0:140, 0:140]
    r2 = (yy - 70) ** 2 + (xx - 70) ** 2
    disc = (r2 <= max_d2) & (r2 > 0)
    assert np.array_equal(wn, np.where(disc, 5, 0)) and np.array_equal(wd[disc], r2[disc]) and wd[70, 70] == 1 and wn[70, 70] == 0
    assert (wd[~disc & (r2 > 0)] == max_d2 + 1).all() and (r2[disc].max() == 4096) == (max_d2 == 4096)
    out = dt.expand_labels(up(lab), 64 if max_d2 == 4096 else np.sqrt(max_d2))
    assert np.array_equal(out.cpu().numpy(), np.where(r2 <= max_d2, 5, 0))


@pytest.mark.parametrize("max_d2", [1, 25, 1024, 4096])
def test_tile_seams(max_d2):
    """Sources on both sides of every seam and in the last row and column; with R >= the tile side a window spans three tiles."""
    TH, TW = dt.TILE_H, dt.TILE_W
    H, W = 2 * TH + 3, 2 * TW + 5
    lab = np.zeros((H, W), np.int32)
    k = 0
    for y in (TH - 1, TH, TH + 1, H - 1):
        for x in (TW - 1, TW, TW + 1, W - 1):
            k += 1
            lab[y, x] = k if k % 3 else -k
    lab[2, 3], lab[2 * TH, 5], lab[7, 2 * TW] = 40, 41, 42
    for frame in (False, True):
        check(lab, max_d2, frame)
    sparse = np.zeros((H, W), np.int32)                                # one source per seam crossing: nothing stops a scan early
    sparse[TH, 0], sparse[0, TW], sparse[H - 1, TW - 1], sparse[TH - 1, W - 1] = 1, 2, 3, 4
    check(sparse, max_d2)


BLOBS = blob_map(70, 131, 40, 170)


@pytest.mark.parametrize("frame", [False, True])
@pytest.mark.parametrize("max_d2", [1, 2, 5, 9, 100, 1024, 4096])
def test_blobs(max_d2, frame):
    wd, wn = check(BLOBS, max_d2, frame, EVERY)
    assert (wd == 1).any() and (wn != BLOBS).any() and ((wd == max_d2 + 1).any() or max_d2 > 100)
    # the raw entry between guard rows: nothing is written in front of or behind the maps
    H, W = BLOBS.shape
    d = up(BLOBS)
    g1 = torch.full(((H + 2) * W,), -7, dtype=torch.int32, device=DEV)
    g2 = torch.full(((H + 2) * W,), -7, dtype=torch.int32, device=DEV)
    _lib.call("kg_label_distance", ptr(d), 1, H, W, max_d2, int(frame), ptr(g1[W:]), ptr(g2[W:]), stream_ptr())
    a, b = g1.cpu().numpy().reshape(H + 2, W), g2.cpu().numpy().reshape(H + 2, W)
    assert np.array_equal(a[1:-1], wd) and np.array_equal(b[1:-1], wn)
    assert (a[0] == -7).all() and (a[-1] == -7).all() and (b[0] == -7).all() and (b[-1] == -7).all()


@pytest.mark.parametrize("max_d2", [1, 8, 100])
def test_checkerboards(max_d2):
    yy, xx = np.mgrid[0:70, 0:131]
    two = np.where((yy + xx) % 2, 3, -4).astype(np.int32)
    four = np.array([I32.min, 0, 9, I32.max], np.int32)[(yy % 2) * 2 + xx % 2]
    for lab in (two, four):
        wd, wn = check(lab, max_d2, False)
        assert (wd == 1).all()
        check(lab, max_d2, True)
    assert np.array_equal(wn[:-1, :-1][(yy % 2 == 1)[:-1, :-1] & (xx % 2 == 1)[:-1, :-1]], np.full(34 * 65, 0))   # I32.max sees 0 and 9 at 1


@pytest.mark.parametrize("max_d2", [9, 100])
def test_one_value_only(max_d2):
    H, W = 100, 200                                                    # the middle tile lies farther than R from every side
    lab = np.full((H, W), -6, np.int32)
    wd, wn = check(lab, max_d2, False)
    assert (wd == max_d2 + 1).all() and (wn == -6).all()
    wd, wn = check(lab, max_d2, True)
    yy, xx = np.mgrid[0:H, 0:W]
    f = np.minimum(np.minimum(yy + 1, xx + 1), np.minimum(H - yy, W - xx))
    assert np.array_equal(wd, np.where(f * f <= max_d2, f * f, max_d2 + 1)) and (wn == -6).all()
    assert np.array_equal(dt.shrink_labels(up(lab), 3, frame=True).cpu().numpy(), np.where(f > 3, -6, 0))


@pytest.mark.parametrize("max_d2", [2, 49])
def test_extreme_values_and_ties(max_d2):
    rng = np.random.default_rng(6)
    vals = np.array([I32.min, -1, 0, 0, 0, 5, I32.max], np.int64)
    lab = vals[rng.integers(0, len(vals), (37, 70))].astype(np.int32)
    lab[rng.random((37, 70)) < 0.5] = 0
    lab[10:21, 30:50] = 0
    lab[15, 29], lab[15, 50], lab[9, 40], lab[21, 40] = I32.max, I32.min, -1, I32.min   # (9, 40) and (21, 40): equally far from (15, 40)
    wd, wn = check(lab, max_d2, False)
    check(lab, max_d2, True)
    assert (wn == I32.min).any() and (wn == I32.max).any() and (wn == -1).any()
    if max_d2 == 49:
        assert wd[15, 40] == 36 and wn[15, 40] == I32.min and wd[14, 40] == 25 and wn[14, 40] == -1 and wn[16, 40] == I32.min


def test_three_images_in_one_launch():
    H, W, max_d2 = 40, 70, 1024
    lab = np.zeros((3, H, W), np.int32)
    lab[1, 0, ::3] = np.arange(1, 25)
    lab[2, H - 1, 1::3] = -np.arange(1, 24)
    wd, wn = dt.distance_host(lab, max_d2)
    gd, gn = dt.distance(up(lab), max_d2)
    assert gd.shape == (3, H, W) and np.array_equal(gd.cpu().numpy(), wd) and np.array_equal(gn.cpu().numpy(), wn)
    assert (wd[0] == max_d2 + 1).all() and (wn[0] == 0).all() and (wd[1:] <= max_d2).any((1, 2)).all()
    for i in range(3):
        od, on = dt.distance(up(lab[i]), max_d2)
        assert torch.equal(od, gd[i]) and torch.equal(on, gn[i])
    assert np.array_equal(dt.expand_labels(up(lab), 30).cpu().numpy(), dt.expand_labels_host(lab, 30))


def raw_regrow(lab, max_d2, frame, op, lo2, hi2):
    d = up(lab)
    out = torch.empty_like(d)
    _lib.call("kg_label_regrow", ptr(d), 1, lab.shape[0], lab.shape[1], max_d2, int(frame), op, lo2, hi2, ptr(out), stream_ptr())
    return out.cpu().numpy()


@pytest.mark.parametrize("dist", [1, 2.3, 7, 30])
def test_regrow_equals_the_host_compositions(dist):
    lab, d = BLOBS, up(BLOBS)
    assert np.array_equal(dt.expand_labels(d, dist).cpu().numpy(), dt.expand_labels_host(lab, dist))
    for frame in (False, True):
        assert np.array_equal(dt.shrink_labels(d, dist, frame).cpu().numpy(), dt.shrink_labels_host(lab, dist, frame))
    for inner in (0, dist / 2, dist - 0.01):
        assert np.array_equal(dt.ring_labels(d, inner, dist).cpu().numpy(), dt.ring_labels_host(lab, inner, dist))
    # the raw entry: hi2 < max_d2, and lo2 == hi2 (an empty ring)
    hi2 = int(dist * dist)
    max_d2 = min(2 * hi2 + 3, 4096)
    wd, wn = dt.distance_host(lab, max_d2)
    fd, _ = dt.distance_host(lab, max_d2, True)
    assert np.array_equal(raw_regrow(lab, max_d2, 0, dt.EXPAND, 0, hi2), np.where((lab == 0) & (wd <= hi2), wn, lab))
    assert np.array_equal(raw_regrow(lab, max_d2, 0, dt.RING, hi2 // 2, hi2), np.where((lab == 0) & (wd > hi2 // 2) & (wd <= hi2), wn, 0))
    assert np.array_equal(raw_regrow(lab, max_d2, 1, dt.SHRINK, 0, hi2), np.where((lab != 0) & (fd > hi2), lab, 0))
    assert not raw_regrow(lab, max_d2, 0, dt.RING, hi2, hi2).any()


def test_inscribed_walk_widths_hostile_jobs_and_bands():
    H, W, nimg = 40, 300, 2
    lab = np.ones((nimg, H, W), np.int32)
    rng = np.random.default_rng(4)
    lab[0][rng.random((H, W)) < 0.002] = 0
    lab[1] = blob_map(H, W, 9, 5)
    max_d2 = 100
    d2 = dt.distance_host(lab, max_d2, True)[0]
    jobs = [[0, 1, 3, 7, 40, 7 + w] for w in (1, 2, 255, 256, 257)] + [
        [0, 1, 0, 0, H, W], [1, 3, -50, -50, H + 50, W + 50], [1, 3, I32.min, I32.min, I32.max, I32.max],
        [0, 1, 20, 30, 10, 40], [0, 1, 5, 5, 5, 9],                   # inverted, empty
        [1, 77, 0, 0, H, W], [1, 0, 0, 0, H, W],                       # an absent id; the background is a value like any other
        [nimg, 1, 0, 0, H, W], [-1, 1, 0, 0, H, W], [I32.max, 1, 0, 0, H, W], [I32.min, 1, 0, 0, H, W],
        [1, 4, H - 1, W - 1, H + 9, W + 9], [1, 4, H, W, H + 9, W + 9]]
    jobs = np.array(jobs, np.int64)
    want = dt.inscribed_rows_host(lab, d2, jobs)
    assert want[:6, 3].tolist() == [int(np.count_nonzero(lab[0, 3:40, 7:7 + w])) for w in (1, 2, 255, 256, 257)] + [int(lab[0].sum())]
    assert want[8:11].tolist() == [[0, -1, -1, 0]] * 3 and want[12:16].tolist() == [[0, -1, -1, 0]] * 4 and want[11, 3] > 0
    d, dd = up(lab), up(d2)
    guard = torch.full((len(jobs) + 2, 4), -7, dtype=torch.int32, device=DEV)
    _lib.call("kg_label_inscribed", ptr(d), ptr(dd), nimg, H, W, ptr(up(jobs.astype(np.int32))), len(jobs), ptr(guard[1:]), stream_ptr())
    g = guard.cpu().numpy()
    assert np.array_equal(g[1:-1], want) and (g[0] == -7).all() and (g[-1] == -7).all()
    assert dt.inscribed_rows(d, dd, np.zeros((0, 6), np.int64)).shape == (0, 4)          # m == 0 launches nothing
    whole = dt.inscribed_host(lab, jobs=jobs, max_d2=max_d2, frame=True)
    assert np.array_equal(whole[["d2max", "y", "x", "count"]].tolist(), [tuple(r) for r in want.tolist()])
    for cap in (65536, 1000, 37):                                      # unsplit; bands of whole rows; row pieces
        got = dt.inscribed(d, jobs=jobs, max_d2=max_d2, frame=True, max_job_pixels=cap)
        assert got.dtype == dt.INSCRIBED_DTYPE and np.array_equal(got, whole), cap
    # n / stats, and an instance thicker than the search radius
    by_n = dt.inscribed(d[1], 9, max_d2=max_d2)
    assert np.array_equal(by_n, dt.inscribed_host(lab[1], 9, max_d2=max_d2))
    stats = ms.labelmetrics.label_stats_host(lab[1], 9)
    assert np.array_equal(dt.inscribed(d[1], 9, stats=stats, max_d2=max_d2), by_n)
    thick = np.zeros((30, 30), np.int32)
    thick[3:27, 4:28] = 1
    sat = dt.inscribed(up(thick), 1, max_d2=16)
    assert sat[0]["saturated"] and sat[0]["d2max"] == 17 and (sat[0]["y"], sat[0]["x"]) == (7, 8) and sat[0]["count"] == 576
    assert np.array_equal(sat, dt.inscribed_host(thick, 1, max_d2=16))


def test_argument_refusals():
    H, W = 8, 9
    d = torch.zeros(H * W + 4, dtype=torch.int32, device=DEV)
    o = torch.zeros(H * W + 4, dtype=torch.int32, device=DEV)
    p, q, s = d.data_ptr(), o.data_ptr(), stream_ptr()

    def refused(match, name, *args):
        with pytest.raises(_lib.KGLibraryError, match=match):
            _lib.call(name, *args, s)
    refused("both NULL", "kg_label_distance", p, 1, H, W, 4, 0, None, None)
    refused("misaligned", "kg_label_distance", p + 2, 1, H, W, 4, 0, q, None)
    refused("misaligned", "kg_label_distance", p, 1, H, W, 4, 0, None, q + 1)
    refused("alias", "kg_label_distance", p, 1, H, W, 4, 0, p, None)
    refused("alias", "kg_label_distance", p, 1, H, W, 4, 0, q, p)
    refused("alias", "kg_label_distance", p, 1, H, W, 4, 0, q, q)
    refused(r"max_d2 0 \(1 \.\. 4096\)", "kg_label_distance", p, 1, H, W, 0, 0, q, None)
    refused(r"max_d2 4097 \(1 \.\. 4096\)", "kg_label_distance", p, 1, H, W, 4097, 0, q, None)
    refused("bad size", "kg_label_distance", p, 0, H, W, 4, 0, q, None)
    refused(r"exceeds 2\^31 - 1", "kg_label_distance", p, 3, 2 ** 15, 2 ** 15, 4, 0, q, None)
    refused("null pointer", "kg_label_distance", None, 1, H, W, 4, 0, q, None)
    refused("frame must be 0", "kg_label_regrow", p, 1, H, W, 4, 1, 0, 0, 4, q)
    refused("frame must be 0", "kg_label_regrow", p, 1, H, W, 4, 1, 1, 0, 4, q)
    refused("lo2 <= hi2", "kg_label_regrow", p, 1, H, W, 4, 0, 1, 3, 2, q)
    refused("lo2 <= hi2", "kg_label_regrow", p, 1, H, W, 4, 0, 0, 0, 5, q)
    refused("lo2 1 must be 0", "kg_label_regrow", p, 1, H, W, 4, 0, 0, 1, 4, q)
    refused("lo2 1 must be 0", "kg_label_regrow", p, 1, H, W, 4, 0, 2, 1, 4, q)
    refused("op 3", "kg_label_regrow", p, 1, H, W, 4, 0, 3, 0, 4, q)
    refused("aliases labels", "kg_label_regrow", p, 1, H, W, 4, 0, 0, 0, 4, p)
    refused("misaligned", "kg_label_regrow", p, 1, H, W, 4, 0, 0, 0, 4, q + 2)
    refused("null pointer", "kg_label_regrow", p, 1, H, W, 4, 0, 0, 0, 4, None)
    j = torch.zeros(6, dtype=torch.int32, device=DEV).data_ptr()
    refused("null pointer", "kg_label_inscribed", p, None, 1, H, W, j, 1, q)
    refused("null pointer", "kg_label_inscribed", p, q, 1, H, W, None, 1, q)
    refused("misaligned", "kg_label_inscribed", p, q + 2, 1, H, W, j, 1, q + 16)
    refused("aliases", "kg_label_inscribed", p, q, 1, H, W, j, 1, q)
    refused("bad size", "kg_label_inscribed", p, q, 1, H, W, j, -1, q)
    assert not bool(o.any()) and not bool(d.any())                    # nothing was launched


# ---- end to end -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cal_model():
    from oracle import weightgen
    m = KGnet.resnet50(pretrained=False)
    m.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    return m.to(DEV).eval()


def same_instances(a, b):
    return (torch.equal(a.labels, b.labels) and np.array_equal(a.dets, b.dets) and np.array_equal(a.table, b.table) and type(a) is type(b)
            and a.table.dtype == b.table.dtype)


def expanded_as_stated(got, plain, dist):
    """got = plain with its labels expanded on the host and its table taken from that map over the whole image"""
    n = len(plain)
    want = dt.expand_labels_host(plain.labels.cpu().numpy(), dist)
    assert type(got) is type(plain) and len(got) == n and np.array_equal(got.dets, plain.dets)
    assert got.labels.is_cuda and got.labels.dtype == torch.int32 and np.array_equal(got.labels.cpu().numpy(), want)
    H, W = want.shape
    jobs = np.concatenate([np.arange(1, n + 1)[:, None], np.tile([0, 0, H, W], (n, 1))], 1)
    assert got.table.dtype == np.int64 and np.array_equal(got.table, tiling.table_from_labels_host(want, jobs, plain.table[:, 0]))
    assert (got.table[:, 1] >= plain.table[:, 1]).all() and got.table[:, 1].sum() > plain.table[:, 1].sum()
    assert ((got.table[:, 1] == 0) == (plain.table[:, 1] == 0)).all()
    return want


def test_predict_tiled_with_expand(cal_model):
    H, W, S = 400, 600, 256
    img = np.random.default_rng(8).integers(0, 256, (H, W, 3), dtype=np.uint8)
    plain = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4)
    n = len(plain)
    print("instances", n)
    assert n > 0 and same_instances(tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4, expand=None), plain)
    got = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4, expand=5)
    expanded_as_stated(got, plain, 5)
    assert got.measurements is None and np.array_equal(got.tile, plain.tile) and np.array_equal(got.origin, plain.origin)
    assert same_instances(dt.expand_instances(plain, 5), got)
    # with clean= and measure=: cleaned, then expanded, then measured
    policy = dict(min_area=4)
    cleaned = cc.clean_instances(plain, **policy)
    both = tiling.predict_tiled(cal_model, up(img), tile=S, overlap=64, batch=4, clean=policy, measure=True, expand=5)
    final = expanded_as_stated(both, cleaned, 5)
    assert np.array_equal(both.measurements.raw, ms.measure_host(final, n, img))
    assert np.array_equal(both.measurements.raw[:, 0], both.table[:, 1])


def test_predict_instances_with_expand(cal_model):
    S = 256
    src = np.random.default_rng(9).integers(0, 256, (2, S, S, 3), dtype=np.uint8)
    x = torch.cat([tiling.cut_tiles(src[i], tiling.plan(S, S, S, 64)) for i in range(2)])
    sizes = [(S, S), (200, 230)]
    plain = inference.predict_instances(cal_model, x, image_sizes=sizes)
    assert all(p is not None and len(p) > 0 for p in plain) and [tuple(p.labels.shape) for p in plain] == sizes
    none = inference.predict_instances(cal_model, x, image_sizes=sizes, expand=None)
    got = inference.predict_instances(cal_model, x, image_sizes=sizes, expand=5, measure=True)
    for p, q, g in zip(plain, none, got):
        assert same_instances(p, q) and q.measurements is None
        final = expanded_as_stated(g, p, 5)
        assert np.array_equal(g.measurements.raw, ms.measure_host(final, len(p)))
    same = inference.predict_instances(cal_model, torch.cat([x, x[:1]]), expand=5)         # two images of one size share a launch
    assert torch.equal(same[0].labels, same[2].labels) and np.array_equal(same[0].table, same[2].table)
