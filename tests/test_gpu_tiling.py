"""GPU: tiled whole-image inference (csrc/tiling.hip, tiling.py) against the host statements of the same semantics (tiling.*_host), and
predict_tiled end to end against the by-hand route over the same tiles.  Every comparison is exact equality.  Shapes are the smallest
at which the kernels can go wrong: unaligned tile origins, widths that are no multiple of the lane's pixel group, tiles that reach past
the image, pixels under one to six tiles, word tails, coordinate sums past 2^31."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from kg_instance_segmentation_amd import KGnet, bitmasks, inference, instances, tiling  # noqa: E402
from kg_instance_segmentation_amd.bitmasks import BitMasks  # noqa: E402

DEV = "cuda"


def device():
    return torch.device(DEV, torch.cuda.current_device())


def seeded_masks(n, H, W, seed, smax=12):
    """n seeded ellipses (even rows) and rectangles (odd rows), uint8 [n, H, W]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((n, H, W), np.uint8)
    for k in range(n):
        cy, cx, ry, rx = rng.integers(0, H), rng.integers(0, W), rng.integers(1, smax + 1), rng.integers(1, smax + 1)
        m[k] = (np.abs(yy - cy) <= ry) & (np.abs(xx - cx) <= rx) if k % 2 else ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
    return m


# ---- cut ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,grid", [(70, 131, (3, 3)), (20, 50, (1, 1)), (32, 64, (1, 1))])
def test_cut(H, W, grid):
    img = np.random.default_rng(100 * H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    img[0, 0] = (0, 255, 1)
    img[H - 1, W - 1] = (255, 0, 254)
    p = tiling.plan(H, W, (32, 64), 8)
    assert p.shape == grid
    if grid == (3, 3):
        assert p.ys.tolist() == [0, 19, 38] and p.xs.tolist() == [0, 33, 67] and W % 4                # unaligned origins, a ragged last group
    want = tiling.cut_tiles_host(img, p)
    got = tiling.cut_tiles(img, p)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (len(p), 3, 32, 64)
    g = got.cpu().numpy()
    assert np.array_equal(g, want)
    assert torch.equal(tiling.cut_tiles(torch.from_numpy(img).to(DEV), p), got)                       # a device image
    half = np.float32(0.5)
    for t, (y0, x0) in enumerate(p.origins):                                                          # stated once more without the host function
        vh, vw = p.valid(t)
        for c in range(3):
            assert np.array_equal(g[t, c, :vh, :vw], img[y0:y0 + vh, x0:x0 + vw, c].astype(np.float32) / np.float32(255) - half)
        assert np.all(g[t, :, vh:] == -half) and np.all(g[t, :, :, vw:] == -half)                     # the padding is exactly -0.5
    assert g[0, :, 0, 0].tolist() == [-0.5, 0.5, np.float32(1) / np.float32(255) - half]


# ---- clip -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 65])
@pytest.mark.parametrize("vh,vw", [(3, 70), (5, 64), (5, 130)])
def test_clip(n, vh, vw):
    H, W = 5, 130
    ld = bitmasks.ld_words(H, W)
    assert ld == 16 and H * bitmasks.words_per_row(W) == 15                                           # a padding word
    rng = np.random.default_rng(1000 * n + 10 * vh + vw)
    words = rng.integers(0, 2 ** 64, (n + 2, ld), dtype=np.uint64)                                    # every bit seeded, two rows beyond n
    dev_words = torch.from_numpy(words.view(np.int64)).to(DEV)
    m = BitMasks(dev_words[:n], H, W)
    assert tiling.clip_masks(m, vh, vw) is m
    got = dev_words.cpu().numpy().view(np.uint64)
    want = words.copy()
    want[:n] = tiling.clip_words_host(words[:n], H, W, vh, vw)
    assert np.array_equal(got, want)
    assert np.array_equal(got[n:], words[n:]) and np.array_equal(got[:, 15], words[:, 15])           # rows beyond n, the padding word
    if n:
        dense, before = bitmasks.unpack_host(got[:n], H, W), bitmasks.unpack_host(words[:n], H, W)
        assert not dense[:, vh:].any() and not dense[:, :, vw:].any() and np.array_equal(dense[:, :vh, :vw], before[:, :vh, :vw])
        assert ((vh, vw) == (H, W)) == np.array_equal(got, words)                                     # the full window is a no-op


# ---- stitch ---------------------------------------------------------------------------------------------------------------------------

def seeded_tile_labels(p, seed, zeros=0.5):
    rng = np.random.default_rng(seed)
    tl = rng.integers(1, 2 ** 31, (len(p), p.th, p.tw)).astype(np.int32)
    tl[rng.random(tl.shape) < zeros] = 0
    tl.reshape(-1)[:4] = (2 ** 31 - 1, 1, 0, 2 ** 31 - 1)
    return tl


def test_stitch():
    grids = {"four": tiling.TilePlan(tiling.plan_axis(97, 40, 16), tiling.plan_axis(101, 64, 16), 40, 64, 97, 101),
             "one": tiling.plan(32, 64, (32, 64), 8), "small": tiling.plan(20, 50, (32, 64), 8), "wide": tiling.plan(33, 700, (32, 64), 8)}
    p = grids["four"]
    assert p.ys.tolist() == [0, 19, 38, 57] and p.xs.tolist() == [0, 37]
    cover = np.zeros((97, 101), np.int64)
    for y0, x0 in p.origins:
        cover[y0:y0 + 40, x0:x0 + 64] += 1
    assert sorted(np.unique(cover).tolist()) == [1, 2, 3, 4, 6]                                       # one to six tiles over a pixel
    assert grids["one"].shape == (1, 1) and grids["small"].shape == (1, 1) and grids["wide"].shape == (2, 13)        # more than one block per row
    for name, p in grids.items():
        for seed, zeros in ((1, 0.5), (2, 0.97), (3, 1.1)):                                           # (the last: all-zero tile maps)
            tl = seeded_tile_labels(p, seed, zeros) if zeros <= 1 else np.zeros((len(p), p.th, p.tw), np.int32)
            want = tiling.stitch_host(tl, p)
            got = tiling.stitch(torch.from_numpy(tl).to(DEV), p)
            assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (p.H, p.W)
            assert np.array_equal(got.cpu().numpy(), want), (name, seed)
            assert (zeros > 1) == (not want.any())


# ---- table ----------------------------------------------------------------------------------------------------------------------------

def tight_boxes(dense):
    out = np.zeros((len(dense), 4), np.int64)
    for k, m in enumerate(dense):
        ys, xs = np.nonzero(m)
        if len(ys):
            out[k] = ys.min(), xs.min(), ys.max() + 1, xs.max() + 1
    return out


@pytest.mark.parametrize("n", [0, 1, 300])
def test_table(n):
    H, W = 97, 301
    dense = seeded_masks(n, H, W, 40 + n, smax=14)
    if n == 300:
        dense[0] = 0
        dense[0, H - 1, W - 1] = 1                                                                    # the last pixel of the map
        dense[1] = 0
        dense[1, :, 0] = dense[1, 0, :] = dense[1, :, W - 1] = dense[1, H - 1, :] = 1                 # a frame: touches all four borders
        dense[1, H - 1, W - 1] = 0
        dense[7] = dense[3]                                                                           # hidden under an earlier instance
    lab = instances.label_map_host(dense)
    boxes = tight_boxes(dense)
    jobs = np.concatenate([np.arange(1, n + 1)[:, None], boxes], 1).astype(np.int32)
    full = dense.sum((1, 2), dtype=np.int64)
    lab_d = torch.from_numpy(lab).to(DEV)
    got = tiling.table_from_labels(lab_d, jobs, torch.from_numpy(full).to(DEV))
    assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == (n, 8)
    got = got.cpu().numpy()
    assert np.array_equal(got, tiling.table_from_labels_host(lab, jobs, full))
    assert np.array_equal(got, instances.table_host(dense))                                           # tight boxes: the table of the masks
    if n == 300:
        assert not got[7, 1:].any() and got[7, 0] > 0 and got[1, 2:6].tolist() == [0, 0, H, W] and got[0].tolist() == [1, 1, H - 1, W - 1, H, W, H - 1, W - 1]
        assert (got[:, 1] < got[:, 0]).sum() > 20                                                     # overlaps do occur
        # other boxes over the same map: the whole image, boxes of zero area, a box that cuts its instance, no area_full
        other = jobs.copy()
        other[0, 1:] = 0, 0, H, W
        other[1, 1:] = 5, 9, 5, 40
        other[2, 1:] = H, W, H, W
        other[4, 3] = (other[4, 1] + other[4, 3]) // 2
        other[5, 0] = 2 ** 31 - 1                                                                     # an id nothing carries
        g2 = tiling.table_from_labels(lab_d, other).cpu().numpy()
        assert np.array_equal(g2, tiling.table_from_labels_host(lab, other)) and not g2[:, 0].any()
        assert not g2[1, 1:].any() and not g2[2, 1:].any() and not g2[5, 1:].any() and np.array_equal(g2[0], np.r_[0, got[0, 1:]])
        with pytest.raises(tiling.KGLibraryError):
            tiling.table_from_labels(lab_d, np.array([[1, 0, 0, H + 1, W]]))


def test_table_box_widths_around_the_walk():
    H, W = 40, 300
    lab = np.ones((H, W), np.int32)
    jobs = np.array([[1, 3, 7, 40, 7 + w] for w in (1, 2, 255, 256, 257)] + [[1, H - 1, 0, H, W], [1, 0, W - 1, H, W]], np.int32)
    want = tiling.table_from_labels_host(lab, jobs)
    assert want[:, 1].tolist() == [37, 74, 37 * 255, 37 * 256, 37 * 257, W, H]
    assert want[4].tolist() == [0, 37 * 257, 3, 7, 40, 264, 257 * sum(range(3, 40)), 37 * sum(range(7, 264))]
    got = tiling.table_from_labels(torch.from_numpy(lab).to(DEV), jobs).cpu().numpy()
    assert np.array_equal(got, want)


def test_table_sums_of_a_full_image():
    """One instance over a whole 1040 x 1388 map, one job over all of it: sum_y is 749 478 240 and sum_x 1 001 081 120 from 1 443 520
    pixels in ONE workgroup; a second job over a 1040 x 2100 map passes 2^31."""
    for H, W in ((1040, 1388), (1040, 2100)):
        lab = torch.ones(H, W, dtype=torch.int32, device=DEV)
        area = torch.tensor([H * W], dtype=torch.int64, device=DEV)
        got = tiling.table_from_labels(lab, np.array([[1, 0, 0, H, W]]), area).cpu().numpy()
        sum_y, sum_x = W * (H * (H - 1) // 2), H * (W * (W - 1) // 2)
        assert got.tolist() == [[H * W, H * W, 0, 0, H, W, sum_y, sum_x]]
    assert sum_x > 2 ** 31


# ---- label_map(ids=...) -----------------------------------------------------------------------------------------------------------------

def test_label_map_ids():
    H, W = 24, 70
    dense = seeded_masks(70, H, W, 22, smax=9)
    m = BitMasks.from_words(bitmasks.pack_host(dense), H, W, device())
    rng = np.random.default_rng(23)
    ids = rng.integers(1, 2 ** 31, 70).astype(np.int32)
    ids[:2] = 2 ** 31 - 1, 1
    plain, ptab = instances.label_map(m)
    assert np.array_equal(plain[0].cpu().numpy(), instances.label_map_host(dense))                    # without ids: unchanged
    lab, tab = instances.label_map(m, ids=ids)
    assert np.array_equal(lab[0].cpu().numpy(), instances.label_map_host(dense, ids=ids)) and torch.equal(tab, ptab)
    lab_dev, _ = instances.label_map(m, ids=torch.from_numpy(ids).to(DEV), with_table=False)
    assert torch.equal(lab_dev, lab)
    rs = [0, 5, 5, 70]
    lab, _ = instances.label_map(m, rs, ids=ids)
    for i, (a, b) in enumerate(zip(rs[:-1], rs[1:])):
        assert np.array_equal(lab[i].cpu().numpy(), instances.label_map_host(dense[a:b], ids=ids[a:b]))
    for bad in (dict(ids=ids[:-1]), dict(ids=ids, priority=np.arange(70)), dict(ids=ids.astype(np.float32)), dict(ids=ids.astype(np.int64) << 4),
                dict(ids=torch.from_numpy(ids)), dict(ids=torch.from_numpy(ids.astype(np.int64)).to(DEV))):
        with pytest.raises(tiling.KGLibraryError):
            instances.label_map(m, **bad)
    none, _ = instances.label_map(BitMasks.empty(H, W, device()), ids=np.zeros(0, np.int32))
    assert tuple(none.shape) == (1, H, W) and int(none.abs().max()) == 0


# ---- assemble on seeded tiles (no model) ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,tile,overlap", [(150, 170, 64, 32), (20, 50, (32, 64), 8)])
def test_assemble_equals_host(H, W, tile, overlap):
    p = tiling.plan(H, W, tile, overlap)
    rng = np.random.default_rng(6)
    n = 90
    tile_of = rng.integers(0, len(p), n)
    y1, x1 = rng.integers(0, p.th - 4, n), rng.integers(0, p.tw - 4, n)
    y2, x2 = np.minimum(y1 + rng.integers(2, 30, n), p.th - 1), np.minimum(x1 + rng.integers(2, 30, n), p.tw - 1)
    conf = rng.random(n).astype(np.float32)
    conf[5] = conf[50]
    masks = np.zeros((n, p.th, p.tw), np.uint8)
    for i in range(n):
        masks[i, y1[i]:y2[i], x1[i]:x2[i]] = rng.random((y2[i] - y1[i], x2[i] - x1[i])) < 0.8
    host, dev = [None] * len(p), [None] * len(p)
    buf = BitMasks.from_words(bitmasks.pack_host(masks), p.th, p.tw, device())
    for t in range(len(p)):
        if len(p) > 1 and t == len(p) - 1:
            continue                                                                                  # a tile without detections: None
        k = np.flatnonzero(tile_of == t) if len(p) > 1 else np.arange(n)
        k = k[np.argsort(-conf[k], kind="stable")]
        dets = np.stack([y1[k], x1[k], y2[k], x2[k], conf[k]], 1).astype(np.float32)
        host[t], dev[t] = [masks[k], dets], [buf[k], dets]
    want = tiling.assemble_host(p, host)
    got = tiling.assemble(p, dev)
    assert len(want) > 10 and isinstance(got, tiling.TiledInstances) and isinstance(got, instances.Instances) and got.masks is None
    assert got.labels.is_cuda and got.labels.dtype == torch.int32 and np.array_equal(got.labels.cpu().numpy(), want.labels)
    assert got.dets.dtype == np.float32 and np.array_equal(got.dets, want.dets)
    assert got.table.dtype == np.int64 and np.array_equal(got.table, want.table)
    assert got.tile.dtype == np.int32 and np.array_equal(got.tile, want.tile) and np.array_equal(got.origin, want.origin)
    assert np.array_equal(bitmasks.unpack_host(got.tile_masks.words_cpu(), p.th, p.tw), want.tile_masks)
    if len(p) > 1:
        assert len(np.unique(got.tile)) > 5 and (want.table[:, 1] < want.table[:, 0]).any()
    else:
        assert masks[:, H:].any() and masks[:, :, W:].any() and not want.tile_masks[:, H:].any() and not want.tile_masks[:, :, W:].any()      # clipped
    empty = tiling.assemble(p, [None] * len(p))
    assert empty.labels.is_cuda and tuple(empty.labels.shape) == (H, W) and int(empty.labels.abs().max()) == 0 and len(empty) == 0
    assert empty.table.shape == (0, 8) and len(empty.tile_masks) == 0


# ---- end to end -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cal_model():
    from oracle import weightgen
    m = KGnet.resnet50(pretrained=False)
    m.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    return m.to(DEV).eval()


def masks_inside_boxes(r, p):
    """every set bit of every tile mask lies inside its det box (tile pixels)"""
    dense = bitmasks.unpack_host(r.tile_masks.words_cpu(), p.th, p.tw)
    box = np.rint(r.dets[:, :4]).astype(np.int64) - np.concatenate([r.origin, r.origin], 1)
    for m, (y1, x1, y2, x2) in zip(dense, box):
        inside = np.zeros_like(m)
        inside[y1:y2, x1:x2] = 1
        if (m & ~inside & 1).any():
            return False
    return True


def test_single_tile_equals_predict_instances(cal_model):
    S = 256
    img = np.random.default_rng(7).integers(0, 256, (S, S, 3), dtype=np.uint8)
    r = tiling.predict_tiled(cal_model, img, tile=S, overlap=64)
    p = tiling.plan(S, S, S, 64)
    assert len(p) == 1
    g = inference.predict_instances(cal_model, tiling.cut_tiles(img, p))[0]
    assert g is not None and len(g) > 0
    print("detections", len(g))
    assert torch.equal(r.labels, g.labels) and tuple(r.labels.shape) == (S, S)
    assert np.array_equal(r.dets, g.dets) and np.array_equal(r.table, g.table)
    assert torch.equal(r.tile_masks.words, g.masks.words) and not r.tile.any() and not r.origin.any()
    assert masks_inside_boxes(r, p)


def test_stitched_image_equals_the_route_by_hand(cal_model):
    H, W, S = 400, 600, 256
    img = np.random.default_rng(8).integers(0, 256, (H, W, 3), dtype=np.uint8)
    r = tiling.predict_tiled(cal_model, img, tile=S, overlap=64, batch=4)
    p = tiling.plan(H, W, S, 64)
    assert p.shape == (2, 3) and p.ys.tolist() == [0, 144] and p.xs.tolist() == [0, 172, 344]
    x = tiling.cut_tiles_host(img, p)
    preds = []
    for a in (0, 4):                                                                                  # the same two chunks
        preds += inference.predict(cal_model, torch.from_numpy(x[a:a + 4]).to(DEV), packed=True)
    want = tiling.assemble_host(p, [None if q is None else [q[0].numpy(), q[1]] for q in preds])
    n = len(want)
    print("detections per tile", [0 if q is None else len(q[1]) for q in preds], "kept", n, "tiles", np.unique(want.tile).tolist())
    lab = r.labels.cpu().numpy()
    assert len(r) == n and np.array_equal(lab, want.labels)
    assert np.array_equal(r.dets, want.dets) and np.array_equal(r.tile, want.tile) and np.array_equal(r.origin, want.origin)
    assert np.array_equal(r.table, want.table)
    assert np.array_equal(bitmasks.unpack_host(r.tile_masks.words_cpu(), S, S), want.tile_masks)
    assert np.array_equal(instances.rle_decode(instances.rle_encode(lab), H, W), lab)
    assert np.all(np.diff(r.dets[:, 4]) <= 0)
    # what makes this a test of stitching
    assert len(np.unique(r.tile)) >= 2                                                                # at least two tiles contribute
    cover = np.zeros((H, W), np.int64)
    for y0, x0 in p.origins:
        cover[y0:y0 + S, x0:x0 + S] += 1
    assert ((lab > 0) & (cover > 1)).any()                                                            # a labelled pixel in an overlap band
    assert masks_inside_boxes(r, p)                                                                   # what the table's boxes rest on
    # the stitched map is the label map of the global masks in id order
    glob = np.zeros((n, H, W), np.uint8)
    for i, (t, (y0, x0)) in enumerate(zip(want.tile, want.origin)):
        vh, vw = p.valid(t)
        glob[i, y0:y0 + vh, x0:x0 + vw] = want.tile_masks[i, :vh, :vw]
    assert np.array_equal(lab, instances.label_map_host(glob)) and np.array_equal(r.table, instances.table_host(glob))
