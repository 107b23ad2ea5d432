"""GPU: connected components of label maps and the clean-up policy (csrc/components.hip, components.py) against the host statements of the
same semantics (components.*_host), and clean= through predict_tiled / predict_instances / LabelEvaluator end to end.  Every comparison
is exact integer equality.  Shapes: a single pixel, a single row, a single column, one 64 x 64 tile exactly, one pixel either side of a
tile edge, and several tiles in both directions with ragged last tiles."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from kg_instance_segmentation_amd import KGnet, _lib, inference, tiling  # noqa: E402
from kg_instance_segmentation_amd import components as cc  # noqa: E402
from kg_instance_segmentation_amd import labelmetrics as lm  # noqa: E402

DEV = "cuda"
SHAPES = [(1, 1), (1, 67), (67, 1), (63, 65), (64, 64), (65, 129), (130, 200)]
CONN = [(4, 0), (4, 4), (8, 0), (8, 4)]


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def seeded_map(H, W, n, seed):
    """test_gpu_labelmetrics.py's seeded blocky map: rectangles painted over each other, corners, one run over a whole row."""
    rng = np.random.default_rng(1000 * H + 10 * W + 7 * n + seed)
    lab = np.zeros((H, W), np.int32)
    for i in range(1, n + 1):
        y, x = rng.integers(0, H), rng.integers(0, W)
        lab[y:y + rng.integers(1, H // 3 + 2), x:x + rng.integers(1, W // 2 + 2)] = i
    lab[H // 2, :] = 1
    lab[0, 0], lab[0, W - 1], lab[H - 1, 0], lab[H - 1, W - 1] = 1, n, 1, n
    lab[lab == n - 1] = 0
    return lab


def serpentine(H, W, v=3):
    """One pixel wide, through every row: full even rows joined by single pixels at alternating ends of the odd rows."""
    lab = np.zeros((H, W), np.int32)
    lab[0::2] = v
    odd = np.arange(1, H, 2)
    lab[odd, np.where((odd // 2) % 2 == 0, W - 1, 0)] = v
    return lab


def comb(H, W, v=2):
    """Vertical teeth two pixels apart, joined only along the last row."""
    lab = np.zeros((H, W), np.int32)
    lab[:, 0::2] = v
    lab[H - 1] = v
    return lab


@functools.lru_cache(maxsize=None)
def maps(H, W):
    yy, xx = np.mgrid[:H, :W]
    rng = np.random.default_rng(H * 1000 + W)
    extreme = np.array([0, -2 ** 31, -1, 2 ** 31 - 1], np.int64)[rng.integers(0, 4, ((H + 2) // 3, (W + 2) // 3))]
    extreme = np.repeat(np.repeat(extreme, 3, 0), 3, 1)[:H, :W].astype(np.int32)
    out = {"seeded": seeded_map(H, W, 12, 0), "zeros": np.zeros((H, W), np.int32), "one": np.full((H, W), 7, np.int32),
           "checker": (((yy + xx) % 2) * 3).astype(np.int32), "serpentine": serpentine(H, W), "comb": comb(H, W),
           "comb_mirrored": comb(H, W)[::-1].copy(), "extreme": extreme}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def host(H, W, name, conn, bg):
    """(comp, m, stats) of a map by the host statements: computed once, shared, never changed."""
    lab = maps(H, W)[name]
    comp, m = cc.components_host(lab, conn, bg)
    stats = cc.component_stats_host(lab, comp, m)
    comp.setflags(write=False)
    stats.setflags(write=False)
    return comp, m, stats


# ---- components and stats on every shape --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("conn,bg", CONN)
@pytest.mark.parametrize("H,W", SHAPES)
def test_components_and_stats_equal_the_host_statements(H, W, conn, bg):
    for name, lab in maps(H, W).items():
        want, m, want_stats = host(H, W, name, conn, bg)
        d = up(lab)
        comp, ncomp = cc.components(d, conn, bg)
        assert comp.dtype == torch.int32 and tuple(comp.shape) == (H, W) and ncomp.dtype == torch.int32 and tuple(ncomp.shape) == (1,)
        got = comp.cpu().numpy()
        assert int(ncomp.item()) == m and np.array_equal(got, want), (name, int(ncomp.item()), m, np.argwhere(got != want)[:4])
        if name == "extreme":                       # (values are compared, never used as an index: components only)
            continue
        stats, start = cc.component_stats(d, comp, ncomp)
        assert stats.dtype == np.int64 and start.tolist() == [0, m] and np.array_equal(stats, want_stats), (name, stats[:3], want_stats[:3])
    # what the shapes are for
    if (conn, bg) == (4, 0):
        assert host(H, W, "checker", 4, 0)[1] == H * W // 2 and host(H, W, "zeros", 4, 0)[1] == 0
        assert host(H, W, "one", 4, 0)[2].tolist() == [[7, H * W, 0, 0, H, W, 1, -1, -1]]
    if conn == 8 and min(H, W) >= 2:
        assert host(H, W, "checker", 8, 0)[1] == 1
    assert host(H, W, "serpentine", conn, 0)[1] == 1 and host(H, W, "comb", conn, 0)[1] == 1 and host(H, W, "comb_mirrored", conn, 0)[1] == 1


def test_diagonal_contacts_across_a_tile_corner():
    H, W = 130, 200
    lab = np.zeros((H, W), np.int32)
    lab[63, 63] = lab[64, 64] = 5                   # two pixels that touch only diagonally across the tile corner
    lab[63, 64] = lab[64, 63] = 9                   # and two more across the other diagonal of the same corner
    lab[63, 128] = lab[64, 127] = 5                 # the same at the next corner along the row ...
    lab[127, 64] = lab[128, 63] = 9                 # ... and at a corner one tile row down
    for conn, m in ((8, 4), (4, 8)):
        for bg in (0, 4):
            comp, ncomp = cc.components(up(lab), conn, bg)
            want, wm = cc.components_host(lab, conn, bg)
            assert wm == m + (bg != 0) and int(ncomp.item()) == wm and np.array_equal(comp.cpu().numpy(), want)
    c8 = cc.components_host(lab, 8, 0)[0]
    assert c8[63, 63] == c8[64, 64] != c8[63, 64] == c8[64, 63] and c8[63, 128] == c8[64, 127] and c8[127, 64] == c8[128, 63]


def test_images_of_a_stack_are_independent():
    H, W = 37, 70
    lab = np.stack([seeded_map(H, W, 6, k) for k in range(3)])
    lab[:, 0] = 4                                   # the last row of every image and the first row of the next hold the same id
    lab[:, H - 1] = 4
    assert not np.array_equal(lab[0], lab[1]) and not np.array_equal(lab[1], lab[2])
    for conn, bg in CONN:
        comp, ncomp = cc.components(up(lab), conn, bg)
        want, wm = cc.components_host(lab, conn, bg)
        got = comp.cpu().numpy()
        assert ncomp.cpu().numpy().tolist() == wm.tolist() and np.array_equal(got, want)
        assert all(got[k, 0, 0] == 1 for k in range(3))                                      # numbering restarts in every image
        stats, start = cc.component_stats(up(lab), comp, ncomp)
        assert start.tolist() == np.concatenate([[0], np.cumsum(wm)]).tolist()
        assert np.array_equal(stats, cc.component_stats_host(lab, want, wm))


def test_stats_of_a_rings_hole():
    lab = np.zeros((70, 90), np.int32)
    lab[10:69, 5:80] = 3
    lab[20:66, 30:70] = 0                           # a hole that crosses tile seams
    lab[1, 1] = 3
    comp, ncomp = cc.components(up(lab), 8, 4)
    stats, _ = cc.component_stats(up(lab), comp, ncomp)
    assert np.array_equal(stats, cc.component_stats_host(lab, *cc.components_host(lab, 8, 4)))
    assert stats.tolist() == [[0, 70 * 90 - 59 * 75 - 1, 0, 0, 70, 90, 1, 2, 3], [3, 1, 1, 1, 2, 2, 0, 1, 1],
                              [3, 59 * 75 - 46 * 40, 10, 5, 69, 80, 0, 1, 4], [0, 46 * 40, 20, 30, 66, 70, 0, 3, 3]]


def test_stats_where_a_wave_walks_several_segments():
    """The stats walk is a grid of 2048 waves that stride over the 64-pixel row segments, each carrying one component from segment to
    segment: 420 x 6 segments make some waves walk two, in one image and across the images of a stack."""
    H, W = 420, 330
    lab = seeded_map(H, W, 40, 2)
    for conn, bg in ((8, 4), (4, 0)):
        want, m = cc.components_host(lab, conn, bg)
        comp, ncomp = cc.components(up(lab), conn, bg)
        assert int(ncomp.item()) == m and np.array_equal(comp.cpu().numpy(), want)
        stats, _ = cc.component_stats(up(lab), comp, ncomp)
        assert np.array_equal(stats, cc.component_stats_host(lab, want, m))
    stack = np.stack([lab[:150], lab[150:300], np.zeros((150, W), np.int32)])
    want, m = cc.components_host(stack, 8, 4)
    comp, ncomp = cc.components(up(stack), 8, 4)
    stats, start = cc.component_stats(up(stack), comp, ncomp)
    assert np.array_equal(comp.cpu().numpy(), want) and start[-1] == m.sum() and np.array_equal(stats, cc.component_stats_host(stack, want, m))


def test_remap_raw_with_a_comp_value_outside_the_components():
    H, W = 65, 129
    lab = maps(H, W)["seeded"]
    comp, m, _ = host(H, W, "seeded", 8, 4)
    bad = comp.copy()
    bad[3, 5], bad[64, 128], bad[10, 10] = m + 1, -7, 2 ** 31 - 1
    newval = (np.arange(m, dtype=np.int32) * 3 + 11)
    want = np.concatenate([[0], newval])[comp].astype(np.int32)
    want[3, 5] = want[64, 128] = want[10, 10] = 0
    d, nv, out = up(bad), up(newval), torch.full((H, W), -1, dtype=torch.int32, device=DEV)
    start = (ctypes.c_int * 2)(0, m)
    _lib.call("kg_component_remap", _lib.ptr(d), 1, H, W, start, m, _lib.ptr(nv), _lib.ptr(out), _lib.stream_ptr())
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(cc.remap(up(comp), [0, m], newval).cpu().numpy(), np.concatenate([[0], newval])[comp])
    assert lab.shape == (H, W)


def test_two_runs_give_identical_components():
    H, W = 130, 200
    for name in ("serpentine", "comb", "comb_mirrored"):
        for conn, bg in ((8, 4), (4, 8)):
            d = up(maps(H, W)[name])
            a, na = cc.components(d, conn, bg)
            b, nb = cc.components(d, conn, bg)
            assert torch.equal(a, b) and torch.equal(na, nb)


# ---- the policy -------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def planted(H, W, n):
    """The seeded map with rings, specks and split ids planted in it."""
    lab = seeded_map(H, W, n, 1).copy()
    lab[5:16, 8:22] = 2; lab[8:12, 12:17] = 0                                               # a ring of id 2 ...
    lab[9, 13] = 3                                                                          # ... with a speck of id 3 in its hole
    lab[30:40, 60:75] = 4; lab[33, 64] = 0; lab[35:37, 68:70] = 0                           # pin-holes of areas 1 and 4
    lab[50:54, 100:104] = 5; lab[58:60, 110:111] = 5; lab[20, 120] = 5                      # id 5 in three pieces
    lab[60:64, 60:68] = 6; lab[62, 64] = 5                                                  # a fragment of 5 inside 6, across a tile seam
    lab[0:3, 30:40] = 7; lab[0, 33] = 0                                                     # a notch in the border: not a hole
    lab.setflags(write=False)
    return lab


@pytest.mark.parametrize("relabel", [False, True])
@pytest.mark.parametrize("fill_holes", [True, False])
@pytest.mark.parametrize("min_area", [0, 5])
@pytest.mark.parametrize("keep", ["largest", "all"])
def test_clean_equals_clean_host(keep, min_area, fill_holes, relabel):
    n = 12
    for H, W, conn in ((65, 129, 8), (130, 200, 4)):
        lab = planted(H, W, n)
        old = np.zeros((n, 8), np.int64)
        old[:, 0] = 1000 + np.arange(n)
        policy = dict(keep=keep, min_area=min_area, fill_holes=fill_holes, relabel=relabel, connectivity=conn, table=old)
        want = cc.clean_host(lab, n, **policy)
        got = cc.clean(up(lab), n, **policy)
        assert len(got) == len(want) == (3 if relabel else 2)
        assert got[0].dtype == torch.int32 and np.array_equal(got[0].cpu().numpy(), want[0])
        assert got[1].dtype == np.int64 and np.array_equal(got[1], want[1])
        if relabel:
            assert got[2].dtype == np.int32 and np.array_equal(got[2], want[2])
        nothing_to_do = keep == "all" and min_area == 0 and not fill_holes and not relabel
        assert (want[0] != lab).any() != nothing_to_do
    with pytest.raises(_lib.KGLibraryError, match=r"pixel\(s\) of the label map lie outside \[0, 3\]"):
        cc.clean(up(planted(65, 129, n)), 3)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cal_model():
    from oracle import weightgen
    m = KGnet.resnet50(pretrained=False)
    m.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    return m.to(DEV).eval()


def same_instances(a, b):
    return (torch.equal(a.labels, b.labels) and np.array_equal(a.dets, b.dets) and np.array_equal(a.table, b.table) and type(a) is type(b)
            and a.table.dtype == b.table.dtype)


def same(a, b):
    if a is None or b is None:
        return a is b
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def test_predict_tiled_with_clean(cal_model):
    H, W, S = 96, 160, 64
    img = np.random.default_rng(8).integers(0, 256, (H, W, 3), dtype=np.uint8)
    plain = tiling.predict_tiled(cal_model, img, tile=S, overlap=16, batch=4)
    assert same_instances(tiling.predict_tiled(cal_model, img, tile=S, overlap=16, batch=4, clean=None), plain)
    n = len(plain)
    assert n > 0
    got = tiling.predict_tiled(cal_model, img, tile=S, overlap=16, batch=4, clean=dict(min_area=4))
    after = cc.clean_instances(plain, min_area=4)
    assert same_instances(got, after) and isinstance(got, tiling.TiledInstances)
    assert got.tile is not None and np.array_equal(got.tile, plain.tile) and np.array_equal(got.origin, plain.origin)
    want_map, want_table = cc.clean_host(plain.labels.cpu().numpy(), n, min_area=4, table=plain.table)
    print("instances", n, "pixels changed", int((want_map != plain.labels.cpu().numpy()).sum()))
    assert np.array_equal(got.labels.cpu().numpy(), want_map) and np.array_equal(got.table, want_table)
    # the cleaned result is scored like any other: on the device, equal to the host route over the cleaned map
    rng = np.random.default_rng(9)
    n_gt = max(n, 3)
    gt = np.zeros((H, W), np.int32)
    for i in range(1, n_gt + 1):
        y, x = rng.integers(0, H), rng.integers(0, W)
        gt[y:y + rng.integers(4, 30), x:x + rng.integers(4, 30)] = i
    ev, hv = lm.LabelEvaluator(), lm.LabelEvaluator()
    c = ev.add(got, (up(gt), n_gt))
    ch = hv.add((want_map, n), (gt, n_gt), got.dets[:, 4])
    a, b = ev.summary(), hv.summary()
    assert c == ch and set(a) == set(b) and all(same(a[k], b[k]) for k in a), (a, b)
    s = lm.evaluate_tiled(cal_model, [(img, (gt, n_gt))], tile=S, overlap=16, batch=4, clean=dict(min_area=4))
    assert all(same(s[k], a[k]) for k in a)


def test_predict_instances_with_clean(cal_model):
    S = 64
    img = np.random.default_rng(8).integers(0, 256, (96, 160, 3), dtype=np.uint8)
    x = tiling.cut_tiles(img, tiling.plan(96, 160, S, 16))[:2].contiguous()
    plain = inference.predict_instances(cal_model, x)
    none = inference.predict_instances(cal_model, x, clean=None)
    got = inference.predict_instances(cal_model, x, clean=dict(min_area=4))
    assert len(plain) == len(none) == len(got) == 2
    print("instances", [None if p is None else len(p) for p in plain])
    for p, q, g in zip(plain, none, got):
        assert (p is None) == (q is None) == (g is None)
        if p is None:
            continue
        after = cc.clean_instances(p, min_area=4)
        assert same_instances(p, q) and same_instances(g, after) and after.masks is p.masks and torch.equal(g.masks.words, p.masks.words)
        want_map, want_table = cc.clean_host(p.labels.cpu().numpy(), len(p), min_area=4, table=p.table)
        assert np.array_equal(g.labels.cpu().numpy(), want_map) and np.array_equal(g.table, want_table)
