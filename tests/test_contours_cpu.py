"""CPU: the host statement of the contour semantics (contours.contours_host, include/kgnet_hip.h) against written-out expectations and
against independent checks: the shoelace areas of the rings add up to the area, the cracks to measure's `edges`, the ring counts to the
component counts, and an even-odd rasterisation of the rings gives the mask back.  Every comparison is exact integer equality."""
import ctypes
import os

import numpy as np
import pytest

from kg_instance_segmentation_amd import _lib
from kg_instance_segmentation_amd import components as cc
from kg_instance_segmentation_amd import contours as ct
from kg_instance_segmentation_amd import measure as ms

E = _lib.KGLibraryError
I32 = np.iinfo(np.int32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mask_map(rows):
    """'#' = id 1, '.' = 0"""
    return np.array([[c == "#" for c in r] for r in rows], bool).astype(np.int32)


def whole(lab, ids=(1,), img=0):
    H, W = lab.shape[-2:]
    return np.array([[img, int(i), 0, 0, H, W] for i in ids], np.int64).reshape(-1, 6)


def rings_of(lab, v=1):
    """(vertex lists as tuples, perimeters, area2s) of id v over the whole map"""
    c = ct.contours_host(lab, whole(lab, [v]))
    return [list(map(tuple, r.tolist())) for r in c.of(0)], c.perimeter.tolist(), c.area2.tolist()


def rasterise(c, k, H, W):
    """Even-odd at the pixel centres: a pixel is inside when an odd number of vertical ring sides lie to its right on its row"""
    out = np.zeros((H, W), np.int64)
    for ring in c.of(k):
        r = ring.astype(np.int64)
        for (ya, xa), (yb, xb) in zip(r.tolist(), np.roll(r, -1, 0).tolist()):
            if xa == xb:
                out[min(ya, yb):max(ya, yb), :xa] += 1                # the pixels (y, x) with x + 0.5 < xa
    return (out & 1).astype(bool)


# ---- written-out expectations -----------------------------------------------------------------------------------------------------------

def test_one_pixel():
    v, p, a = rings_of(np.ones((1, 1), np.int32))
    assert v == [[(0, 0), (0, 1), (1, 1), (1, 0)]] and p == [4] and a == [2]
    lab = np.zeros((5, 7), np.int32)
    lab[3, 4] = 1
    assert rings_of(lab)[0] == [[(3, 4), (3, 5), (4, 5), (4, 4)]]


def test_two_pixels_meeting_at_a_corner_get_two_rings():
    v, p, a = rings_of(mask_map(["#.", ".#"]))
    assert v == [[(0, 0), (0, 1), (1, 1), (1, 0)], [(1, 1), (1, 2), (2, 2), (2, 1)]] and p == [4, 4] and a == [2, 2]
    v, p, a = rings_of(mask_map([".#", "#."]))                         # the other diagonal: starts (0, 1) and (1, 0)
    assert v == [[(0, 1), (0, 2), (1, 2), (1, 1)], [(1, 0), (1, 1), (2, 1), (2, 0)]] and a == [2, 2]


def test_ring_of_three_by_three_has_one_hole():
    v, p, a = rings_of(mask_map(["###", "#.#", "###"]))
    assert v[0] == [(0, 0), (0, 3), (3, 3), (3, 0)] and p == [12, 4] and a == [18, -2]
    assert v[1] == [(2, 1), (2, 2), (1, 2), (1, 1)]                   # the hole starts at the top edge of pixel (2, 1) and runs anticlockwise


def test_l_shape():
    v, p, a = rings_of(mask_map(["#.", "#.", "##"]))
    assert v == [[(0, 0), (0, 1), (2, 1), (2, 2), (3, 2), (3, 0)]] and p == [10] and a == [8]


NESTED = mask_map(["#####", "#...#", "#.#.#", "#...#", "#####"])


def test_island_in_a_hole_in_a_ring():
    """Ring, hole, island have the area2 signs +, -, +.  In ring order the island comes second: its start (2, 2) precedes the hole's
    (4, 1), the top edge of the ring's pixel below the hole, in raster order."""
    v, p, a = rings_of(NESTED)
    assert a == [50, 2, -18] and p == [20, 4, 12]
    assert v == [[(0, 0), (0, 5), (5, 5), (5, 0)], [(2, 2), (2, 3), (3, 3), (3, 2)], [(4, 1), (4, 4), (1, 4), (1, 1)]]


def test_pinch_vertex_is_visited_twice_by_a_hole():
    """A hole made of two background pixels that meet at a corner is ONE ring (the background is 8-connected) through that corner twice"""
    lab = mask_map(["####", "#.##", "##.#", "####"])
    c = ct.contours_host(lab, whole(lab))
    assert c.area2.tolist() == [32, -4] and c.perimeter.tolist() == [16, 8] and c.count.tolist() == [4, 8]
    hole = list(map(tuple, c.of(0)[1].tolist()))
    assert hole.count((2, 2)) == 2 and len(set(hole)) == 7


# ---- invariants on seeded random masks ---------------------------------------------------------------------------------------------------

def component_counts(me):
    """(4-connected components of the mask, 8-connected components of the padded complement minus one) by components_host"""
    pad = np.zeros((me.shape[0] + 2, me.shape[1] + 2), np.int32)
    pad[1:-1, 1:-1] = me
    comp, _ = cc.components_host(pad, connectivity=4, bg_connectivity=8)
    return len(np.unique(comp[pad == 1])), len(np.unique(comp[pad == 0])) - 1


def check_invariants(lab, v, c, k=0, box=None):
    H, W = lab.shape
    y1, x1, y2, x2 = box if box is not None else (0, 0, H, W)
    me = np.zeros((H, W), bool)
    me[y1:y2, x1:x2] = lab[y1:y2, x1:x2] == v
    a, b = int(c.ring_ptr[k]), int(c.ring_ptr[k + 1])
    assert int(c.area2[a:b].sum()) == 2 * int(me.sum()) == 2 * int(c.areas()[k])
    sides = sum(int((me & ~np.roll(np.pad(me, 1), s, ax)[1:-1, 1:-1]).sum()) for s in (1, -1) for ax in (0, 1))
    assert int(c.perimeters()[k]) == sides
    assert (c.count[a:b] >= 4).all() and (c.count[a:b] % 2 == 0).all() and (c.area2[a:b] != 0).all()
    starts = [tuple(r[0].tolist()) for r in c.of(k)]
    assert starts == sorted(starts) and len(set(starts)) == len(starts)
    assert np.array_equal(rasterise(c, k, H, W), me)
    outer, holes = component_counts(me)
    assert int((c.area2[a:b] > 0).sum()) == outer and int(c.is_hole()[a:b].sum()) == holes
    for r in c.of(k):                                                 # consecutive vertices differ in exactly one coordinate, alternately
        d = np.roll(r, -1, 0).astype(np.int64) - r
        assert ((d != 0).sum(1) == 1).all() and ((d[:, 0] != 0) != np.roll(d[:, 0] != 0, 1)).all()
    assert [int(np.abs(np.roll(r, -1, 0).astype(np.int64) - r).sum()) for r in c.of(k)] == c.perimeter[a:b].tolist()


@pytest.mark.parametrize("seed", range(12))
def test_invariants_on_random_masks(seed):
    rng = np.random.default_rng(seed)
    for _ in range(12):
        H, W = rng.integers(1, 14, 2)
        lab = (rng.random((H, W)) < rng.choice([0.3, 0.5, 0.7, 0.9])).astype(np.int32)
        c = ct.contours_host(lab, whole(lab))
        check_invariants(lab, 1, c)
        edges = ms.measure_host(np.pad(lab, 1), [[0, 1, 0, 0, H + 2, W + 2]])[0, ms.GEOMETRY_COLUMNS.index("edges")]
        assert int(c.perimeters()[0]) == int(edges)


def test_perimeter_is_measures_edges_on_a_label_map():
    rng = np.random.default_rng(3)
    lab = rng.integers(0, 5, (31, 45)).repeat(2, 0).repeat(3, 1).astype(np.int32)
    c = ct.contours_host(lab, 4)                                      # the ids 1 .. 4 inside their own boxes
    rows = ms.measure_host(lab, 4)
    assert np.array_equal(c.perimeters(), rows[:, ms.GEOMETRY_COLUMNS.index("edges")]) and np.array_equal(c.areas(), rows[:, 0])
    for k in range(4):
        check_invariants(lab, k + 1, c, k)


def test_ring_counts_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(11)
    for _ in range(40):
        H, W = rng.integers(1, 14, 2)
        me = rng.random((H, W)) < rng.choice([0.3, 0.6, 0.9])
        c = ct.contours_host(me.astype(np.int32), whole(me))
        outer = ndi.label(me)[1]
        holes = ndi.label(~np.pad(me, 1), structure=np.ones((3, 3)))[1] - 1
        assert int((c.area2 > 0).sum()) == outer and int(c.is_hole().sum()) == holes


# ---- edge cases --------------------------------------------------------------------------------------------------------------------------

def test_a_p_cut_by_its_box_is_closed_at_the_box():
    lab = np.ones((6, 8), np.int32)
    c = ct.contours_host(lab, [[0, 1, 1, 2, 4, 7], [0, 1, -5, -5, 3, 3], [0, 1, 4, 6, 99, 99]])
    assert [list(map(tuple, r[0].tolist())) for r in (c.of(0), c.of(1), c.of(2))] == \
        [[(1, 2), (1, 7), (4, 7), (4, 2)], [(0, 0), (0, 3), (3, 3), (3, 0)], [(4, 6), (4, 8), (6, 8), (6, 6)]]
    rng = np.random.default_rng(5)
    lab = (rng.random((12, 13)) < 0.7).astype(np.int32)
    box = (2, 3, 9, 11)
    check_invariants(lab, 1, ct.contours_host(lab, [[0, 1, *box]]), 0, box)


def test_extreme_ids_are_ordinary():
    ids = [0, -1, I32.min, I32.max]
    rng = np.random.default_rng(4)
    lab = np.array(ids + [7], np.int32)[rng.integers(0, 5, (11, 13))]
    c = ct.contours_host(lab, whole(lab, ids + [8]))
    assert (c.counts()[:4] > 0).all() and c.counts()[4] == 0
    for k, v in enumerate(ids):
        check_invariants(lab, v, c, k)


def test_bad_jobs_get_zero_rings():
    lab = np.ones((4, 5), np.int32)
    jobs = [[0, 1, 0, 0, 4, 5], [-1, 1, 0, 0, 4, 5], [1, 1, 0, 0, 4, 5], [0, 1, 3, 3, 3, 5], [0, 1, 3, 4, 1, 2], [0, 9, 0, 0, 4, 5], [0, 1, 4, 5, 9, 9],
            [0, 1, 2, 2, 4, 5]]
    c = ct.contours_host(lab, jobs)
    assert len(c) == 8 and c.counts().tolist() == [1, 0, 0, 0, 0, 0, 0, 1] and c.areas().tolist() == [20, 0, 0, 0, 0, 0, 0, 6]
    assert len(ct.contours_host(lab, np.zeros((0, 6), np.int64))) == 0 and len(ct.contours_host(0 * lab, 0)) == 0
    for bad in ([[0, 1, 0, 0, 4]], [[0, 1, 0, 0, 4, 2 ** 31]], [[0.5, 1, 0, 0, 4, 5]]):
        with pytest.raises(E):
            ct.contours_host(lab, bad)
    with pytest.raises(E):
        ct.contours_host(lab.astype(np.float32), jobs)
    with pytest.raises(E):
        ct.contours_host(np.zeros((0, 4), np.int32), jobs)


def test_a_stack_of_three_maps():
    rng = np.random.default_rng(6)
    lab = rng.integers(0, 4, (3, 9, 10)).astype(np.int32)
    lab[1] = 0
    c = ct.contours_host(lab, [3, 0, 3])
    assert len(c) == 6
    for i, sl in ((0, (0, 3)), (2, (3, 6))):
        assert c.slice(*sl) == ct.contours_host(lab[i], 3)
    jobs = np.concatenate([whole(lab, [1, 2, 3], i) for i in (2, 0, 1)])
    got = ct.contours_host(lab, jobs)
    assert got.slice(0, 3) == ct.contours_host(lab[2], whole(lab, [1, 2, 3])) and got.counts()[6:].sum() == 0
    assert got.slice(0, len(got)) == got and got != c and got.slice(2, 2).counts().tolist() == []


def test_coco_and_geojson_on_the_nested_case():
    c = ct.contours_host(NESTED, whole(NESTED, [1, 5]))
    assert c.coco(0) == [[0, 0, 5, 0, 5, 5, 0, 5], [2, 2, 3, 2, 3, 3, 2, 3]] and c.coco(1) == []        # [x, y] pairs; the hole is dropped
    g = c.geojson(0)
    assert g["type"] == "MultiPolygon" and len(g["coordinates"]) == 2
    big, island = g["coordinates"]
    assert big[0] == [[0, 0], [5, 0], [5, 5], [0, 5], [0, 0]] and len(big) == 2 and island == [[[2, 2], [3, 2], [3, 3], [2, 3], [2, 2]]]
    assert big[1][0] == big[1][-1] and sorted(map(tuple, big[1][:-1])) == [(1, 1), (1, 4), (4, 1), (4, 4)]
    assert c.geojson(1) == {"type": "MultiPolygon", "coordinates": []}
    one = ct.contours_host(mask_map(["###", "#.#", "###"]), 1).geojson(0)
    assert one["type"] == "Polygon" and len(one["coordinates"]) == 2
    # two separate rings, each with its own hole: every hole goes to the ring around it
    lab = np.zeros((3, 7), np.int32)
    lab[:, :3] = lab[:, 4:] = 1
    lab[1, 1] = lab[1, 5] = 0
    g = ct.contours_host(lab, 1).geojson(0)
    assert [len(p) for p in g["coordinates"]] == [2, 2] and g["coordinates"][1][1][0] == [5, 2]


def test_contours_object():
    c = ct.contours_host(NESTED, whole(NESTED, [1, 5, 0]))
    assert len(c) == 3 and c.counts().tolist() == [3, 0, 2] and c.rows().tolist() == [0, 0, 0, 2, 2] and c.verts.dtype == np.int32
    assert c.first.tolist() == [0, 4, 8, 12, 16] and c.is_hole().tolist() == [False, False, True, False, True]
    assert c.areas().tolist() == [17, 0, 8] and c.perimeters().tolist() == [36, 0, 16]
    s = c.slice(2, 3)
    assert s.first.tolist() == [0, 4] and np.array_equal(s.verts, c.verts[12:]) and s.ring_ptr.tolist() == [0, 2]
    assert c == ct.Contours(c.ring_ptr, c.first, c.count, c.perimeter, c.area2, c.verts) and c != s and c != 3
    for bad in (([0, 2], [0], [4], [4], [2], np.zeros((4, 2))), ([0, 1], [1], [4], [4], [2], np.zeros((4, 2))), ([0, 1], [0], [4], [4], [2], np.zeros((3, 2)))):
        with pytest.raises(E):
            ct.Contours(*bad)


def test_fits_at_its_boundary():
    assert ct.fits(8190, 30) and not ct.fits(8191, 30) and ct.fits(8190, 1) and not ct.fits(8190, 31)
    assert ct.fits(1, 1) and not ct.fits(0, 5) and not ct.fits(5, 0)
    assert ct.fits(250, 250) and ct.fits(510, 478) and not ct.fits(511, 479) and ct.fits(510, 510) == ((512 * 32 * 17) <= 2 ** 18)
    for h, w in ((8190, 30), (8191, 30), (100, 94), (100, 95), (2729, 94), (2730, 94), (2, 32766), (1, 32768)):
        assert ct.fits(h, w) == ((h + 2) * 32 * (-(-(w + 2) // 32) | 1) <= 2 ** 18)


# ---- the C entries ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from kg_instance_segmentation_amd import build
    build.build()
    return _lib.load()


def test_entries_are_declared_bound_and_exported(lib):
    import inspect
    import re
    from kg_instance_segmentation_amd import build, inference, instances, tiling
    header = open(os.path.join(ROOT, "include", "kgnet_hip.h")).read()
    for name, nargs in (("kg_label_contour_counts", 8), ("kg_label_contours", 11)):
        assert name in _lib._SIGS and name in _lib.SYMBOLS and hasattr(lib, name) and len(_lib._SIGS[name]) == nargs
        assert re.search(r"\bint " + name + r"\(", header), name
    assert "contours.hip" in build.SOURCES and build.SOURCES["contours.hip"] == [] and "contours.hip" not in build.ROWS_SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "contours.hip"))
    for fn in (inference.predict_instances, tiling.predict_tiled):
        assert inspect.signature(fn).parameters["contours"].default is None
    a = instances.Instances(None, np.zeros((0, 5), np.float32), None, None)
    b = tiling.TiledInstances(None, np.zeros((0, 5), np.float32), None, None, None, None)
    assert a.contours is None and b.contours is None and a.runs is None and not hasattr(a, "__dict__")


def test_entries_refuse_bad_arguments_before_any_launch(lib):
    buf = (ctypes.c_longlong * 4096)()                      # host memory: the entries may never get as far as a launch
    p = ctypes.addressof(buf)
    P, JOBS, OUT, VERTS = (ctypes.c_void_p(p + k * 4096) for k in range(4))

    def counts(labels=P, nimg=1, H=8, W=8, jobs=JOBS, m=3, out=OUT):
        return lib.kg_label_contour_counts(labels, nimg, H, W, jobs, m, out, None)

    def rows(labels=P, nimg=1, H=8, W=8, jobs=JOBS, m=3, rings=OUT, R=4, verts=VERTS, V=16):
        return lib.kg_label_contours(labels, nimg, H, W, jobs, m, rings, R, verts, V, None)

    def err(rc, name, text):
        msg = lib.kg_last_error().decode()
        assert rc != 0 and name in msg and text in msg, (rc, msg)

    for call, name in ((counts, "kg_label_contour_counts"), (rows, "kg_label_contours")):
        err(call(labels=None), name, "null pointer")
        err(call(jobs=None), name, "null pointer")
        err(call(H=32769), name, "32768")
        err(call(W=32769), name, "32768")
        err(call(nimg=0), name, "bad size")
        err(call(H=0), name, "bad size")
        err(call(W=-1), name, "bad size")
        err(call(m=-1), name, "bad size")
        err(call(nimg=3, H=32768, W=32768), name, "exceeds 2^31 - 1")
        err(call(labels=ctypes.c_void_p(p + 2)), name, "misaligned")
        err(call(jobs=ctypes.c_void_p(p + 4096 + 1)), name, "misaligned")
        assert call(m=0) == 0 and call(m=0, jobs=None) == 0
    err(counts(out=None), "kg_label_contour_counts", "null pointer")
    err(counts(out=ctypes.c_void_p(p + 2 * 4096 + 4)), "kg_label_contour_counts", "misaligned")
    err(counts(out=P), "kg_label_contour_counts", "aliases")
    assert counts(m=0, jobs=None, out=None) == 0
    err(rows(rings=None), "kg_label_contours", "null pointer")
    err(rows(verts=None), "kg_label_contours", "null pointer")
    err(rows(R=-1), "kg_label_contours", "R -1")
    err(rows(V=-1), "kg_label_contours", "V -1")
    err(rows(rings=ctypes.c_void_p(p + 2 * 4096 + 4)), "kg_label_contours", "misaligned")
    err(rows(verts=ctypes.c_void_p(p + 3 * 4096 + 2)), "kg_label_contours", "misaligned")
    err(rows(rings=P), "kg_label_contours", "aliases")
    err(rows(verts=P), "kg_label_contours", "aliases")
    err(rows(verts=OUT), "kg_label_contours", "aliases")
    assert rows(R=0, V=0, rings=None, verts=None) == 0 and rows(m=0, jobs=None, rings=None, verts=None, R=0, V=0) == 0


def test_device_routes_refuse_host_maps():
    lab = np.ones((4, 4), np.int32)
    for fn in (lambda: ct.contours(lab, 1), lambda: ct.contour_counts(lab, [[0, 1, 0, 0, 4, 4]]), lambda: ct.contour_rows(lab, [[0, 1, 0, 0, 4, 4, 0, 0]], 1, 4)):
        with pytest.raises(E):
            fn()
