"""CPU: the host statements of the label-map clean-up (components.components_host / component_stats_host / clean_host) on hand-made maps,
against scipy.ndimage.label where scipy is installed, and the argument checks of the three C entry points, which all happen on the host
before any HIP call.  Every comparison is exact integer equality."""
import ctypes

import numpy as np
import pytest

from kg_instance_segmentation_amd import components as cc
from kg_instance_segmentation_amd import instances
from kg_instance_segmentation_amd._lib import KGLibraryError


def A(rows):
    return np.array(rows, np.int32)


# ---- components_host on hand-made maps ----------------------------------------------------------------------------------------------------

def test_two_blobs_of_one_id_are_two_components():
    lab = A([[1, 1, 0, 0, 1],
             [1, 0, 0, 1, 1],
             [0, 0, 0, 0, 0]])
    comp, m = cc.components_host(lab)
    assert m == 2 and comp.dtype == np.int32
    assert np.array_equal(comp, A([[1, 1, 0, 0, 2],
                                   [1, 0, 0, 2, 2],
                                   [0, 0, 0, 0, 0]]))


def test_two_ids_that_touch_are_never_joined():
    lab = A([[1, 1, 2, 2],
             [1, 2, 2, 0]])
    for conn in (4, 8):
        comp, m = cc.components_host(lab, conn)
        assert m == 2 and np.array_equal(comp, A([[1, 1, 2, 2], [1, 2, 2, 0]]))


def test_a_diagonal_pair_is_one_component_under_8_and_two_under_4():
    lab = A([[0, 3, 0],
             [3, 0, 0],
             [0, 0, 3]])
    c8, m8 = cc.components_host(lab, 8)
    c4, m4 = cc.components_host(lab, 4)
    assert m8 == 2 and np.array_equal(c8, A([[0, 1, 0], [1, 0, 0], [0, 0, 2]]))
    assert m4 == 3 and np.array_equal(c4, A([[0, 1, 0], [2, 0, 0], [0, 0, 3]]))


def test_background_components_are_numbered_together_with_ids():
    lab = A([[0, 5, 0, 0],
             [5, 5, 5, 0],
             [5, 0, 5, 0],
             [5, 5, 5, 0]])
    comp, m = cc.components_host(lab, 8, 4)
    assert m == 4
    assert np.array_equal(comp, A([[1, 2, 3, 3],
                                   [2, 2, 2, 3],
                                   [2, 4, 2, 3],
                                   [2, 2, 2, 3]]))
    # with 8 for the background the corner pixel joins nothing new here, but the two zero regions at the top still do not touch
    assert cc.components_host(lab, 4, 8)[1] == 4
    st = cc.component_stats_host(lab, comp, m)
    assert st.dtype == np.int64 and st.shape == (4, 9)
    assert st[3].tolist() == [0, 1, 2, 1, 3, 2, 0, 2, 2]                       # the hole: not on the border, enclosed by component 2 alone
    assert st[1].tolist() == [5, 9, 0, 0, 4, 3, 1, 1, 4]
    assert st[0].tolist() == [0, 1, 0, 0, 1, 1, 1, 2, 2]


def test_stack_of_images_and_bad_arguments():
    lab = np.stack([A([[1, 1], [0, 1]]), A([[1, 0], [0, 1]])])
    comp, m = cc.components_host(lab, 4)
    assert m.tolist() == [1, 2] and np.array_equal(comp[1], A([[1, 0], [0, 2]]))
    assert len(cc.component_stats_host(lab, comp, m)) == 3
    for bad in ((5, 0), (8, 3)):
        with pytest.raises(KGLibraryError):
            cc.components_host(lab, *bad)
    big = A([[-2 ** 31, -1], [2 ** 31 - 1, -1]])
    assert np.array_equal(cc.components_host(big, 4)[0], A([[1, 2], [3, 2]]))


def blocky(H, W, n, seed):
    rng = np.random.default_rng(1000 * H + 10 * W + 7 * n + seed)
    lab = np.zeros((H, W), np.int32)
    for i in range(1, n + 1):
        y, x = rng.integers(0, H), rng.integers(0, W)
        lab[y:y + rng.integers(1, H // 3 + 2), x:x + rng.integers(1, W // 2 + 2)] = i
    holes = rng.random((H, W)) < 0.08
    lab[holes] = 0
    return lab


def by_first_pixel(part):
    """A partition given as an integer map (0 = outside) renumbered 1 .. m in raster order of each part's first pixel."""
    flat = part.reshape(-1)
    ids, first = np.unique(flat, return_index=True)
    ids, first = ids[ids != 0], first[ids != 0]
    lut = {int(i): k + 1 for k, i in enumerate(ids[np.argsort(first)])}
    return np.array([lut.get(int(v), 0) for v in flat], np.int64).reshape(part.shape)


def test_cross_check_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    structure = {4: ndi.generate_binary_structure(2, 1), 8: ndi.generate_binary_structure(2, 2)}
    for H, W, n, seed in ((23, 31, 6, 0), (40, 67, 12, 1), (64, 64, 30, 2)):
        lab = blocky(H, W, n, seed)
        for conn in (4, 8):
            for bg in (0, 4, 8):
                comp, m = cc.components_host(lab, conn, bg)
                assert comp.max(initial=0) == m
                want = np.zeros((H, W), np.int64)
                nxt = 0
                for v in np.unique(lab):
                    c = conn if v else bg
                    if c == 0:
                        continue
                    part, k = ndi.label(lab == v, structure[c])
                    want[part > 0] = part[part > 0] + nxt
                    nxt += k
                assert m == nxt and np.array_equal(comp, by_first_pixel(want)), (H, W, conn, bg)


# ---- clean_host ---------------------------------------------------------------------------------------------------------------------------

RING = A([[0, 0, 0, 0, 0],
          [0, 1, 1, 1, 0],
          [0, 1, 0, 1, 0],
          [0, 1, 1, 1, 0],
          [0, 0, 0, 0, 0]])


def test_a_ring_is_filled():
    out, tab = cc.clean_host(RING, 1)
    want = RING.copy()
    want[2, 2] = 1
    assert out.dtype == np.int32 and np.array_equal(out, want)
    assert tab.dtype == np.int64 and tab.tolist() == [[0, 9, 1, 1, 4, 4, 18, 18]]
    assert np.array_equal(cc.clean_host(RING, 1, fill_holes=False)[0], RING)


def test_a_ring_around_another_ids_pixel_keeps_the_pixel():
    lab = RING.copy()
    lab[2, 2] = 2
    out, tab = cc.clean_host(lab, 2)
    assert np.array_equal(out, lab) and tab[1].tolist() == [0, 1, 2, 2, 3, 3, 2, 2]


def test_a_hole_that_touches_the_border_is_not_filled():
    lab = A([[1, 0, 1],
             [1, 0, 1],
             [1, 1, 1]])
    assert np.array_equal(cc.clean_host(lab, 1)[0], lab)


def test_a_hole_enclosed_by_two_ids_is_not_filled():
    lab = A([[1, 1, 2, 2],
             [1, 0, 0, 2],
             [1, 1, 2, 2]])
    assert np.array_equal(cc.clean_host(lab, 2)[0], lab)


def test_max_hole_area_is_honoured():
    lab = np.ones((6, 7), np.int32)
    lab[1, 1] = 0
    lab[3:5, 3:5] = 0
    out = cc.clean_host(lab, 1, max_hole_area=1)[0]
    want = lab.copy()
    want[1, 1] = 1
    assert np.array_equal(out, want)
    assert np.array_equal(cc.clean_host(lab, 1, max_hole_area=4)[0], np.ones((6, 7), np.int32))
    assert np.array_equal(cc.clean_host(lab, 1, max_hole_area=0)[0], lab)


def test_keep_largest_with_an_area_tie_keeps_the_first_component():
    lab = A([[0, 0, 0, 2, 2],
             [1, 1, 0, 0, 0],
             [0, 0, 0, 1, 1],
             [2, 0, 0, 0, 0]])
    out, tab = cc.clean_host(lab, 2)
    assert np.array_equal(out, A([[0, 0, 0, 2, 2],
                                  [1, 1, 0, 0, 0],
                                  [0, 0, 0, 0, 0],
                                  [0, 0, 0, 0, 0]]))
    assert np.array_equal(cc.clean_host(lab, 2, keep="all")[0], lab)
    assert tab[:, 1].tolist() == [2, 2]


def test_min_area_removes_a_whole_id_and_its_row_is_zeros():
    lab = A([[1, 1, 1, 0, 2],
             [1, 1, 1, 0, 2],
             [0, 0, 0, 0, 0]])
    old = np.arange(16, dtype=np.int64).reshape(2, 8) + 100
    out, tab = cc.clean_host(lab, 2, min_area=3, table=old)
    assert np.array_equal(out, np.where(lab == 1, 1, 0))
    assert tab[1].tolist() == [0] * 8 and tab[0].tolist() == [100, 6, 0, 0, 2, 3, 3, 6]       # area_full carried over for the survivor


def test_a_fragment_inside_another_id_is_dropped_but_filled_only_by_a_second_call():
    lab = np.full((7, 7), 1, np.int32)
    lab[3, 3] = 2                                   # a fragment of 2 inside 1
    lab[0, 5:] = 2                                  # the larger piece of 2
    once, _ = cc.clean_host(lab, 2)
    want = lab.copy()
    want[3, 3] = 0
    assert np.array_equal(once, want)               # decided on the components of the INPUT map: the new hole stays
    twice, _ = cc.clean_host(once, 2)
    want[3, 3] = 1
    assert np.array_equal(twice, want)


def test_relabel_returns_old_ids():
    lab = A([[0, 4, 4, 0, 2],
             [0, 4, 4, 0, 0],
             [7, 0, 0, 0, 0]])
    old = np.zeros((7, 8), np.int64)
    old[:, 0] = np.arange(1, 8) * 10
    out, tab, old_ids = cc.clean_host(lab, 7, min_area=2, relabel=True, table=old)
    assert old_ids.dtype == np.int32 and old_ids.tolist() == [4]
    assert np.array_equal(out, np.where(lab == 4, 1, 0)) and tab.tolist() == [[40, 4, 0, 1, 2, 3, 2, 6]]
    out, tab, old_ids = cc.clean_host(lab, 7, relabel=True)
    assert old_ids.tolist() == [2, 4, 7] and np.array_equal(out, np.select([lab == 2, lab == 4, lab == 7], [1, 2, 3], 0))
    assert tab.shape == (3, 8)


def test_table_equals_table_host_of_the_cleaned_maps_dense_masks():
    n = 9
    lab = blocky(40, 67, n, 3)
    for policy in (dict(), dict(keep="all", min_area=5), dict(connectivity=4, fill_holes=False), dict(max_hole_area=2, min_area=3)):
        out, tab = cc.clean_host(lab, n, **policy)
        dense = np.stack([out == i for i in range(1, n + 1)])
        assert np.array_equal(tab[:, 1:], instances.table_host(dense)[:, 1:]), policy
        assert not tab[:, 0].any()
    assert (cc.clean_host(lab, n)[0] != lab).any()


def test_a_value_outside_the_ids_raises_naming_the_pixel_count():
    lab = A([[1, 3, 3], [0, -1, 1]])
    with pytest.raises(KGLibraryError, match=r"3 pixel\(s\) of the label map lie outside \[0, 2\]"):
        cc.clean_host(lab, 2)
    with pytest.raises(KGLibraryError):
        cc.clean_host(lab, 3, keep="biggest")
    with pytest.raises(KGLibraryError, match="relabel"):
        cc.clean_instances(instances.Instances(lab, np.zeros((3, 5), np.float32), np.zeros((3, 8), np.int64), None), relabel=True)


def test_clean_instances_on_a_host_map_keeps_everything_but_labels_and_table():
    dets = np.zeros((1, 5), np.float32)
    old = np.array([[77, 8, 1, 1, 4, 4, 16, 16]], np.int64)
    inst = instances.Instances(RING, dets, old, "masks")
    got = cc.clean_instances(inst, min_area=2)
    assert type(got) is instances.Instances and got.dets is dets and got.masks == "masks"
    assert got.labels[2, 2] == 1 and got.table.tolist() == [[77, 9, 1, 1, 4, 4, 18, 18]]
    assert inst.labels is RING and inst.table is old


# ---- the C entry points check their arguments on the host -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from kg_instance_segmentation_amd import _lib, build
    build.build()
    return _lib.load()


def test_entries_are_declared_bound_and_exported(lib):
    import os
    from kg_instance_segmentation_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kgnet_hip.h")).read()
    for name in ("kg_label_components_workspace_bytes", "kg_label_components", "kg_component_stats", "kg_component_remap"):
        assert name + "(" in hdr and name in _lib._SIGS and hasattr(lib, name)
    assert "components.hip" in __import__("kg_instance_segmentation_amd.build", fromlist=["SOURCES"]).SOURCES


def test_workspace_helper(lib):
    ws = lib.kg_label_components_workspace_bytes
    assert ws(1, 64, 64) == 4 * (4096 + 1) and ws(3, 37, 70) == 4 * 3 * (37 * 70 + 1) and ws(1, 65, 64) == 4 * (65 * 64 + 2)
    assert ws(0, 4, 4) == -1 and ws(1, 0, 4) == -1 and ws(1, 4, -1) == -1 and ws(2, 32768, 32768) == -1 and ws(1, 65536, 32768) == -1


def test_entries_refuse_bad_arguments_before_any_launch(lib):
    buf = (ctypes.c_int * 4096)()                   # host memory: no entry may get as far as a launch
    p = ctypes.addressof(buf)
    odd = ctypes.c_void_p(p + 1)
    P = ctypes.c_void_p(p)
    H = W = 8
    need = lib.kg_label_components_workspace_bytes(1, H, W)
    start = (ctypes.c_int * 2)(0, 3)

    def err(rc, name, text):
        msg = lib.kg_last_error().decode()
        assert rc != 0 and name in msg and text in msg, (rc, msg)

    def lc(labels=P, nimg=1, h=H, w=W, conn=8, bg=0, comp=ctypes.c_void_p(p + 1024), ncomp=P, work=P, nbytes=need):
        return lib.kg_label_components(labels, nimg, h, w, conn, bg, comp, ncomp, work, ctypes.c_long(nbytes), None)

    err(lc(labels=None), "kg_label_components", "null pointer")
    err(lc(comp=None), "kg_label_components", "null pointer")
    err(lc(ncomp=None), "kg_label_components", "null pointer")
    err(lc(work=None), "kg_label_components", "null pointer")
    err(lc(conn=5), "kg_label_components", "connectivity 5")
    err(lc(bg=3), "kg_label_components", "bg_connectivity 3")
    err(lc(nimg=2, h=32768, w=32768), "kg_label_components", "exceeds 2^31 - 1")
    err(lc(h=0), "kg_label_components", "bad size")
    err(lc(nbytes=need - 1), "kg_label_components", "workspace")
    err(lc(labels=odd), "kg_label_components", "misaligned")
    err(lc(work=odd), "kg_label_components", "misaligned")

    def cs(labels=P, comp=P, nimg=1, h=H, w=W, st=start, total=3, stats=P):
        return lib.kg_component_stats(labels, comp, nimg, h, w, st, total, stats, None)

    err(cs(labels=None), "kg_component_stats", "null pointer")
    err(cs(stats=None), "kg_component_stats", "null pointer")
    err(cs(st=None), "kg_component_stats", "null pointer")
    err(cs(nimg=2, h=32768, w=32768), "kg_component_stats", "exceeds 2^31 - 1")
    err(cs(comp=odd), "kg_component_stats", "misaligned")
    err(cs(st=(ctypes.c_int * 2)(1, 3)), "kg_component_stats", "comp_start[0]")
    err(cs(st=(ctypes.c_int * 3)(0, 3, 2), nimg=2, total=2), "kg_component_stats", "decreases")
    err(cs(total=4), "kg_component_stats", "comp_start[nimg]")

    def rm(comp=P, nimg=1, h=H, w=W, st=start, total=3, newval=P, out=ctypes.c_void_p(p + 1024)):
        return lib.kg_component_remap(comp, nimg, h, w, st, total, newval, out, None)

    err(rm(comp=None), "kg_component_remap", "null pointer")
    err(rm(newval=None), "kg_component_remap", "null pointer")
    err(rm(out=None), "kg_component_remap", "null pointer")
    err(rm(nimg=2, h=32768, w=32768), "kg_component_remap", "exceeds 2^31 - 1")
    err(rm(out=odd), "kg_component_remap", "misaligned")
    err(rm(st=(ctypes.c_int * 2)(2, 3)), "kg_component_remap", "comp_start[0]")
    err(rm(st=(ctypes.c_int * 3)(0, 3, 1), nimg=2, total=1), "kg_component_remap", "decreases")
    err(rm(out=P), "kg_component_remap", "aliases")
