"""CPU: the host statements of sampleprep's label-map route (label_masks_host, warp_labels_host: the yardsticks of the GPU tests) against
the restatement of the mask route (tests/sampleprep_ref.py) on the population of tests/sampleprep_labels_cases.py; boxes that cut, invert
or lie far away; LabelSource's validation; the two C entries' declaration and every host check of kg_sp_warp_labels, on host memory.
No compute entry point is launched.  There is no tolerance anywhere in this file."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import sampleprep_labels_cases as cases
import sampleprep_ref as ref
from kg_instance_segmentation_amd import _lib, sampleprep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32 = np.iinfo(np.int32)


def test_population_covers_what_it_claims():
    seen, sizes, counts = set(), set(), set()
    for q in range(64):
        img, lab, n, p, (H, W) = cases.sample(q)
        seen.add(p.switches()); sizes.add((lab.shape, (H, W))); counts.add(n)
        area = np.bincount(lab.reshape(-1), minlength=cases.NIDS + 1)[1:]
        assert lab.max() <= cases.NIDS and lab.min() == 0
        assert np.count_nonzero(area) * 2 >= cases.NIDS, q                   # at least half the ids keep pixels
        assert np.count_nonzero(area == 0) >= 1 and area[cases.HIDDEN - 1] == 0, q   # and at least one has none
        if p.expand:
            assert p.canvas[0] > lab.shape[0] and p.canvas[1] > lab.shape[1]
    assert len(seen) == 64 and counts == set(cases.COUNTS)
    assert {s for s, _ in sizes} == set(cases.SIZES) and {o for _, o in sizes} == set(cases.OUTPUTS)
    for bi in range(8):
        images, labs, ns, params, H, W = cases.batch(bi)
        assert len({lab.shape for lab in labs}) == 4 and sorted(set(ns)) == sorted(cases.COUNTS)


def test_label_masks_host_equals_the_mask_route_restatement():
    some = 0
    for q in range(64):
        img, lab, n, p, (H, W) = cases.sample(q)
        for ids in (np.arange(1, cases.NIDS + 1), np.arange(1, n + 1)):
            want = ref.prepare_sample(img, cases.dense(lab, ids), p, H, W, targets=False)["warped"]
            got = sampleprep.label_masks_host(lab, cases.boxes(lab, ids), p, H, W)
            assert got.dtype == np.uint8 and got.shape == (len(ids), H, W) and np.array_equal(got, want), q
            some += int(want.any())
    assert some > 64


def test_warped_map_agrees_with_the_masks():
    for q in range(64):
        img, lab, n, p, (H, W) = cases.sample(q)
        ids = np.arange(0, cases.NIDS + 2)                                       # 0 and an absent id among them
        wm = sampleprep.warp_labels_host([lab], [p], H, W)
        assert wm.dtype == np.int32 and wm.shape == (1, H, W)
        masks = sampleprep.label_masks_host(lab, cases.boxes(lab, ids), p, H, W)
        full = np.array([[v, 0, 0, lab.shape[0], lab.shape[1]] for v in ids])
        inside = ref.warp_masks(np.ones((1,) + lab.shape, np.uint8), p, H, W)[0].astype(bool)
        for k, v in enumerate(ids):
            # id 0 has pixels wherever the window shows background: outside the window every id gives 0, id 0 included
            want = (wm[0] == v) & inside
            assert np.array_equal(masks[k], want), (q, v)
        assert np.array_equal(sampleprep.label_masks_host(lab, full, p, H, W), masks)
        assert not (wm[0][~inside]).any()
    two = sampleprep.warp_labels_host([cases.sample(1)[1], cases.sample(2)[1]], [cases.sample(1)[3], cases.sample(2)[3]], 64, 64)
    assert two.shape == (2, 64, 64) and two[0].any() and two[1].any()


def test_boxes_that_cut_invert_or_lie_far_away():
    lab = np.zeros((40, 56), np.int32)
    lab[10:30, 12:44] = 7
    lab[0, 0] = 7                                                                # a stray pixel of the id outside every box below
    for p, (H, W) in ((sampleprep.identity_params(), (40, 56)), (cases.make_params(np.random.RandomState(3), 40, 56, 0b111000), (64, 64)),
                      (cases.make_params(np.random.RandomState(4), 40, 56, 0b011000), (96, 72))):
        whole = sampleprep.label_masks_host(lab, [[7, 0, 0, 40, 56]], p, H, W)[0]
        cut = np.zeros_like(lab)
        cut[15:22, 20:31] = 7
        jobs = [[7, 15, 20, 22, 31],                                             # smaller than the instance: the instance cut to the box
                [7, 22, 20, 15, 31], [7, 15, 31, 22, 20], [7, 22, 31, 15, 20],   # inverted in y, in x, in both
                [7, I32.min, I32.min, I32.min + 5, I32.min + 5], [7, I32.max - 5, I32.max - 5, I32.max, I32.max],   # far away
                [7, I32.max, I32.max, I32.min, I32.min],                         # far and inverted
                [7, I32.min, I32.min, I32.max, I32.max],                         # far on both sides: the whole map
                [7, -3, -9, 22, 31], [7, 15, 20, 400, 560]]                      # half outside: clamped to the map
        got = sampleprep.label_masks_host(lab, jobs, p, H, W)
        assert np.array_equal(got[0], sampleprep.label_masks_host(cut, [[7, 0, 0, 40, 56]], p, H, W)[0]) and got[0].any()
        assert got[0].sum() < whole.sum() and not (got[0] & ~whole).any()
        assert not got[1:7].any()
        assert np.array_equal(got[7], whole)
        for k, sl in ((8, np.s_[:22, :31]), (9, np.s_[15:, 20:])):
            part = np.zeros_like(lab)
            part[sl] = lab[sl]
            assert np.array_equal(got[k], sampleprep.label_masks_host(part, [[7, 0, 0, 40, 56]], p, H, W)[0]) and got[k].any()
    ident = sampleprep.label_masks_host(lab, jobs[:1], sampleprep.identity_params(), 40, 56)[0]     # the identity map: the cut itself
    assert np.array_equal(ident, cut == 7)


def rows_of(head, box):
    """the two halves job_rows returns, as the rows (img, id, y1, x1, y2, x2)"""
    return np.concatenate([head, box], 1).tolist()


def test_label_source_validation():
    lab = cases.sample(0)[1]
    ok = sampleprep.LabelSource(lab, n=37)
    assert len(ok) == 37 and ok.shape == lab.shape and ok.labels.dtype == np.int32
    assert len(sampleprep.LabelSource(lab.astype(np.int64), jobs=np.zeros((4, 5), np.int64))) == 4
    assert len(sampleprep.LabelSource(torch.from_numpy(lab), n=0)) == 0           # a host tensor is a host array
    st = np.zeros((37, 5), np.int64)
    assert sampleprep.LabelSource(lab, n=37, stats=st).stats is st
    for bad in (lab.astype(np.float32), lab[None], lab[0], np.zeros((0, 5), np.int32), lab.astype(np.int64) + 2 ** 40, "map",
                torch.from_numpy(lab).float(), torch.from_numpy(lab)[None]):
        with pytest.raises(ValueError, match="label map"):
            sampleprep.LabelSource(bad, n=1)
    with pytest.raises(ValueError, match="not both and not neither"):
        sampleprep.LabelSource(lab, n=3, jobs=np.zeros((3, 5), np.int32))
    with pytest.raises(ValueError, match="not both and not neither"):
        sampleprep.LabelSource(lab)
    with pytest.raises(ValueError, match="stats belong to n"):
        sampleprep.LabelSource(lab, jobs=np.zeros((3, 5), np.int32), stats=st[:3])
    for bad in (st[:36], st[:, :4], st.astype(np.float64), np.zeros((38, 5), np.int32), st + 2 ** 31, st - 2 ** 31 - 1, torch.zeros(36, 5, dtype=torch.int32),
                torch.zeros(37, 5, dtype=torch.int64)):
        with pytest.raises(ValueError, match="stats"):
            sampleprep.LabelSource(lab, n=37, stats=bad)
    for bad in (np.zeros((3, 6), np.int32), np.zeros((3, 5), np.float32), np.zeros(5, np.int32), np.full((1, 5), 2 ** 31)):
        with pytest.raises(ValueError, match="jobs"):
            sampleprep.LabelSource(lab, jobs=bad)
    for bad in (-1, 1.5, True, 2 ** 31):
        with pytest.raises(ValueError, match="instance count"):
            sampleprep.LabelSource(lab, n=bad)
    # the rows a source contributes as image 3 of a batch, from the three host forms
    stats = np.array([[6, 1, 2, 3, 5], [0, 9, 9, 9, 9], [1, 4, 4, 5, 5]])
    head, box, dev_box = sampleprep.LabelSource(lab, n=3, stats=stats).job_rows(3, None)
    assert dev_box is None and head.dtype == box.dtype == np.int32
    assert rows_of(head, box) == [[3, 1, 1, 2, 3, 5], [3, 2, 0, 0, 0, 0], [3, 3, 4, 4, 5, 5]]
    head, box, _ = sampleprep.LabelSource(lab, jobs=[[9, 1, 2, 3, 4], [-4, 0, 0, 1, 1]]).job_rows(2, None)
    assert rows_of(head, box) == [[2, 9, 1, 2, 3, 4], [2, -4, 0, 0, 1, 1]]
    head, box, _ = sampleprep.LabelSource(lab, n=0).job_rows(0, None)
    assert head.shape == (0, 2) and box.shape == (0, 4)


def test_job_table_of_a_batch_from_host_boxes():
    """what travels with the image table, and the finished table made of it (host tensors stand in for the uploaded buffer)"""
    lab = cases.sample(0)[1]
    srcs = [sampleprep.LabelSource(lab, jobs=[[9, 1, 2, 3, 4], [-4, 0, 0, 1, 1]]), sampleprep.LabelSource(lab, n=0),
            sampleprep.LabelSource(lab, n=2, stats=np.array([[6, 1, 2, 3, 5], [0, 9, 9, 9, 9]]))]
    rows = [s.job_rows(i, None) for i, s in enumerate(srcs)]
    want = [[0, 9, 1, 2, 3, 4], [0, -4, 0, 0, 1, 1], [2, 1, 1, 2, 3, 5], [2, 2, 0, 0, 0, 0]]
    flat = sampleprep._jobs_upload(rows)
    assert flat.dtype == np.int32 and flat.ndim == 1 and flat.reshape(4, 6).tolist() == want
    assert sampleprep._jobs_device(rows, torch.from_numpy(flat), 4).tolist() == want
    # one image's boxes as a tensor (device stats in a batch): the (img, id) columns first, then the boxes the host knows
    head, box, _ = rows[2]
    mixed = [rows[0], rows[1], (head, None, torch.from_numpy(np.ascontiguousarray(box)))]
    flat = sampleprep._jobs_upload(mixed)
    assert flat.tolist() == [0, 9, 0, -4, 2, 1, 2, 2, 1, 2, 3, 4, 0, 0, 1, 1]
    assert sampleprep._jobs_device(mixed, torch.from_numpy(flat), 4).tolist() == want


def test_from_instances_takes_the_table_boxes():
    from kg_instance_segmentation_amd import instances
    lab = np.zeros((20, 30), np.int32)
    lab[2:6, 3:9] = 1
    lab[10:12, 1:4] = 3                                                          # id 2 holds no visible pixel
    table = np.zeros((3, 8), np.int64)
    table[0] = [30, 24, 2, 3, 6, 9, 0, 0]
    table[1] = [12, 0, 7, 7, 9, 9, 0, 0]                                          # hidden: its full-mask box must not be used
    table[2] = [6, 6, 10, 1, 12, 4, 0, 0]
    src = sampleprep.LabelSource.from_instances(instances.Instances(lab, np.zeros((3, 5), np.float32), table, None))
    assert len(src) == 3 and rows_of(*src.job_rows(0, None)[:2]) == [[0, 1, 2, 3, 6, 9], [0, 2, 0, 0, 0, 0], [0, 3, 10, 1, 12, 4]]
    with pytest.raises(ValueError):
        sampleprep.LabelSource.from_instances(lab)


def test_a_mixed_batch_is_refused():
    img, lab, n, p, (H, W) = cases.sample(9)
    src = sampleprep.LabelSource(lab, n=n)
    for masks in ([src, cases.dense(lab, [1, 2])], [cases.dense(lab, [1, 2]), src]):
        with pytest.raises(ValueError, match="either all label sources"):
            sampleprep.prepare_batch([img, img], masks, [p, p], H, W)
        with pytest.raises(ValueError, match="either all label sources"):
            sampleprep.prepare_batch_full([img, img], masks, [p, p], H, W)


# ---- the C entries ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from kg_instance_segmentation_amd import build
    build.build()
    return _lib.load()


def test_entries_are_declared_bound_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "kgnet_hip.h")).read()
    for name, nargs in (("kg_sp_warp_labels", 9), ("kg_sp_warp_labelmap", 6)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert name in _lib.SYMBOLS and hasattr(lib, name) and len(_lib._SIGS[name]) == nargs
    assert "labels[sy][sx] == id" in hdr and "(unsigned)img < (unsigned)N" in hdr    # the statement itself
    for name in ("LabelSource", "warp_labels", "label_masks_host", "warp_labels_host"):
        assert hasattr(sampleprep, name)


def test_warp_labels_entry_refuses_bad_arguments_before_any_launch(lib):
    """every host check of kg_sp_warp_labels, on host memory: the entry may never get as far as a launch.  (The one check that cannot be
    made to fail is the size of the index type: every index is a 64-bit integer, and ntot * H * W < 2^31 * 2^16 * 2^12 fits it.)"""
    name = "kg_sp_warp_labels"
    buf = (ctypes.c_longlong * 8192)()
    p = ctypes.addressof(buf)
    assert p % 16 == 0
    IMGS, JOBS, OUT, BOX = (ctypes.c_void_p(p + k * 16384) for k in range(4))

    def call(imgs=IMGS, N=2, jobs=JOBS, ntot=3, H=8, W=8, out=OUT, box=BOX):
        return lib.kg_sp_warp_labels(imgs, N, jobs, ntot, H, W, out, box, None)

    def err(rc, text):
        msg = lib.kg_last_error().decode()
        assert rc != 0 and name in msg and text in msg, (rc, msg)

    for kw in (dict(imgs=None), dict(jobs=None), dict(out=None), dict(box=None)):
        err(call(**kw), "null pointer")
    for v in (0, -1, 65536, I32.max):
        err(call(N=v), f"N {v}")
    err(call(ntot=-1), "bad size")
    err(call(ntot=I32.min), "bad size")
    for h, w in ((0, 8), (8, 0), (-8, 8), (12, 8), (8, 12), (8, 4), (65536, 8), (8, 4104), (65544, 8)):
        err(call(H=h, W=w), "multiples of 8")
    err(call(jobs=ctypes.c_void_p(p + 16384 + 2)), "misaligned")
    err(call(box=ctypes.c_void_p(p + 3 * 16384 + 1)), "misaligned")
    err(call(out=ctypes.c_void_p(p + 2 * 16384 + 4), W=16), "misaligned")        # 16-byte stores where W % 16 == 0
    err(call(imgs=ctypes.c_void_p(p + 4)), "misaligned")
    # out holds 3 * 64 bytes, box 3 * 64, jobs 3 * 24, imgs 2 * 80
    err(call(out=BOX), "overlaps")
    err(call(out=JOBS), "overlaps")
    err(call(box=JOBS), "overlaps")
    err(call(out=ctypes.c_void_p(p + 3 * 16384 + 188)), "overlaps")              # starts at the last dword of box
    err(call(out=ctypes.c_void_p(p + 3 * 16384 - 4)), "overlaps")                # its last dword is the first of box
    err(call(out=ctypes.c_void_p(p + 16384 + 68)), "overlaps")                   # starts at the last dword of jobs
    err(call(box=ctypes.c_void_p(p + 16384 + 68)), "overlaps")
    err(call(out=ctypes.c_void_p(p + 156)), "overlaps")                          # starts at the last dword of imgs
    err(call(box=ctypes.c_void_p(p + 156)), "overlaps")
    # nothing to do: KG_OK with null buffers, yet the sizes are still checked
    assert call(ntot=0) == 0 and call(ntot=0, imgs=None, jobs=None, out=None, box=None) == 0
    assert call(ntot=0, N=65535, H=65528, W=4096, out=None, box=None, jobs=None) == 0
    err(call(ntot=0, N=0), "N 0")
    err(call(ntot=0, W=12), "multiples of 8")


def test_warp_labelmap_entry_refuses_bad_arguments_before_any_launch(lib):
    name = "kg_sp_warp_labelmap"
    buf = (ctypes.c_longlong * 4096)()
    p = ctypes.addressof(buf)
    IMGS, OUT = ctypes.c_void_p(p), ctypes.c_void_p(p + 16384)

    def call(imgs=IMGS, N=2, H=8, W=8, out=OUT):
        return lib.kg_sp_warp_labelmap(imgs, N, H, W, out, None)

    def err(rc, text):
        msg = lib.kg_last_error().decode()
        assert rc != 0 and name in msg and text in msg, (rc, msg)

    err(call(imgs=None), "null pointer")
    err(call(out=None), "null pointer")
    for v in (0, -1, 65536):
        err(call(N=v), f"N {v}")
    for h, w in ((0, 8), (12, 8), (8, 12), (65536, 8), (8, 4104)):
        err(call(H=h, W=w), "multiples of 8")
    err(call(out=ctypes.c_void_p(p + 16384 + 4)), "misaligned")
    err(call(imgs=ctypes.c_void_p(p + 4)), "misaligned")
    err(call(out=ctypes.c_void_p(p + 144)), "overlaps")                          # inside the image table
    err(call(imgs=ctypes.c_void_p(p + 16384 + 504)), "overlaps")                 # the table starts inside out's last bytes
