"""The detection stage (csrc/postproc.hip behind postprocessing.py and nms.py) against the C oracle, bit for bit, where its kernels change path.

Every comparison is np.array_equal with oracle/postproc.py (pinned to the reference by tests/test_oracle_postproc.py); tests/detect_cases.py holds
the seeded inputs, tests/test_detect_cases_cpu.py asserts from the oracle alone that they reach what is claimed here.  Every output buffer handed to
the C ABI is the inner part of a larger allocation pre-filled with NaN (or -7): the rows in front of it, behind its stated capacity and behind the
returned count have to come back unchanged.

A  STAGES.  heat, blur, peaks (ids, xs, ys), peak confidences and skeletons of skeletons_device(debug=True) on maps that are no multiple of the
   32 x 32 Hough tile, of the grouping cells or of the 1024-element peak chunk (1 x 1, 1 x 70, 70 x 1, 25 x 17, 33 x 70, 31 x 97, 65 x 87), and on
   strips that cross the seams of group_kernel in both orientations: cells of 8 / 16 px at 256 | 257, of 16 / 32 px at 512 | 513, the LDS path
   against the general one at 1024 | 1025.  Random (untrained-network) maps and synth.head_maps objects.  The same tests run once more in a child
   process with KG_HOUGH_TILE=0 (the scatter formulation of the vote; the library reads the switch once); after a child that died on a signal,
   hung or reported a GPU fault this file starts nothing more on the GPU.  Batched: three images per kg_postproc_batch call.  End to end: detect and
   detect_batch on the four head maps of a 200 x 136 image (200 x 136 .. 25 x 17), one image of the batch empty.
B  BOX ASSEMBLY.  kg_skeleton_boxes / kg_skeleton_boxes_batch on tables that cycle through all 32 keypoint masks (every branch of skeleton_box):
   the 1024-row chunk seam (1, 1023, 1024, 1025, 2049, 3000 rows), the carry of the row offset over chunks, scales and appending calls,
   nskel > skel_cap, more boxes than box_cap, a batch whose images have 0, 1, 1025 and 2049 rows.
C  NMS.  kg_nms / kg_nms_batch / non_maximum_suppression_numpy on populations in which equal confidences are the rule: 2047 / 2048 boxes (LDS path)
   against 2049 / 5000 (global path), exact duplicates, zero-area boxes (0 / 0), negative and inverted boxes, thresholds 0, 0.1, 0.5, 1, the
   clamp of nbox to box_cap, a batch whose images take different paths, a 9 x 9 grid in which suppression chains.  Besides the kept rows the
   kept INDICES are compared (read from the workspace: [order | keep | dead], as kg_nms lays it out), which is what tells equal rows apart.
   The path is chosen by min(nbox, box_cap), not by box_cap: the two runs of the 2048-row prefix the case list asks for (box_cap 2048; the first
   2048 of 2049 rows with nbox = 2048) both take the LDS path.  The prefix plus one far box of the lowest confidence takes the global path and has
   to keep the same rows, then that box.
D  CAPACITIES of kg_postproc_scale / kg_postproc_batch, as include/kgnet_hip.h now states them: npeaks_out is the full count, the first
   min(T, peak_cap) peaks in scan order are returned, ranked and grouped, nskel counts the skeletons formed, rows [: min(nskel, skel_cap)] are
   written.  On the LDS path of the grouping nskel is the full count of the oracle's grouping even when skel_cap is exceeded (asserted); on the
   general path a skeleton beyond skel_cap is not recorded and so cannot stop a later seed within 10 px of it: nskel is then only known to
   exceed skel_cap (the first skel_cap rows are the oracle's either way).

Two statements of the case list did not survive the oracle and are tested as the oracle has them: (1) equal confidences are ranked by index
ascending and picked from the top, so of exact duplicates the LATER index is kept and the earlier ones lose; (2) with do_refine the two rejecting
branches of skeleton_box are unreachable -- refine_skeleton keeps exactly the rows skeleton_box accepts (test_detect_cases_cpu).
No case failed against the library as it stands: nothing in postproc.hip had to change.

MEASURED on MI355X, 2026-10-21, on this file as committed: 119 tests, all passing, wall time of the file 8.4 s -- the KG_HOUGH_TILE=0 child
(25 tests) 4.7 s of it, the slowest other test 0.23 s (1 x 1, the first launch of the process).  Values compared with the oracle, all equal:
A 2 425 842 (the child repeats the stage tests' share of them), B 203 575, C 302 924, D 851 790.
Checked once against scratch builds of postproc.hip with one seam broken (wrong results only, every index in bounds): without the s_base carry
between the chunks of boxes_kernel the twenty part-B tests with more than 1024 rows, an append or a batch fail and nothing else; with the cell
grid of group_fast cut to W >> CS instead of rounded up, 27 tests of parts A and D fail -- every size with a partial cell on the LDS path, the
batched, end-to-end and child runs included -- while the multiples of the cell (24 x 256, 40 x 256) and the general path (1025) pass.
"""
import os
import subprocess
import sys
from ctypes import c_double, c_int, c_long, c_void_p

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import detect_cases as dc  # noqa: E402
from kg_instance_segmentation_amd import _lib  # noqa: E402
from kg_instance_segmentation_amd import nms as knms  # noqa: E402
from kg_instance_segmentation_amd import postprocessing as kpp  # noqa: E402
from kg_instance_segmentation_amd._lib import ptr, stream_ptr  # noqa: E402
from oracle import postproc as op  # noqa: E402

DEV = "cuda"
G = 8                                   # guard rows in front of and behind every output
NAN = float("nan")
COMPARED = {"A": 0, "B": 0, "C": 0, "D": 0}
_DIED = []


@pytest.fixture(autouse=True)
def _nothing_after_a_dead_child():
    assert not _DIED, "not started: the KG_HOUGH_TILE=0 child died, hung or reported a GPU fault"


def up(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)          # (a copy: the cached cases are read-only)


def same(part, name, got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    bad = np.argwhere(got != ref)
    assert np.array_equal(got, ref), (name, len(bad), [(tuple(i), got[tuple(i)], ref[tuple(i)]) for i in bad[:4]])
    COMPARED[part] += int(ref.size)


def untouched(a, fill):
    a = np.asarray(a)
    return bool(np.isnan(a).all()) if fill != fill else bool((a == fill).all())


def guarded(rows, tail, fill, dtype):
    """-> (the whole allocation [G + rows + G, *tail] filled with `fill`, its inner rows: the buffer the entry point gets)"""
    full = torch.full((G + rows + G,) + tuple(tail), fill, dtype=dtype, device=DEV)
    return full, full[G:G + rows]


def inner(full, rows, fill, written=None):
    """host copy of the inner rows after asserting that the guards -- and the rows from `written` on -- still hold `fill`"""
    h = full.cpu().numpy()
    assert untouched(h[:G], fill) and untouched(h[G + rows:], fill), "guard rows written"
    body = h[G:G + rows]
    if written is not None:
        assert untouched(body[written:], fill), "rows behind the returned count written"
    return body


# ---- part A: stages ---------------------------------------------------------------------------------------------------------------------------

def run_stages(kp, short, mid):
    t = [up(a) for a in (kp, short, mid)]
    skel, nsk, dbg = kpp.skeletons_device(*t, debug=True)
    torch.cuda.synchronize()
    npk = int(dbg["npeaks"].item())
    return dict(heat=dbg["heat"].cpu().numpy(), blur=dbg["blur"].cpu().numpy(), peaks=dbg["peaks"][:, :npk].cpu().numpy().T,
                peak_conf=dbg["conf"][:npk].cpu().numpy(), skel=skel[:int(nsk.item())].cpu().numpy(), npeaks=npk)


def check_stages(got, ref):
    assert got["npeaks"] == ref["npeaks"]
    for k in ("heat", "blur", "peaks", "peak_conf", "skel"):
        same("A", k, got[k], ref[k])


def size_id(s):
    return f"{s[0]}x{s[1]}"


@pytest.mark.parametrize("size", dc.RAGGED + dc.SEAMS, ids=size_id)
def test_stages_random_maps(size):
    check_stages(run_stages(*dc.stage_maps(*size)), dc.stage_reference(*size))


@pytest.mark.parametrize("case", dc.SYNTH, ids=lambda c: f"{c[0]}x{c[1]}")
def test_stages_synth_objects(case):
    check_stages(run_stages(*dc.synth_maps(*case)), dc.synth_reference(*case))
    sk = kpp.get_skeletons_and_masks(*[up(a) for a in dc.synth_maps(*case)])
    assert len(sk) == len(dc.synth_reference(*case)["skel"]) and all(np.array_equal(a, b) for a, b in zip(sk, dc.synth_reference(*case)["skel"]))


@pytest.mark.parametrize("size", dc.BATCH_SIZES, ids=size_id)
def test_batched_images_equal_their_own_oracle(size):
    H, W = size
    maps = [dc.random_maps(H, W, dc.default_seed(H, W) + 1 + i) for i in range(3)]
    skel, nsk = kpp.skeletons_batch_device(*[up(np.concatenate([m[k] for m in maps], 0)) for k in range(3)])
    torch.cuda.synchronize()
    nsk, skel = nsk.cpu().numpy(), skel.cpu().numpy()
    for i, m in enumerate(maps):
        ref = dc.oracle_stages(*m)["skel"]
        assert nsk[i] == len(ref) and len(ref) >= 20, i
        same("A", f"image {i}", skel[i, :nsk[i]], ref)


def test_end_to_end_200x136():
    decs, refs = dc.end_to_end()
    dec = [[up(np.concatenate([d[l][k] for d in decs], 0)) for k in range(3)] for l in range(4)]
    got = kpp.detect_batch(dec, 0.5)
    assert len(got) == 3 and got[1] is None and refs[1] is None
    for i in (0, 2):
        same("A", f"detect_batch image {i}", got[i], refs[i])
    for i in range(3):
        one = kpp.detect([[t[i:i + 1] for t in d] for d in dec], 0.5)
        if refs[i] is None:
            assert one is None
        else:
            same("A", f"detect image {i}", one, refs[i])


# ---- part B: box assembly ---------------------------------------------------------------------------------------------------------------------------

class BoxBuffer:
    """boxes [cap, 5] between guard rows and a device counter, for kg_skeleton_boxes (which appends behind nbox)"""

    def __init__(self, cap):
        self.cap = cap
        self.full, self.rows = guarded(cap, (5,), NAN, torch.float64)
        self.nbox = torch.zeros(1, dtype=torch.int32, device=DEV)

    def append(self, table, scale, do_refine, nskel=None, skel_cap=None):
        """table: host [n, 5, 3]; nskel / skel_cap default to n"""
        n = len(table)
        sk = up(np.asarray(table, np.float64).reshape(n, 15))
        skel_cap = n if skel_cap is None else skel_cap
        assert 1 <= skel_cap <= n                      # the entry reads min(nskel, skel_cap) rows: all inside `sk`
        ns = torch.tensor([n if nskel is None else nskel], dtype=torch.int32, device=DEV)
        _lib.call("kg_skeleton_boxes", ptr(sk), ptr(ns), skel_cap, c_double(scale), do_refine, ptr(self.rows), ptr(self.nbox), self.cap, stream_ptr())

    def result(self):
        torch.cuda.synchronize()
        n = int(self.nbox.item())
        return n, inner(self.full, self.cap, NAN, written=min(n, self.cap))[:min(n, self.cap)]


@pytest.mark.parametrize("do_refine", [0, 1])
@pytest.mark.parametrize("scale", [1, 8])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049, 3000])
def test_boxes_chunk_seams(n, scale, do_refine):
    t = dc.skeleton_table(n, n)
    ref = dc.boxes_reference(t, scale, do_refine)
    buf = BoxBuffer(n)
    buf.append(t, scale, do_refine)
    k, rows = buf.result()
    assert k == len(ref)
    same("B", "boxes", rows, ref)


def test_boxes_of_nothing():
    assert kpp.skeleton_to_box([], 4) == [] and kpp.gather_skeleton([], [], [], []).shape == (0,)     # (the wrapper launches nothing)
    buf = BoxBuffer(4)
    buf.append(np.zeros((1, 5, 3)), 2, 0, nskel=0)          # through the C ABI: no row is read, none written, nbox stays 0
    assert buf.result()[0] == 0


def test_skeleton_to_box_python_level():
    t = dc.skeleton_table(2049, 2049)
    rows = [r.copy() for r in t]
    got = np.asarray(kpp.skeleton_to_box(rows, 8)).reshape(-1, 5)
    same("B", "skeleton_to_box", got, op.boxes(t, 8))
    scaled = t.copy(); scaled[:, :, :2] *= 8
    same("B", "scaled in place", np.asarray(rows), scaled)


APPEND = [(1500, 1), (700, 2), (0, 4), (40, 8)]


@pytest.mark.parametrize("do_refine", [0, 1])
def test_boxes_append_over_scales(do_refine):
    tables = [dc.skeleton_table(n, 50 + i) for i, (n, _) in enumerate(APPEND)]
    ref = op.gather(*[op.refine(t) if do_refine and len(t) else t for t in tables])
    buf = BoxBuffer(2240)
    for t, (n, scale) in zip(tables, APPEND):
        if n:
            buf.append(t, scale, do_refine)
    k, rows = buf.result()
    assert k == len(ref) and k > 1024
    same("B", "four appending calls", rows, ref)
    # the same tables as the four scales of ONE kg_skeleton_boxes_batch call with N = 1 (an empty scale: one unread row, nskel 0)
    dev = [up((t if len(t) else np.zeros((1, 5, 3))).reshape(-1, 15)) for t in tables]
    cnt = [torch.tensor([len(t)], dtype=torch.int32, device=DEV) for t in tables]
    full, out = guarded(2240, (5,), NAN, torch.float64)
    nbox = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    _lib.call("kg_skeleton_boxes_batch", 1, 4, (c_void_p * 4)(*[d.data_ptr() for d in dev]), (c_void_p * 4)(*[c.data_ptr() for c in cnt]),
              (c_int * 4)(*[d.shape[0] for d in dev]), (c_double * 4)(*[float(s) for _, s in APPEND]), do_refine, ptr(out), ptr(nbox), 2240, stream_ptr())
    torch.cuda.synchronize()
    assert int(nbox.item()) == len(ref)
    same("B", "one batch call", inner(full, 2240, NAN, written=len(ref))[:len(ref)], ref)


@pytest.mark.parametrize("do_refine", [0, 1])
def test_boxes_nskel_beyond_skel_cap(do_refine):
    """nskel = skel_cap + 500: boxes_kernel clamps to skel_cap (`if (n > skcap) n = skcap`).  The 500 rows behind skel_cap exist in the
    allocation and are complete skeletons, so a lost clamp shows as 500 more boxes."""
    cap = 1100
    t = dc.skeleton_table(cap + 500, 7)
    t[cap:] = dc.skeleton_table(32, 8)[31]
    ref = dc.boxes_reference(t[:cap], 2, do_refine)
    buf = BoxBuffer(cap + 500)
    buf.append(t, 2, do_refine, nskel=cap + 500, skel_cap=cap)
    k, rows = buf.result()
    assert k == len(ref)
    same("B", "clamped", rows, ref)


def test_boxes_beyond_box_cap():
    """more boxes than box_cap: nbox is the full count, the first box_cap rows are written, and a later appending call writes nothing and adds
    its own count"""
    t, t2 = dc.skeleton_table(3000, 3000), dc.skeleton_table(700, 701)
    ref, ref2 = op.boxes(t, 2), op.boxes(t2, 4)
    assert len(ref) > 1000 and len(ref2) > 0
    buf = BoxBuffer(1000)
    buf.append(t, 2, 0)
    k, rows = buf.result()
    assert k == len(ref)
    same("B", "first box_cap rows", rows, ref[:1000])
    buf.append(t2, 4, 0)
    k, rows = buf.result()
    assert k == len(ref) + len(ref2)
    same("B", "unchanged by the call after the overflow", rows, ref[:1000])


@pytest.mark.parametrize("do_refine", [0, 1])
def test_boxes_batch_of_unequal_images(do_refine):
    counts, scales, cap, box_cap = [0, 1, 1025, 2049], (1, 2), 2049, 2400
    tables = [[dc.skeleton_table(n, 100 * s + i) for i, n in enumerate(counts)] for s in range(2)]
    none = np.zeros((0, 5, 3))
    refs = [op.gather(*[op.refine(tables[s][i]) if do_refine and counts[i] else tables[s][i] for s in range(2)], none, none) for i in range(4)]
    assert max(len(r) for r in refs) <= box_cap
    skel = []
    for s in range(2):
        a = np.full((4, cap, 5, 3), NAN)
        for i, n in enumerate(counts):
            a[i, :n] = tables[s][i]
        skel.append(up(a))
    cnt = [torch.tensor(counts, dtype=torch.int32, device=DEV) for _ in range(2)]
    full, out = guarded(4 * box_cap, (5,), NAN, torch.float64)
    nbox = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    _lib.call("kg_skeleton_boxes_batch", 4, 2, (c_void_p * 2)(*[d.data_ptr() for d in skel]), (c_void_p * 2)(*[c.data_ptr() for c in cnt]),
              (c_int * 2)(cap, cap), (c_double * 2)(*[float(s) for s in scales]), do_refine, ptr(out), ptr(nbox), box_cap, stream_ptr())
    torch.cuda.synchronize()
    body = inner(full, 4 * box_cap, NAN).reshape(4, box_cap, 5)
    assert nbox.cpu().tolist() == [len(r) for r in refs] and len(refs[0]) == 0
    for i, r in enumerate(refs):
        same("B", f"image {i}", body[i, :len(r)], r.reshape(-1, 5))
        assert untouched(body[i, len(r):], NAN), i               # image 0: nothing at all


# ---- part C: NMS --------------------------------------------------------------------------------------------------------------------------------

def al256(v):
    return (v + 255) & ~255


def nms_call(boxes, nbox, box_cap, thresh):
    """kg_nms on host boxes [>= box_cap, 5] -> (nkeep, kept rows, kept indices); out lies between guard rows, nkeep starts as -7"""
    assert len(boxes) >= box_cap >= 1                       # the entry reads min(nbox, box_cap) rows
    bd = up(np.asarray(boxes, np.float64))
    nb = torch.tensor([nbox], dtype=torch.int32, device=DEV)
    nws = _lib.load().kg_nms_batch_workspace_bytes(1, box_cap)
    ws = torch.zeros(nws, dtype=torch.uint8, device=DEV)
    full, out = guarded(box_cap, (5,), NAN, torch.float64)
    nk = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    _lib.call("kg_nms", ptr(bd), ptr(nb), box_cap, c_double(thresh), ptr(ws), c_long(nws), ptr(out), ptr(nk), stream_ptr())
    torch.cuda.synchronize()
    k = int(nk.item())
    assert 0 <= k <= box_cap
    rows = inner(full, box_cap, NAN, written=k)[:k]
    keep = ws.cpu().numpy()[al256(box_cap * 4):][:4 * k].copy().view(np.int32)
    return k, rows, keep


def check_nms(got, boxes, keep_ref):
    k, rows, keep = got
    assert k == len(keep_ref)
    same("C", "pick order", keep, keep_ref)
    same("C", "kept rows", rows, np.asarray(boxes)[keep_ref].reshape(-1, 5))


NMS_NAMES = [str(n) for n in dc.NMS_SIZES] + ["300+specials", "2049+specials"]


@pytest.mark.parametrize("thresh", dc.NMS_THRESHOLDS)
@pytest.mark.parametrize("name", NMS_NAMES)
def test_nms_sizes(name, thresh):
    b = dc.nms_case(name)
    ref = dc.nms_reference(name, thresh)
    assert np.array_equal(b[ref], op.nms(b, thresh))
    check_nms(nms_call(b, len(b), len(b), thresh), b, ref)


def test_nms_numpy_entry():
    b = dc.nms_case("2049")
    same("C", "non_maximum_suppression_numpy", knms.non_maximum_suppression_numpy(b.copy(), 0.5), b[dc.nms_reference("2049", 0.5)])
    assert knms.non_maximum_suppression_numpy(np.zeros((0, 5)), 0.5) is None
    g = dc.nms_case("grid")
    same("C", "grid through numpy", knms.non_maximum_suppression_numpy(g.copy(), 0.3), g[dc.nms_reference("grid", 0.3)])


@pytest.mark.parametrize("thresh", [0.1, 0.5])
def test_nms_prefix_on_both_paths(thresh):
    b = dc.nms_case("2049")
    ref = dc.nms_pick(b[:2048], thresh)
    check_nms(nms_call(b[:2048], 2048, 2048, thresh), b, ref)                 # box_cap 2048
    check_nms(nms_call(b, 2048, 2049, thresh), b, ref)                        # the first 2048 of 2049 rows: still n = 2048, the LDS path
    far = np.concatenate([b[:2048], [[5000., 5000., 5010., 5010., -1.]]], 0)  # n = 2049: the global path; the far box is picked last
    want = np.concatenate([ref, [2048]]).astype(np.int32)
    assert np.array_equal(dc.nms_pick(far, thresh), want)
    check_nms(nms_call(far, 2049, 2049, thresh), far, want)


@pytest.mark.parametrize("name,cap", [("300", 200), ("2049", 1949), ("5000", 4900)])
def test_nms_clamps_nbox_to_box_cap(name, cap):
    """nbox = box_cap + 100 (nms_kernel: `if (n > boxcap) n = boxcap`); the 100 rows exist, so a lost clamp would show in the result"""
    b = dc.nms_case(name)
    check_nms(nms_call(b, cap + 100, cap, 0.5), b, dc.nms_pick(b[:cap], 0.5))


def test_nms_of_no_box():
    k, rows, _ = nms_call(dc.nms_case("300")[:16], 0, 16, 0.5)               # (nms_call asserts that out is untouched behind nkeep = 0)
    assert k == 0 and len(rows) == 0


@pytest.mark.parametrize("thresh", [0.1, 0.5])
def test_nms_batch_of_unequal_images(thresh):
    """five images in one kg_nms_batch call: none, one, the LDS path at its limit, the global path, a small one -- every image's rows equal the
    oracle's (and so test_nms_sizes' single-image calls) and start behind the rows of the images before it"""
    names, cap = [None, "1", "2048", "2049", "300"], 2049
    boxes = np.full((5, cap, 5), NAN)
    counts = []
    for i, nm in enumerate(names):
        n = 0 if nm is None else len(dc.nms_case(nm))
        counts.append(n)
        if n:
            boxes[i, :n] = dc.nms_case(nm)
    refs = [np.zeros((0, 5)) if nm is None else dc.nms_case(nm)[dc.nms_reference(nm, thresh)] for nm in names]
    bd = up(boxes)
    nb = torch.tensor(counts, dtype=torch.int32, device=DEV)
    nws = _lib.load().kg_nms_batch_workspace_bytes(5, cap)
    ws = torch.zeros(nws, dtype=torch.uint8, device=DEV)
    full, out = guarded(5 * cap, (5,), NAN, torch.float64)
    nk = torch.full((5,), -7, dtype=torch.int32, device=DEV)
    _lib.call("kg_nms_batch", 5, ptr(bd), ptr(nb), cap, c_double(thresh), ptr(ws), c_long(nws), ptr(out), ptr(nk), stream_ptr())
    torch.cuda.synchronize()
    assert nk.cpu().tolist() == [len(r) for r in refs]
    total = sum(len(r) for r in refs)
    same("C", "rows of all images", inner(full, 5 * cap, NAN, written=total)[:total], np.concatenate(refs, 0))


def test_nms_grid_chains():
    g = dc.nms_case("grid")
    check_nms(nms_call(g, 81, 81, 0.3), g, dc.nms_reference("grid", 0.3))
    assert len(dc.nms_reference("grid", 0.3)) == 41


# ---- part D: capacities ---------------------------------------------------------------------------------------------------------------------------

def postproc_call(maps, peak_cap, skel_cap, thresh=0.004):
    """kg_postproc_scale with every output between guard rows -> dict of host arrays (counters start as -7)"""
    kp, short, mid = [up(a[0]) for a in maps]
    H, W = kp.shape[-2:]
    nws = _lib.load().kg_postproc_workspace_bytes(H, W, peak_cap, skel_cap)
    ws = torch.zeros(nws, dtype=torch.uint8, device=DEV)
    f_skel, skel = guarded(skel_cap, (5, 3), NAN, torch.float64)
    f_heat, heat = guarded(5 * H, (W,), NAN, torch.float64)
    f_blur, blur = guarded(5 * H, (W,), NAN, torch.float64)
    f_pk, pk = guarded(3 * peak_cap, (), -7, torch.int32)
    f_cf, cf = guarded(peak_cap, (), NAN, torch.float64)
    nsk = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    npk = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    _lib.call("kg_postproc_scale", ptr(kp), ptr(short), ptr(mid), H, W, c_double(thresh), ptr(ws), c_long(nws), peak_cap, skel_cap, ptr(skel), ptr(nsk),
              ptr(heat), ptr(blur), ptr(pk), ptr(cf), ptr(npk), stream_ptr())
    torch.cuda.synchronize()
    T, ns = int(npk.item()), int(nsk.item())
    m = min(T, peak_cap)
    peaks = inner(f_pk, 3 * peak_cap, -7).reshape(3, peak_cap)[:, :m].T
    return dict(npeaks=T, nskel=ns, heat=inner(f_heat, 5 * H, NAN).reshape(5, H, W), blur=inner(f_blur, 5 * H, NAN).reshape(5, H, W), peaks=peaks,
                peak_conf=inner(f_cf, peak_cap, NAN)[:m], skel=inner(f_skel, skel_cap, NAN, written=min(ns, skel_cap))[:min(ns, skel_cap)])


@pytest.mark.parametrize("case", dc.CAP_CASES, ids=lambda c: f"{c[0]}x{c[1]}-peaks{c[2]}-skel{c[3]}")
def test_capacities_of_postproc_scale(case):
    """npeaks is the full count; peaks, ranking and grouping are those of the first peak_cap peaks in scan order; nskel counts the skeletons formed
    -- the oracle's full count wherever the LDS path of group_kernel runs or skel_cap suffices -- and rows [: min(nskel, skel_cap)] are written"""
    H, W, peak_cap, skel_cap = case
    ref = dc.cap_reference(H, W, peak_cap)
    got = postproc_call(dc.random_maps(H, W), peak_cap, skel_cap)
    assert got["npeaks"] == ref["npeaks"]
    for k in ("heat", "blur", "peaks", "peak_conf"):
        same("D", k, got[k], ref[k])
    if case in dc.SKEL_OVERFLOW:
        assert got["nskel"] > skel_cap
    if dc.group_route(min(peak_cap, ref["npeaks"]), H, W) != "general" or case not in dc.SKEL_OVERFLOW:
        assert got["nskel"] == len(ref["skel"])
    same("D", "skel", got["skel"], ref["skel"][:skel_cap])


def test_capacities_per_image_of_postproc_batch():
    """one kg_postproc_batch call, peak_cap = 200, over images with fewer, exactly 200 and more peaks: every image equals the oracle's grouping of
    its own first 200 peaks"""
    maps, thresh, refs = dc.cap_batch()
    H, W, cap = 65, 87, dc.CAP_BATCH_PEAK_CAP
    dev = [up(np.concatenate([m[k] for m in maps], 0)) for k in range(3)]
    nws = _lib.load().kg_postproc_batch_workspace_bytes(3, H, W, cap, cap)
    ws = torch.zeros(nws, dtype=torch.uint8, device=DEV)
    full, skel = guarded(3 * cap, (5, 3), NAN, torch.float64)
    nsk = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    _lib.call("kg_postproc_batch", ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), 3, H, W, c_double(thresh), ptr(ws), c_long(nws), cap, cap, ptr(skel), ptr(nsk),
              stream_ptr())
    torch.cuda.synchronize()
    body = inner(full, 3 * cap, NAN).reshape(3, cap, 5, 3)
    assert nsk.cpu().tolist() == [len(r["skel"]) for r in refs]
    for i, r in enumerate(refs):
        same("D", f"image {i}", body[i, :len(r["skel"])], r["skel"])
        assert untouched(body[i, len(r["skel"]):], NAN), i


# ---- the scatter formulation, last: nothing of this file runs on the GPU after a child that died ---------------------------------------------------

def test_stages_with_the_scatter_formulation_in_a_child_process():
    """KG_HOUGH_TILE=0: test_stages_random_maps and test_stages_synth_objects once more in a process that selects the scatter formulation"""
    if os.environ.get("KG_HOUGH_TILE") == "0":
        return                  # (this IS the child)
    n = len(dc.RAGGED) + len(dc.SEAMS) + len(dc.SYNTH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "test_stages_random_maps or test_stages_synth_objects"],
                           capture_output=True, text=True, env=dict(os.environ, KG_HOUGH_TILE="0"), cwd=root, timeout=240)
    except subprocess.TimeoutExpired:
        _DIED.append("timeout")
        raise
    out = r.stdout + r.stderr
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or "illegal memory access" in out or "HSA_STATUS_ERROR" in out or "Memory access fault" in out:
        _DIED.append(r.returncode)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert f"{n} passed" in r.stdout.splitlines()[-1], r.stdout[-500:]


def test_report_compared_values():
    """(report) values compared with the oracle by this process, per part"""
    print("[detect] compared values per part:", COMPARED)
