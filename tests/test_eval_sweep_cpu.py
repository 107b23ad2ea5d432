"""CPU: bit-packed masks and the single-pass evaluation.  The new entry points (kg_mask_paste_bits, kg_mask_pack_bits, kg_mask_unpack_bits,
kg_bitmask_areas, kg_bitmask_inter_pairs, kg_mask_bits_ld) are exported and bound and validate their arguments on the host before any HIP
call; the host packing states the layout of include/kgnet_hip.h; match_thresholds / Evaluator reproduce the reference's per-threshold
evaluation (golden fp / tp / scores / overlaps, and the AP aggregation of eval.py) from one IoU table per image."""
import ctypes
import subprocess

import numpy as np
import pytest

from kg_instance_segmentation_amd import _lib, bitmasks, evaluation
from oracle import evalparts as oev

NEW = ("kg_mask_bits_ld", "kg_mask_paste_bits", "kg_mask_pack_bits", "kg_mask_unpack_bits", "kg_bitmask_areas", "kg_bitmask_inter_pairs")
FAKE = ctypes.c_void_p(4096)     # (never dereferenced: every call below fails its host-side checks first)


@pytest.fixture(scope="module")
def lib():
    from kg_instance_segmentation_amd import build
    build.build()
    return _lib.load()


def _err(lib):
    return lib.kg_last_error().decode()


def test_new_symbols_exported_and_bound(lib):
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    for name in NEW:
        assert name in _lib._SIGS and name in _lib.SYMBOLS
        assert name in exported, name
        assert getattr(lib, name).argtypes == _lib._SIGS[name]
    assert lib.kg_mask_bits_ld.restype is ctypes.c_long
    # main library only: the half-precision build has no mask entry points
    nm16 = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_F16_PATH], capture_output=True, text=True, check=True).stdout
    assert not any(name in nm16 for name in NEW)


def _ld(H, W):
    return (H * ((W + 63) // 64) + 1) // 2 * 2


def test_bits_ld_is_the_stated_formula(lib):
    for H, W in ((64, 64), (512, 509), (520, 696), (1, 1), (1024, 1024)):
        assert lib.kg_mask_bits_ld(H, W) == _ld(H, W) == bitmasks.ld_words(H, W), (H, W)
    assert lib.kg_mask_bits_ld(64, 64) == 64 and lib.kg_mask_bits_ld(1, 1) == 2 and lib.kg_mask_bits_ld(512, 509) == 4096
    assert lib.kg_mask_bits_ld(0, 5) == -1 and "kg_mask_bits_ld" in _err(lib)
    assert lib.kg_mask_bits_ld(5, -1) == -1


def test_paste_bits_bad_arguments(lib):
    fn, t = lib.kg_mask_paste_bits, ctypes.c_float(0.5)
    ld = _ld(300, 200)
    assert fn(None, FAKE, 3, 256, 256, 300, 200, t, FAKE, ld, None) != 0 and "kg_mask_paste_bits: null pointer" in _err(lib)
    assert fn(FAKE, None, 3, 256, 256, 300, 200, t, FAKE, ld, None) != 0 and "null pointer" in _err(lib)
    assert fn(FAKE, FAKE, 3, 256, 256, 300, 200, t, None, ld, None) != 0 and "null pointer" in _err(lib)
    assert fn(FAKE, FAKE, -1, 256, 256, 300, 200, t, FAKE, ld, None) != 0 and "kg_mask_paste_bits: bad size" in _err(lib)
    assert fn(FAKE, FAKE, 3, 0, 256, 300, 200, t, FAKE, ld, None) != 0 and "bad size" in _err(lib)
    assert fn(FAKE, FAKE, 3, 256, 256, 300, 0, t, FAKE, ld, None) != 0 and "bad size" in _err(lib)
    assert fn(FAKE, FAKE, 3, 256, 256, 300, 200, t, FAKE, ld - 2, None) != 0 and "kg_mask_paste_bits: ld_words" in _err(lib)
    assert fn(FAKE, FAKE, 3, 256, 256, 300, 200, t, FAKE, ld + 1, None) != 0 and "ld_words" in _err(lib)
    assert fn(FAKE, FAKE, 0, 256, 256, 300, 200, t, FAKE, ld, None) == 0          # nothing to paste: no launch, as kg_mask_paste


def test_pack_unpack_bits_bad_arguments(lib):
    ld = _ld(64, 65)
    fn = lib.kg_mask_pack_bits
    assert fn(None, 0, 2, 64, 65, FAKE, ld, None) != 0 and "kg_mask_pack_bits: null pointer" in _err(lib)
    assert fn(FAKE, 0, 2, 64, 65, None, ld, None) != 0 and "null pointer" in _err(lib)
    assert fn(FAKE, 1, 0, 64, 65, FAKE, ld, None) != 0 and "kg_mask_pack_bits: bad size" in _err(lib)
    assert fn(FAKE, 1, 2, 64, 0, FAKE, ld, None) != 0 and "bad size" in _err(lib)
    assert fn(FAKE, 1, 2, -3, 65, FAKE, ld, None) != 0 and "bad size" in _err(lib)
    assert fn(FAKE, 0, 2, 64, 65, FAKE, 64, None) != 0 and "kg_mask_pack_bits: ld_words" in _err(lib)      # (one word per row: too small)
    assert fn(FAKE, 0, 2, 63, 65, FAKE, 63 * 2 + 1, None) != 0 and "ld_words" in _err(lib)                  # (odd)
    fn = lib.kg_mask_unpack_bits
    assert fn(None, ld, 2, 64, 65, FAKE, 1, None) != 0 and "kg_mask_unpack_bits: null pointer" in _err(lib)
    assert fn(FAKE, ld, 2, 64, 65, None, 1, None) != 0 and "null pointer" in _err(lib)
    assert fn(FAKE, ld, -1, 64, 65, FAKE, 1, None) != 0 and "kg_mask_unpack_bits: bad size" in _err(lib)
    assert fn(FAKE, ld, 2, 0, 65, FAKE, 0, None) != 0 and "bad size" in _err(lib)
    assert fn(FAKE, ld - 2, 2, 64, 65, FAKE, 0, None) != 0 and "kg_mask_unpack_bits: ld_words" in _err(lib)
    assert fn(FAKE, ld + 1, 2, 64, 65, FAKE, 0, None) != 0 and "ld_words" in _err(lib)


def test_bitmask_counts_bad_arguments(lib):
    fn = lib.kg_bitmask_areas
    assert fn(None, 3, 64, FAKE, None) != 0 and "kg_bitmask_areas: null pointer" in _err(lib)
    assert fn(FAKE, 3, 64, None, None) != 0 and "null pointer" in _err(lib)
    assert fn(FAKE, 0, 64, FAKE, None) != 0 and "kg_bitmask_areas: bad row count" in _err(lib)
    assert fn(FAKE, 3, 63, FAKE, None) != 0 and "kg_bitmask_areas: ld_words" in _err(lib)
    assert fn(FAKE, 3, 0, FAKE, None) != 0 and "ld_words" in _err(lib)
    assert fn(ctypes.c_void_p(4104), 3, 64, FAKE, None) != 0 and "16-byte" in _err(lib)
    fn = lib.kg_bitmask_inter_pairs
    assert fn(None, 3, FAKE, 3, FAKE, 5, 64, FAKE, None) != 0 and "kg_bitmask_inter_pairs: null pointer" in _err(lib)
    assert fn(FAKE, 3, None, 3, FAKE, 5, 64, FAKE, None) != 0 and "null pointer" in _err(lib)
    assert fn(FAKE, 3, FAKE, 3, None, 5, 64, FAKE, None) != 0 and "null pointer" in _err(lib)
    assert fn(FAKE, 3, FAKE, 3, FAKE, 5, 64, None, None) != 0 and "null pointer" in _err(lib)
    assert fn(FAKE, 0, FAKE, 3, FAKE, 5, 64, FAKE, None) != 0 and "kg_bitmask_inter_pairs: bad row or pair count" in _err(lib)
    assert fn(FAKE, 3, FAKE, 3, FAKE, 0, 64, FAKE, None) != 0 and "bad row or pair count" in _err(lib)
    assert fn(FAKE, 3, FAKE, 3, FAKE, 5, 65, FAKE, None) != 0 and "kg_bitmask_inter_pairs: ld_words" in _err(lib)
    assert fn(FAKE, 3, FAKE, 3, FAKE, 5, -2, FAKE, None) != 0 and "ld_words" in _err(lib)


@pytest.mark.parametrize("W", [1, 63, 64, 65, 509])
def test_host_pack_round_trip(W):
    rng = np.random.default_rng(W)
    H, n = 7, 3
    m = (rng.random((n, H, W)) > 0.5)
    for src in (m.astype(np.uint8), m.astype(np.float32) * 0.25, m):
        words = bitmasks.pack_host(src)
        assert words.dtype == np.uint64 and words.shape == (n, _ld(H, W))
        assert np.array_equal(bitmasks.unpack_host(words, H, W), m.astype(np.uint8))
        # the documented host recipe recovers the same pixels; the bits at x >= W and the padding word are zero
        wpr = (W + 63) // 64
        bits = np.unpackbits(words.view(np.uint8), axis=-1, bitorder="little")
        rows = bits[:, :H * wpr * 64].reshape(n, H, wpr * 64)
        assert np.array_equal(rows[:, :, :W], m.astype(np.uint8)) and not rows[:, :, W:].any() and not bits[:, H * wpr * 64:].any()
    assert bitmasks.pack_host(np.zeros((0, H, W), np.uint8)).shape == (0, _ld(H, W))
    assert bitmasks.unpack_host(np.zeros((0, _ld(H, W)), np.uint64), H, W).shape == (0, H, W)


def test_host_pack_is_the_literal_layout():
    H, W = 3, 70                                  # two words per row, 6 words, no padding word; (3, 3) below has one
    rng = np.random.default_rng(0)
    for H, W in ((3, 70), (3, 3), (1, 1), (2, 64)):
        m = (rng.random((2, H, W)) > 0.4).astype(np.uint8)
        m[0, H - 1, W - 1] = 1
        wpr = (W + 63) // 64
        ref = [[0] * _ld(H, W) for _ in range(2)]
        for k in range(2):
            for y in range(H):
                for x in range(W):
                    if m[k, y, x]:
                        ref[k][y * wpr + x // 64] |= 1 << (x % 64)
        assert bitmasks.pack_host(m).tolist() == ref


def _golden_case(g, name):
    return (g[f"{name}.gt_masks"], g[f"{name}.gt_boxes"], g[f"{name}.det_masks"], g[f"{name}.det"])


def _oracle_table(gm, dm, keep):
    iou = np.zeros(keep.shape, np.float64)
    for d, j in np.argwhere(keep):
        iou[d, j] = oev.mask_iou(dm[d], gm[j])
    return iou


@pytest.mark.parametrize("name", ["a", "b"])
def test_match_thresholds_vs_golden(golden, name):
    g = golden("evalparts.npz")
    gm, gb, dm, dd = _golden_case(g, name)
    keep = evaluation.box_keep(gb, dd[:, :4])
    assert keep.any() and np.array_equal(keep, np.array([oev._box_inter(gb, dd[d, :4]) > 0. for d in range(len(dd))]))
    m = evaluation.match_thresholds(dd[:, 4], keep, _oracle_table(gm, dm, keep), [0.5, 0.75])
    mb = evaluation.match_thresholds_boxes(dd, gb, [0.5, 0.75])
    for t, tag in enumerate(("50", "75")):
        k = f"{name}.seg{tag}"
        r = m["per_threshold"][t]
        assert np.array_equal(r["fp"], g[k + ".fp"]) and np.array_equal(r["tp"], g[k + ".tp"])
        assert np.array_equal(np.asarray(m["scores"], np.float32), g[k + ".scores"])
        assert np.array_equal(np.asarray(r["overlaps"], np.float64), g[k + ".overlaps"])
        k = f"{name}.box{tag}"
        assert np.array_equal(mb["per_threshold"][t]["fp"], g[k + ".fp"]) and np.array_equal(mb["per_threshold"][t]["tp"], g[k + ".tp"])
        assert np.array_equal(np.asarray(mb["scores"], np.float32), g[f"{name}.seg{tag}.scores"])
    assert m["per_threshold"][0]["tp"].sum() > m["per_threshold"][1]["tp"].sum() >= 1


def _aggregate(all_fp, all_tp, all_scores, npos):
    """eval.py:163-176 restated"""
    all_fp = np.asarray(all_fp); all_tp = np.asarray(all_tp); all_scores = np.asarray(all_scores)
    sorted_ind = np.argsort(-all_scores)
    all_fp = np.cumsum(all_fp[sorted_ind]); all_tp = np.cumsum(all_tp[sorted_ind])
    rec = all_tp / float(npos)
    prec = all_tp / np.maximum(all_tp + all_fp, np.finfo(np.float64).eps)
    return oev.voc_ap(rec, prec, use_07_metric=False)


def test_evaluator_summary_vs_per_threshold_oracle(golden):
    """Stream: case a, an image without prediction and 4 GT instances, case b -- fed with precomputed IoU tables (no GPU)."""
    g = golden("evalparts.npz")
    a, b = _golden_case(g, "a"), _golden_case(g, "b")
    none_boxes = np.array([[1, 1, 9, 9], [20, 20, 30, 31], [5, 40, 15, 50], [60, 60, 70, 70]], np.float32)
    stream = [a, (np.zeros((4, 96, 96), np.uint8), none_boxes, None, None), b]
    ev = evaluation.Evaluator()
    assert np.array_equal(ev.thresholds, np.linspace(0.5, 0.95, 10))
    preds = [None if dm is None else [None, dd] for _, _, dm, dd in stream]
    tables = [None if dm is None else _oracle_table(gm, dm, evaluation.box_keep(gb, dd[:, :4])) for gm, gb, dm, dd in stream]
    ev.add_batch(preds[:2], [s[0] for s in stream[:2]], [s[1] for s in stream[:2]], iou_tables=tables[:2])       # two calls: the state
    ev.add_batch(preds[2:], [s[0] for s in stream[2:]], [s[1] for s in stream[2:]], iou_tables=tables[2:])       # accumulates
    for gm, gb, dm, dd in stream:
        ev.add_boxes(dd, gb, (96, 96), (96, 96))
    got = ev.summary()
    tps = []
    for t, thr in enumerate(np.linspace(0.5, 0.95, 10)):
        all_fp, all_tp, all_scores, ovl, npos = [], [], [], [], 0
        bfp, btp, bsc, bnpos = [], [], [], 0
        for gm, gb, dm, dd in stream:
            if dm is None:
                npos += len(gb); bnpos += len(gb)
                continue
            fp, tp, conf, o = oev.seg_evaluation(gm, gb, dm, dd, thr)
            all_fp.extend(fp); all_tp.extend(tp); all_scores.extend(conf); ovl.extend(o); npos += len(gm)
            fp, tp, conf = oev.bbox_evaluation(gb, dd, thr)
            bfp.extend(fp); btp.extend(tp); bsc.extend(conf); bnpos += len(gb)
        assert npos == 20 and bnpos == 20
        tps.append(int(np.sum(all_tp)))
        assert got["seg_ap"][t] == _aggregate(all_fp, all_tp, all_scores, npos), thr
        if ovl:
            assert got["seg_iou"][t] == np.mean(ovl), thr
        else:
            assert np.isnan(got["seg_iou"][t])
        assert got["dec_ap"][t] == _aggregate(bfp, btp, bsc, bnpos), thr
    print("true positives per threshold", tps, "seg_ap", got["seg_ap"])
    assert tps[0] == 12 and tps[0] > tps[5] >= 1 and got["seg_ap"][0] > got["seg_ap"][5] > 0
