"""GPU: bit-packed masks and the single-pass evaluation.  kg_mask_paste_bits gives kg_mask_paste's pixels bit for bit; packing on the
host and on the device give the same words; predict(packed=True) equals predict(); areas / intersections on bits are exact; Evaluator and
evaluate() equal the existing per-threshold path (eval_parts.seg_evaluation / bbox_evaluation, ten runs, aggregated as eval.py does)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from kg_instance_segmentation_amd import KGnet, _lib, eval_parts as kev, evaluation, inference, postprocessing as kpp  # noqa: E402
from kg_instance_segmentation_amd.bitmasks import BitMasks, ld_words, pack_host, unpack_host  # noqa: E402
from oracle import evalparts as oev, weightgen  # noqa: E402

DEV = "cuda"
THR = np.linspace(0.5, 0.95, 10)
MIXED = [(256, 256), (300, 200), (256, 256), (520, 696)]


class _DS:
    def __init__(self, gm, gb):
        self.gm, self.gb = gm, gb

    def load_annotation(self, index, type):
        return self.gm[index] if type == "mask" else self.gb[index]


@pytest.fixture(scope="module")
def cal():
    """calibrated-weights model, a 256^2 batch of 4, its forward_dec outputs, detections and forward_seg rows"""
    m = KGnet.resnet50(pretrained=False)
    m.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    m = m.to(DEV).eval()
    x = (torch.rand(4, 3, 256, 256, generator=torch.Generator().manual_seed(7)) - 0.5).to(DEV)
    with torch.no_grad():
        out = m.forward_dec(x)
        dec, feats = list(out[:4]), out[4]
        dets = kpp.detect_batch(dec, 0.5)
        assert any(d is not None for d in dets)
        pred = m.forward_seg(feats, [d if d is not None else np.zeros((0, 5)) for d in dets])
    return m, x, dec, feats, dets, pred.kg_meta


def _check_padding(words, h, w):
    """bits at x >= w and the words from h * wpr on are zero"""
    wpr = (w + 63) // 64
    assert words.shape[1] == ld_words(h, w)
    assert not words[:, h * wpr:].any()
    if w % 64:
        last = words[:, :h * wpr].reshape(len(words), h, wpr)[:, :, -1]
        assert not (last >> np.uint64(w % 64)).any()


@pytest.mark.parametrize("size", [(256, 256), (300, 200), (520, 696)])
def test_paste_bits_equals_paste_u8(cal, size):
    meta = cal[5]
    h, w = size
    args = (meta["flat"], meta["off"], meta["h"], meta["w"], meta["boxes"], 256, 256, w, h, 0.5)
    u8, d0 = kpp.paste_rows(*args, device_u8=True)
    bm, d1 = kpp.paste_rows(*args, packed=True)
    assert isinstance(bm, BitMasks) and bm.shape == tuple(u8.shape) and len(bm) == len(meta["off"]) > 0
    words = bm.words_cpu()
    ref = u8.cpu().numpy()
    print(f"{size}: {len(bm)} masks, {int(ref.sum())} foreground pixels, {bm.nbytes} bytes packed / {ref.nbytes} as bytes")
    assert ref.any() and not ref.all()
    assert np.array_equal(unpack_host(words, h, w), ref)
    _check_padding(words, h, w)
    assert np.array_equal(d0, d1)
    assert torch.equal(bm.to_u8(), u8)


@pytest.mark.parametrize("out_size", [(61, 67), (75, 50), (130, 200)])
@pytest.mark.parametrize("thresh", [0.5, 0.0])
def test_paste_bits_hand_made_table(out_size, thresh):
    """Input 61 x 67; an empty box (y2 <= y1), an empty box (x2 <= x1), boxes at the four image borders, a 1-pixel box, boxes whose patch
    has / has not the box's size.  (75, 50) has an odd word count: the padding word is written.  thresh 0: the pixels outside count."""
    in_h, in_w = 61, 67
    rng = np.random.default_rng(11)
    rows = [(5, 7, 30, 30, 30, 52),      # y2 <= y1
            (5, 7, 10, 40, 30, 40),      # x2 <= x1
            (9, 11, 0, 0, 20, 25),       # top-left corner
            (12, 8, 40, 45, 60, 66),     # bottom-right corner (clamped to input - 1)
            (61, 67, 0, 0, 60, 66),      # the whole image
            (3, 3, 33, 21, 34, 22),      # one pixel
            (4, 6, 0, 64, 1, 65),        # one pixel in the last word of a row
            (14, 20, 17, 30, 31, 50),    # patch of the box's own size
            (20, 14, 17, 3, 57, 64)]     # spans both words of a row
    tab, off = [], 0
    for ph, pw, y1, x1, y2, x2 in rows:
        tab.append([off, ph, pw, y1, x1, y2, x2, 0]); off += ph * pw
    flat = torch.from_numpy(rng.random(off).astype(np.float32)).to(DEV)
    tabd = torch.from_numpy(np.asarray(tab, np.int32)).to(DEV)
    h, w = out_size
    n, ld = len(rows), ld_words(h, w)
    u8 = torch.full((n, h, w), 7, dtype=torch.uint8, device=DEV)
    words = torch.full((n, ld), -1, dtype=torch.int64, device=DEV)
    t = ctypes.c_float(thresh)
    _lib.call("kg_mask_paste", _lib.ptr(flat), _lib.ptr(tabd), n, in_h, in_w, h, w, t, _lib.ptr(u8), 1,
              _lib.stream_ptr())
    _lib.call("kg_mask_paste_bits", _lib.ptr(flat), _lib.ptr(tabd), n, in_h, in_w, h, w, t, _lib.ptr(words), ctypes.c_long(ld), _lib.stream_ptr())
    ref = u8.cpu().numpy()
    got = words.cpu().numpy().view(np.uint64)
    assert np.array_equal(unpack_host(got, h, w), ref)
    _check_padding(got, h, w)
    if thresh > 0:
        assert not ref[0].any() and not ref[1].any() and ref[4].sum() > ref[5].sum() >= 0 and ref[2:].any()
    else:
        assert ref.all()


def test_from_dense_host_and_device_agree():
    rng = np.random.default_rng(3)
    for n, h, w in ((5, 37, 130), (3, 512, 509), (2, 9, 64), (4, 3, 1)):
        m = rng.random((n, h, w)) > 0.6
        ref = pack_host(m)
        host = BitMasks.from_dense(m.astype(np.uint8), DEV)
        dev8 = BitMasks.from_dense(torch.from_numpy(m.astype(np.uint8) * 3).to(DEV))
        dev32 = BitMasks.from_dense(torch.from_numpy(m.astype(np.float32) * 0.5).to(DEV))
        devb = BitMasks.from_dense(torch.from_numpy(m).to(DEV))
        for b in (host, dev8, dev32, devb):
            assert len(b) == n and (b.h, b.w) == (h, w) and b.words.is_cuda
            assert np.array_equal(b.words_cpu(), ref)
        _check_padding(ref, h, w)
        assert torch.equal(dev8.to_u8(), torch.from_numpy(m.astype(np.uint8)).to(DEV))
        out = dev32.numpy()
        assert out.dtype == np.float32 and np.array_equal(out, m.astype(np.float32))
        assert torch.equal(host.to_f32(), torch.from_numpy(m.astype(np.float32)).to(DEV))
        # row slicing and index arrays
        assert np.array_equal(host[1:].numpy(), m[1:].astype(np.float32))
        idx = np.array([n - 1, 0])
        assert np.array_equal(host[idx].words_cpu(), ref[idx]) and len(host[:0]) == 0
    assert len(BitMasks.from_dense(np.zeros((0, 8, 8), np.uint8), DEV)) == 0


def test_predict_packed_equals_predict(cal):
    model, x = cal[0], cal[1]
    for sizes in (None, MIXED):
        ref = inference.predict(model, x, image_sizes=sizes)
        got = inference.predict(model, x, image_sizes=sizes, packed=True)
        assert len(got) == len(ref) and any(r is not None for r in ref)
        for g, r in zip(got, ref):
            assert (g is None) == (r is None)
            if r is not None:
                assert isinstance(g[0], BitMasks) and g[0].shape == r[0].shape
                assert np.array_equal(g[0].numpy(), r[0]) and g[0].numpy().dtype == r[0].dtype
                assert g[1].dtype == r[1].dtype and np.array_equal(g[1], r[1])
    # an image without detection: None in both forms
    decz = [[t.clone() for t in d] for d in cal[2]]
    for d in decz:
        for t in d:
            t[2].zero_()
    gotz = inference.predict_from_heads(model, decz, cal[3], 256, 256, image_sizes=MIXED, packed=True)
    refz = inference.predict_from_heads(model, decz, cal[3], 256, 256, image_sizes=MIXED)
    assert gotz[2] is None and refz[2] is None
    assert all((g is None) == (r is None) and (r is None or np.array_equal(g[0].numpy(), r[0])) for g, r in zip(gotz, refz))


@pytest.fixture(scope="module")
def population():
    """the rectangles of test_gpu_evalparts.test_iou_table_full_size_vs_oracle (512 x 509, 300 + 300, seed 4), with their boxes, and
    confidences drawn from the same generator afterwards"""
    H, W, n = 512, 509, 300
    rng = np.random.default_rng(4)
    gm = np.zeros((n, H, W), np.uint8); dm = np.zeros((n, H, W), np.uint8)
    gb = np.zeros((n, 4), np.float32); db = np.zeros((n, 5), np.float32)
    for k in range(n):
        h, w = rng.integers(14, 40, 2); y, x = rng.integers(0, H - 48), rng.integers(0, W - 48)
        gm[k, y:y + h, x:x + w] = 1
        sy, sx = rng.integers(-6, 7, 2)
        dm[k, max(y + sy, 0):y + sy + h, max(x + sx, 0):x + sx + w] = 1
        gb[k] = [y, x, y + h, x + w]
        db[k, :4] = [max(y + sy, 0), max(x + sx, 0), y + sy + h, x + sx + w]
    db[:, 4] = rng.random(n)
    return gm, dm, gb, db


def test_bit_counts_are_exact(population):
    gm, dm = population[:2]
    n = len(gm)
    pairs = np.array([(d, g) for d in range(n) for g in range(n) if (abs(d - g) <= 1 or (d * 7 + g) % 97 == 0)], np.int32)
    dense = kev.mask_iou_table(dm, gm, pairs)
    bd, bg = BitMasks.from_dense(dm, DEV), BitMasks.from_dense(torch.from_numpy(gm).to(DEV))
    assert bd.nbytes == n * 4096 * 8                             # 32 KB per mask against 254.5 KB as bytes
    for a, b in ((bd, bg), (bd, gm), (dm, bg)):
        got = kev.mask_iou_table(a, b, pairs)
        assert got.dtype == np.float64 and np.array_equal(got, dense)
    ref = np.array([oev.mask_iou(dm[d], gm[g]) for d, g in pairs[:400]], np.float64)
    assert np.array_equal(dense[:400], ref)
    # areas alone, and the counts behind the table
    aa, ab, inter = kev.bit_counts(bd, bg, pairs)
    assert np.array_equal(aa.cpu().numpy(), dm.reshape(n, -1).sum(1)) and np.array_equal(ab.cpu().numpy(), gm.reshape(n, -1).sum(1))
    assert np.array_equal(inter.cpu().numpy()[:50], [int(np.logical_and(dm[d], gm[g]).sum()) for d, g in pairs[:50]])
    diag = dense[pairs[:, 0] == pairs[:, 1]]
    counts = [int((diag >= t).sum()) for t in THR]
    print("diagonal pairs at or above each threshold", counts)
    assert counts == [210, 179, 151, 112, 77, 49, 30, 14, 2, 1]
    with pytest.raises(_lib.KGLibraryError):
        kev.bit_counts(bd[:5], bg[:5], [[0, 5]])


def _per_threshold(preds, gt_masks, gt_boxes, raw_dets, sizes, input_size):
    """The existing path: for every threshold one pass over the images through eval_parts.seg_evaluation / bbox_evaluation (dense
    float32 masks), aggregated as eval.py:138-179 / :189-234."""
    ds = _DS(gt_masks, gt_boxes)
    seg_ap, seg_iou, dec_ap, seg_tp = [], [], [], []

    def ap_of(all_fp, all_tp, all_scores, npos):
        all_fp = np.asarray(all_fp); all_tp = np.asarray(all_tp); all_scores = np.asarray(all_scores)
        sorted_ind = np.argsort(-all_scores)
        all_fp = np.cumsum(all_fp[sorted_ind]); all_tp = np.cumsum(all_tp[sorted_ind])
        rec = all_tp / float(npos)
        prec = all_tp / np.maximum(all_tp + all_fp, np.finfo(np.float64).eps)
        return kev.voc_ap(rec, prec, use_07_metric=False)
    for thr in THR:
        all_fp, all_tp, all_scores, ovl, npos = [], [], [], [], 0
        for i, p in enumerate(preds):
            if p is None:
                npos += len(gt_boxes[i])
                continue
            fp, tp, all_scores, npos, ovl = kev.seg_evaluation(i, ds, p[0], p[1], all_scores, npos, ovl, thr)
            all_fp.extend(fp); all_tp.extend(tp)
        seg_ap.append(ap_of(all_fp, all_tp, all_scores, npos)); seg_iou.append(np.mean(ovl)); seg_tp.append(int(np.sum(all_tp)))
        all_fp, all_tp, all_scores, npos = [], [], [], 0
        for i, d in enumerate(raw_dets):
            if d is None:
                npos += len(gt_boxes[i])
                continue
            height, width = sizes[i]
            b = np.asarray(d, np.float32).copy()
            b[:, 0] = b[:, 0] / input_size[0] * height; b[:, 1] = b[:, 1] / input_size[1] * width
            b[:, 2] = b[:, 2] / input_size[0] * height; b[:, 3] = b[:, 3] / input_size[1] * width
            fp, tp, all_scores, npos = kev.bbox_evaluation(i, ds, b, all_scores, npos, thr)
            all_fp.extend(fp); all_tp.extend(tp)
        dec_ap.append(ap_of(all_fp, all_tp, all_scores, npos))
    return seg_ap, seg_iou, dec_ap, seg_tp


def _same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def test_evaluator_equals_per_threshold_path(population):
    gm, dm, gb, db = population
    parts = [slice(75 * i, 75 * i + 75) for i in range(4)]
    dense = [[dm[s].astype(np.float32), db[s]] for s in parts]
    dense[3] = None                                              # (the one pair at IoU >= 0.95 is in image 1)
    gt_masks, gt_boxes = [gm[s] for s in parts], [gb[s] for s in parts]
    raw = [None if p is None else p[1] for p in dense]
    seg_ap, seg_iou, dec_ap, seg_tp = _per_threshold(dense, [g.astype(np.float32) for g in gt_masks], gt_boxes, raw, [(512, 509)] * 4, (512, 509))
    print("true positives per threshold", seg_tp)
    assert seg_tp[0] >= 100 and seg_tp[0] > seg_tp[5] and seg_tp[9] >= 1
    for p, g in zip(dense[:3], gt_boxes):
        assert evaluation.box_keep(g, p[1][:, :4]).any()         # the pair table of every image with detections is non-empty
    # the same stream, every mask form: packed / device bytes / float32 host predictions, NumPy / BitMasks / device tensor ground truth
    preds = [[BitMasks.from_dense(dm[parts[0]], DEV), db[parts[0]]], [torch.from_numpy(dm[parts[1]]).to(DEV), db[parts[1]]], dense[2], None]
    gts = [gt_masks[0], BitMasks.from_dense(gt_masks[1], DEV), torch.from_numpy(gt_masks[2]).to(DEV), gt_masks[3]]
    for split in ((4,), (1, 3)):
        ev = evaluation.Evaluator()
        o = 0
        for k in split:
            ev.add_batch(preds[o:o + k], gts[o:o + k], gt_boxes[o:o + k])
            o += k
        for i in range(4):
            ev.add_boxes(raw[i], gt_boxes[i], (512, 509), (512, 509))
        got = ev.summary()
        for t in range(10):
            assert got["seg_ap"][t] == seg_ap[t] and got["seg_iou"][t] == seg_iou[t] and got["dec_ap"][t] == dec_ap[t], (split, t)
    assert seg_ap[0] > seg_ap[5] > seg_ap[9] > 0


def test_evaluate_end_to_end(cal):
    model, x = cal[0], cal[1]
    for sizes in (None, MIXED):
        ref = inference.predict(model, x, image_sizes=sizes)
        assert any(r is not None and len(r[0]) for r in ref)
        hw = [(256, 256)] * 4 if sizes is None else sizes
        gt_masks, gt_boxes = [], []
        for r, (h, w) in zip(ref, hw):
            if r is None:
                gt_masks.append(np.zeros((2, h, w), np.float32)); gt_boxes.append(np.array([[1, 1, 20, 20], [30, 30, 50, 60]], np.float32))
                continue
            keep = [k for k in range(len(r[0])) if k % 3 != 2]                    # every third instance dropped
            g = np.zeros((len(keep), h, w), np.float32)
            g[:, 2:, 2:] = r[0][keep][:, :-2, :-2]                                # the rest shifted by 2 pixels
            gt_masks.append(g); gt_boxes.append((r[1][keep, :4] + 2).astype(np.float32))
        got = evaluation.evaluate(model, [(x, sizes, gt_masks, gt_boxes)])
        with torch.no_grad():
            raw = kpp.detect_batch(list(model.forward_dec(x)[:4]), 0.5)
        seg_ap, seg_iou, dec_ap, seg_tp = _per_threshold(ref, gt_masks, gt_boxes, raw, hw, (256, 256))
        print("sizes", sizes, "true positives per threshold", seg_tp, "seg_ap", np.round(seg_ap, 4), "dec_ap", np.round(dec_ap, 4))
        assert seg_tp[0] >= 1
        for t in range(10):
            assert _same(got["seg_ap"][t], seg_ap[t]) and _same(got["seg_iou"][t], seg_iou[t]) and _same(got["dec_ap"][t], dec_ap[t]), (sizes, t)
