#!/usr/bin/env python
"""Evaluation sweep probe: what the masks cost in each form, and the ten-threshold segmentation evaluation the old way against
Evaluator.add_batch.  Calibrated weights on a random batch at 512^2 (~150-290 detections per image), synthetic ground truth (every
image's own predicted masks, every third dropped, the rest shifted by 2 pixels, as full-size uint8 host arrays), N in {1, 8, 16}.
Per image:

  (a) predict(device_u8=True)                                  ms
  (b) predict(packed=True)                                     ms
  (c) ten eval_parts.seg_evaluation calls (thresholds 0.50 .. 0.95) on the dense u8 device masks, ground-truth upload included -- the
      per-threshold loop of eval.py's run_seg_ap without its ten network passes; image by image, timed over the first --old-images images
  (d) Evaluator.add_batch on the packed masks of the whole batch (host packing + upload of the ground truth included)
  (e) bytes of masks per image as float32 / bytes / bits

Every timed region has a device synchronise on both sides; one warm-up, then the median of --reps repeats with their min .. max.
On a tree without packed masks only (a), (c) and (e) are reported.  Prints one JSON line.

    python tools/eval_sweep_probe.py [--ns 1,8,16] [--reps 5] [--size 512] [--old-images 2]"""
import argparse
import inspect
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from kg_instance_segmentation_amd import KGnet, eval_parts, inference  # noqa: E402

HAS_PACKED = "packed" in inspect.signature(inference.predict).parameters
THR = np.linspace(0.5, 0.95, 10)


class _DS:
    def __init__(self, gm, gb):
        self.gm, self.gb = gm, gb

    def load_annotation(self, index, type):
        return self.gm[index] if type == "mask" else self.gb[index]


def timed(fn, reps):
    """median, min, max in ms of `reps` runs after one warm-up"""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def per_image(t, n):
    return {"median_ms": round(t[0] / n, 3), "min_ms": round(t[1] / n, 3), "max_ms": round(t[2] / n, 3)}


def synthetic_gt(preds):
    gm, gb = [], []
    for p in preds:
        if p is None:
            gm.append(np.zeros((0, 1, 1), np.uint8)); gb.append(np.zeros((0, 4), np.float32))
            continue
        m = p[0].cpu().numpy()
        keep = [k for k in range(len(m)) if k % 3 != 2]
        g = np.zeros((len(keep),) + m.shape[1:], np.uint8)
        g[:, 2:, 2:] = m[keep][:, :-2, :-2]
        gm.append(g); gb.append((p[1][keep, :4] + 2).astype(np.float32))
    return gm, gb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="1,8,16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--old-images", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    from oracle import weightgen
    model = KGnet.resnet50(pretrained=False)
    model.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    model = model.to(dev).eval()
    S = a.size
    res = {"probe": "eval_sweep", "size": S, "reps": a.reps, "packed_masks": HAS_PACKED, "device": torch.cuda.get_device_name(0), "n": {}}
    for n in [int(v) for v in a.ns.split(",")]:
        x = (torch.rand(n, 3, S, S, generator=torch.Generator().manual_seed(n)) - 0.5).to(dev)
        row = {}
        u8 = inference.predict(model, x, device_u8=True)
        nd = [0 if p is None else len(p[0]) for p in u8]
        row["detections_per_image"] = round(float(np.mean(nd)), 1)
        px = S * S
        row["e_mask_bytes_per_image"] = {"float32": int(np.mean(nd) * px * 4), "u8": int(np.mean(nd) * px)}
        row["a_predict_u8"] = per_image(timed(lambda: inference.predict(model, x, device_u8=True), a.reps), n)
        gm, gb = synthetic_gt(u8)
        row["gt_per_image"] = round(float(np.mean([len(g) for g in gm])), 1)
        ds = _DS(gm, gb)
        old = [i for i in range(n) if u8[i] is not None][:a.old_images]
        tps = []

        def old_way():
            tps.clear()
            for thr in THR:
                tp_sum = 0
                for i in old:
                    fp, tp, _, _, _ = eval_parts.seg_evaluation(i, ds, u8[i][0], u8[i][1], [], 0, [], thr)
                    tp_sum += int(tp.sum())
                tps.append(tp_sum)
        row["c_ten_seg_evaluation"] = per_image(timed(old_way, a.reps), max(len(old), 1))
        row["c_images_timed"] = len(old)
        row["c_true_positives_per_threshold"] = list(tps)
        if HAS_PACKED:
            from kg_instance_segmentation_amd import evaluation
            row["b_predict_packed"] = per_image(timed(lambda: inference.predict(model, x, packed=True), a.reps), n)
            packed = inference.predict(model, x, packed=True)
            row["e_mask_bytes_per_image"]["bits"] = int(np.mean([0 if p is None else p[0].nbytes for p in packed]))
            assert all((p is None) == (q is None) and (p is None or torch.equal(p[0].to_u8(), q[0])) for p, q in zip(packed, u8))
            evs = []

            def new_way():
                ev = evaluation.Evaluator()
                ev.add_batch(packed, gm, gb)
                evs.append(ev)
            row["d_evaluator_add_batch"] = per_image(timed(new_way, a.reps), n)
            # the same images through both paths give the same true positives
            ev = evaluation.Evaluator()
            ev.add_batch([packed[i] for i in old], [gm[i] for i in old], [gb[i] for i in old])
            row["d_true_positives_per_threshold"] = [int(np.sum(t)) for t in ev.seg.tp]
            assert row["d_true_positives_per_threshold"] == row["c_true_positives_per_threshold"]
            del packed, evs
        print(n, json.dumps(row), file=sys.stderr, flush=True)
        res["n"][n] = row
        del x, u8, gm, gb
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
