#!/usr/bin/env python
"""Label-map evaluation on one MI355X -> profiles/labelmetrics_bench.json.

Inputs: the calibrated weights and seeded uint8 images of 1040 x 1388 and 2048 x 2048 (tile 512, overlap 128, 8 tiles per predict call); the
ground truth is a seeded label map of about as many instances as predict_tiled finds (its own instances moved by two pixels, every third
replaced by a rectangle).  Per image, in alternating windows of one warmed-up process:
  a  LabelEvaluator.add on the predict_tiled result with the ground truth already on the device (wall clock around a synchronisation),
     against the host route -- both maps copied back, contingency_host and the same metrics -- and as a share of predict_tiled's own time
  b  kg_label_stats and kg_label_inter_jobs alone (device events), each next to a device-to-device copy that moves the bytes it reads,
     as a ratio; the jobs are those of the image's own contingency
  c  kg_label_stats on a map that is ONE id: its worst case, every run head adds to one address
Every figure is the median of the repeats with their minimum and maximum.

    python tools/labelmetrics_bench.py [--sizes 1040x1388,2048x2048] [--reps 5] [--out profiles/labelmetrics_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from kg_instance_segmentation_amd import KGnet, tiling  # noqa: E402
from kg_instance_segmentation_amd import labelmetrics as lm  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def events(fn, inner=10):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def stat(ts):
    return {"median": round(float(np.median(ts)), 4), "min": round(float(np.min(ts)), 4), "max": round(float(np.max(ts)), 4)}


def seeded_gt(lab, n, seed):
    """the prediction's own instances moved by two pixels, every third id replaced by a seeded rectangle: int32 [H, W], ids 1 .. n"""
    rng = np.random.default_rng(seed)
    H, W = lab.shape
    gt = np.roll(lab, (2, 2), (0, 1)).astype(np.int32)
    gt[:2] = 0
    gt[:, :2] = 0
    gt[(gt % 3) == 0] = 0
    for i in range(3, n + 1, 3):
        y, x = rng.integers(0, H - 40), rng.integers(0, W - 40)
        gt[y:y + rng.integers(8, 40), x:x + rng.integers(8, 40)] = i
    return gt


def host_route(labels, gt_d, n, n_gt, conf):
    ev = lm.LabelEvaluator()
    ev.add((labels.cpu().numpy(), n), (gt_d.cpu().numpy(), n_gt), conf)
    return ev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1040x1388,2048x2048")
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "labelmetrics_bench.json"))
    a = ap.parse_args()
    from oracle import weightgen
    dev = torch.device("cuda", 0)
    model = KGnet.resnet50(pretrained=False)
    model.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    model = model.to(dev).eval()
    kw = dict(tile=a.tile, overlap=a.overlap, batch=a.batch)
    res = {"probe": "labelmetrics_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps, "tile": a.tile, "overlap": a.overlap, "batch": a.batch,
           "units": "ms (a: wall clock around a synchronisation; b, c: device events)", "configs": []}
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        img = np.random.default_rng(H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
        r = tiling.predict_tiled(model, img, **kw)                           # (also the warm-up)
        n = n_gt = len(r)
        gt = seeded_gt(r.labels.cpu().numpy(), n_gt, H * W)
        gt_d = torch.from_numpy(gt).to(dev)
        conf = r.dets[:, 4]
        c = lm.LabelEvaluator().add(r, (gt_d, n_gt))
        assert c == lm.LabelEvaluator().add((r.labels.cpu().numpy(), n), (gt, n_gt), conf)        # both routes count the same
        sp, sg = r.table[:, 1:6], lm.label_stats(gt_d, n_gt)
        pieces, _ = lm.split_jobs(lm.candidate_pairs(sp, sg))
        jobs_d = torch.from_numpy(pieces).to(dev)
        box_pixels = int(((pieces[:, 4] - pieces[:, 2]).astype(np.int64) * (pieces[:, 5] - pieces[:, 3])).sum())
        one = torch.ones(H, W, dtype=torch.int32, device=dev)
        stats_bytes, inter_bytes = H * W * 4, 2 * 4 * box_pixels + pieces.nbytes
        bufs = {k: (torch.empty(b, dtype=torch.uint8, device=dev), torch.empty(b, dtype=torch.uint8, device=dev))
                for k, b in (("stats", stats_bytes), ("inter", inter_bytes))}
        t_pred, t_add, t_host, t_stats, t_statsc, t_inter, t_interc, t_one = [], [], [], [], [], [], [], []
        for _ in range(a.reps):
            t_pred.append(wall(lambda: tiling.predict_tiled(model, img, **kw)))
            t_add.append(wall(lambda: lm.LabelEvaluator().add(r, (gt_d, n_gt))))
            t_host.append(wall(lambda: host_route(r.labels, gt_d, n, n_gt, conf)))
            t_stats.append(events(lambda: lm.label_stats_device(gt_d, n_gt)))
            t_statsc.append(events(lambda: bufs["stats"][1].copy_(bufs["stats"][0])))
            t_inter.append(events(lambda: lm.inter_jobs(r.labels, gt_d, jobs_d)))
            t_interc.append(events(lambda: bufs["inter"][1].copy_(bufs["inter"][0])))
            t_one.append(events(lambda: lm.label_stats_device(one, n_gt)))
        row = {"image": [H, W], "instances": n, "gt_instances": n_gt, "pairs_that_meet": len(c.pairs), "jobs": len(pieces), "job_box_pixels": box_pixels,
               "a_predict_tiled": stat(t_pred), "a_add_device": stat(t_add), "a_add_host_route": stat(t_host),
               "a_host_over_device": round(float(np.median(t_host) / np.median(t_add)), 3),
               "a_add_share_of_predict_tiled": round(float(np.median(t_add) / np.median(t_pred)), 5),
               "b_label_stats": stat(t_stats), "b_label_stats_copy_same_bytes": stat(t_statsc), "b_label_stats_bytes": int(stats_bytes),
               "b_label_stats_ratio_to_copy": round(float(np.median(t_stats) / np.median(t_statsc)), 3),
               "b_inter_jobs": stat(t_inter), "b_inter_jobs_copy_same_bytes": stat(t_interc), "b_inter_jobs_bytes": int(inter_bytes),
               "b_inter_jobs_ratio_to_copy": round(float(np.median(t_inter) / np.median(t_interc)), 3),
               "c_label_stats_single_id": stat(t_one), "c_single_id_over_seeded": round(float(np.median(t_one) / np.median(t_stats)), 3)}
        print(json.dumps(row), file=sys.stderr, flush=True)
        res["configs"].append(row)
        del gt_d, jobs_d, one, bufs, r
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
