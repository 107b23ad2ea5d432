#!/usr/bin/env python
"""Boundary distances on one MI355X -> profiles/boundaries_bench.json.

Inputs: the calibrated weights and seeded uint8 images of 1040 x 1388 and 2048 x 2048 (tile 512, overlap 128, 8 tiles per predict call),
scored against the shifted ground truth tools/labelmetrics_bench.py builds (seeded_gt).  Per image, in alternating windows of one
warmed-up process:
  a  boundaries.pair_distances over the true-positive pairs (IoU > 0.5; wall clock around a synchronisation) against the route a user
     has without it: both maps copied back and, per pair, one scipy.ndimage.distance_transform_edt of each outline on the union box
     (skipped, and said so, where scipy does not import)
  b  LabelEvaluator.add with boundary=True against LabelEvaluator.add without, in the same process
  c  kg_label_border_counts and kg_label_border_d2 alone (device events; the table already on the device, values left there), beside
     kg_label_inter_jobs on the same pairs
and the stated worst cases, on synthetic maps (pair_distances as wall clock, the two entries by device events):
  all_250     ONE pair of 250 x 250 objects with sources="all": 62 500 sources against the rectangles of the target box
  stripes_90  a pair of one-pixel stripes over 90 x 90: every pixel a border pixel, 4050 sources against a list of 4050 targets
  one_pixel   512 x 512 pairs of one pixel each: 524 288 jobs
Every figure is the median of the repeats with their minimum and maximum.

    python tools/boundaries_bench.py [--sizes 1040x1388,2048x2048] [--reps 5] [--out profiles/boundaries_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from kg_instance_segmentation_amd import KGnet, tiling  # noqa: E402
from kg_instance_segmentation_amd import boundaries as bd  # noqa: E402
from kg_instance_segmentation_amd import labelmetrics as lm  # noqa: E402
from labelmetrics_bench import seeded_gt  # noqa: E402

try:
    from scipy import ndimage as ndi  # noqa: E402
except ImportError:                                                    # the host side is then not measured
    ndi = None


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


def scipy_route(a_d, b_d, pairs, sa, sb):
    """What a user does today: both maps copied back; per pair the union box grown by one pixel, the two outlines by binary_erosion, one
    distance transform of each -> the squared distances of both directions, one after another"""
    a, b = a_d.cpu().numpy(), b_d.cpu().numpy()
    H, W = a.shape
    out = []
    for i, j in np.asarray(pairs).tolist():
        y1, x1 = max(min(sa[i - 1, 1], sb[j - 1, 1]) - 1, 0), max(min(sa[i - 1, 2], sb[j - 1, 2]) - 1, 0)
        y2, x2 = min(max(sa[i - 1, 3], sb[j - 1, 3]) + 1, H), min(max(sa[i - 1, 4], sb[j - 1, 4]) + 1, W)
        ma, mb = a[y1:y2, x1:x2] == i, b[y1:y2, x1:x2] == j
        ea, eb = ma & ~ndi.binary_erosion(ma), mb & ~ndi.binary_erosion(mb)       # the array's edge erodes: the ring, or the map's frame
        out.append(np.rint(ndi.distance_transform_edt(~eb)[ea] ** 2).astype(np.int32))
        out.append(np.rint(ndi.distance_transform_edt(~ea)[eb] ** 2).astype(np.int32))
    return out


def kernels(a_d, b_d, pj, mode, reps, inner=10):
    """The two entries by device events on the jobs of pj, the table on the device"""
    cnt = bd.border_counts(a_d, b_d, pj.jobs, mode).cpu().numpy().astype(np.int64)
    table = pj.jobs.astype(np.int64)
    table[:, 12] = np.cumsum(cnt[:, 0]) - cnt[:, 0]
    D = int(cnt[:, 0].sum())
    jd = torch.from_numpy(table.astype(np.int32)).to(a_d.device)
    out = torch.empty(D, dtype=torch.int32, device=a_d.device)
    t = {"counts": [], "d2": []}
    for _ in range(reps):
        t["counts"].append(events(lambda: bd.border_counts(a_d, b_d, jd, mode), inner))
        t["d2"].append(events(lambda: bd.border_d2(a_d, b_d, jd, mode, D, out), inner))
    return {"jobs": len(pj), "sources": D, "targets_listed": int(cnt[:, 1].sum()), "source_target_products": int((cnt[:, 0] * cnt[:, 1]).sum()),
            "label_border_counts": stat(t["counts"]), "label_border_d2": stat(t["d2"])}


def worst_cases(dev, reps):
    out = {}

    def case(name, a, b, pairs, sources, host_reps):
        a_d, b_d = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        n_a, n_b = int(a.max()), int(b.max())
        sa, sb = lm.label_stats_host(a, n_a), lm.label_stats_host(b, n_b)
        run = lambda: bd.pair_distances(a_d, b_d, pairs, sa, sb, sources=sources)  # noqa: E731
        got = run()
        row = {"map": list(a.shape), "pairs": len(pairs), "sources_mode": sources, "wall_pair_distances": stat([wall(run) for _ in range(reps)])}
        if ndi is not None and host_reps and sources == "border":
            seen = []
            row["wall_scipy_route"] = stat([wall(lambda: seen.append(scipy_route(a_d, b_d, pairs, sa, sb))) for _ in range(host_reps)])
            assert all(np.array_equal(v, got.of(k // 2, k % 2)) for k, v in enumerate(seen[-1]))
            row["scipy_route_repeats"] = host_reps
        row.update(kernels(a_d, b_d, bd.pair_jobs(pairs, sa, sb, *a.shape), bd.mode_of(name, sources), reps, inner=3))
        out[name] = row
        print(name, json.dumps(row), file=sys.stderr, flush=True)
    a = np.zeros((260, 262), np.int32)
    a[4:254, 5:255] = 1
    case("all_250_one_pair_sources_all", a, np.roll(a, (3, 2), (0, 1)), [(1, 1)], "all", 0)
    s = np.zeros((92, 92), np.int32)
    s[1:91, 1:91:2] = 1
    case("stripes_90_every_pixel_border", s, np.roll(s, 1, 1), [(1, 1)], "border", reps)
    S = 512
    lab = np.arange(1, S * S + 1, dtype=np.int32).reshape(S, S)
    case("one_pixel_512_distinct_pairs", lab, np.roll(lab, 1, 1), np.stack([np.arange(1, S * S + 1)] * 2, 1), "border", 0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1040x1388,2048x2048")
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boundaries_bench.json"))
    a = ap.parse_args()
    from oracle import weightgen
    dev = torch.device("cuda", 0)
    model = KGnet.resnet50(pretrained=False)
    model.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    model = model.to(dev).eval()
    kw = dict(tile=a.tile, overlap=a.overlap, batch=a.batch)
    res = {"probe": "boundaries_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps, "tile": a.tile, "overlap": a.overlap, "batch": a.batch,
           "host_route": ("both maps copied back + per pair binary_erosion and scipy.ndimage.distance_transform_edt of each outline on the union box"
                          if ndi is not None else "not measured: scipy does not import"),
           "units": "ms (a, b, wall_*: wall clock around a synchronisation; c and the worst cases' entries: device events)",
           "not_measured": ["medpy / MONAI (not installed)", "more than one image per launch", "the host merge and the metrics alone"],
           "configs": []}
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        img_d = torch.from_numpy(np.random.default_rng(H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
        r = tiling.predict_tiled(model, img_d, **kw)                          # (also the warm-up)
        n = n_gt = len(r)
        gt_d = torch.from_numpy(seeded_gt(r.labels.cpu().numpy(), n_gt, H * W)).to(dev)
        sp, sg = np.asarray(r.table)[:, 1:6].astype(np.int64), lm.label_stats(gt_d, n_gt)
        c = lm.LabelEvaluator().add(r, (gt_d, n_gt))
        pairs = c.pairs[c.iou() > 0.5]
        got = bd.pair_distances(r.labels, gt_d, pairs, sp, sg)
        pj = bd.pair_jobs(pairs, sp, sg, H, W)
        row = {"image": [H, W], "instances": n, "pairs_that_meet": len(c.pairs), "true_positive_pairs": len(pairs), "map_bytes": 4 * H * W,
               "mean_hausdorff": float(np.mean(got.hausdorff())) if len(pairs) else None}
        if ndi is not None:
            assert all(np.array_equal(v, got.of(k // 2, k % 2)) for k, v in enumerate(scipy_route(r.labels, gt_d, pairs, sp, sg)))    # the same integers
        inter = np.concatenate([pairs.astype(np.int64), np.maximum(sp[pairs[:, 0] - 1, 1:3], sg[pairs[:, 1] - 1, 1:3]),
                                np.minimum(sp[pairs[:, 0] - 1, 3:5], sg[pairs[:, 1] - 1, 3:5])], 1)
        inter_d = torch.from_numpy(inter.astype(np.int32)).to(dev)
        t = {k: [] for k in ("device", "host", "add", "add_boundary", "inter")}
        for _ in range(a.reps):
            t["add"].append(wall(lambda: lm.LabelEvaluator().add(r, (gt_d, n_gt))))
            t["add_boundary"].append(wall(lambda: lm.LabelEvaluator(boundary=True).add(r, (gt_d, n_gt))))
            t["device"].append(wall(lambda: bd.pair_distances(r.labels, gt_d, pairs, sp, sg)))
            if ndi is not None:
                t["host"].append(wall(lambda: scipy_route(r.labels, gt_d, pairs, sp, sg)))
            t["inter"].append(events(lambda: lm.inter_jobs(r.labels, gt_d, inter_d)))
        med = {k: float(np.median(v)) for k, v in t.items() if v}
        row.update({"a_pair_distances": stat(t["device"]), "b_add": stat(t["add"]), "b_add_boundary": stat(t["add_boundary"]),
                    "b_boundary_over_plain": round(med["add_boundary"] / med["add"], 4)})
        if ndi is not None:
            row.update({"a_scipy_route": stat(t["host"]), "a_scipy_over_device": round(med["host"] / med["device"], 3)})
        row.update({"c_" + key: v for key, v in kernels(r.labels, gt_d, pj, 0, a.reps).items()})
        row["c_label_inter_jobs_same_pairs"] = stat(t["inter"])
        print(json.dumps(row), file=sys.stderr, flush=True)
        res["configs"].append(row)
        del r, img_d, gt_d
        torch.cuda.empty_cache()
    res["worst_cases"] = worst_cases(dev, a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
