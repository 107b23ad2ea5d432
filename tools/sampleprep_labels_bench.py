#!/usr/bin/env python
"""Measures sampleprep's label-map route on the GPU (README "Training samples from label maps").

    python tools/sampleprep_labels_bench.py [--batch 8] [--size 512] [--reps 5] [--out profiles/sampleprep_labels_bench.json]

Configurations: 8 images, 512 x 512 output, sources of 520 x 696 and 1024 x 1024, 37 and 300 instances per image from a seeded
non-overlapping label map (one ellipse per cell of a jittered grid), train-pipeline parameters from a seeded generator.  Per configuration,
in ONE process on the same instances, medians of `--reps` alternating repeats with [min - max]:
  (a) ms per batch, wall clock around a synchronisation, of prepare_batch_full from
        labels   LabelSource on device label maps (boxes from label_stats_device: nothing touches the host);
        labels_boxes_known  the same with the boxes already on the host (stats=: what from_instances passes from the table);
        bits     BitMasks already on the device (the mask route at its best: the masks were made earlier, at no cost counted here);
        today    what a user with a device label map does without this route: the map copied back, dense labels == id on the host,
                 BitMasks.from_dense (packed on the host), the words uploaded, prepare_batch_full;
  (b) ms of the single launches, device events: kg_sp_warp_labels with the instances' boxes, with every box the whole map (the worst case:
      every pixel is loaded for every instance) and kg_sp_warp_masks on bit-packed and on byte masks, beside a device fill (torch.zeros)
      and a device-to-device copy of the bytes `out` holds.
A difference counts only where it lies outside the repeats' own spread.  There is no CPU fallback: without a GPU the tool fails."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from kg_instance_segmentation_amd import _lib, labelmetrics, sampleprep
from kg_instance_segmentation_amd.bitmasks import BitMasks


def grid_map(rs, h, w, n):
    """int32 [h, w] with ids 1 .. n, one ellipse per cell of a jittered grid: the instances never overlap"""
    g = int(np.ceil(np.sqrt(n)))
    ch, cw = h / g, w / g
    lab = np.zeros((h, w), np.int32)
    yy, xx = np.mgrid[0:h, 0:w]
    for v in range(1, n + 1):
        gy, gx = divmod(v - 1, g)
        ry, rx = ch * rs.uniform(0.25, 0.45), cw * rs.uniform(0.25, 0.45)
        cy, cx = (gy + 0.5) * ch + rs.uniform(-0.04, 0.04) * ch, (gx + 0.5) * cw + rs.uniform(-0.04, 0.04) * cw
        y0, y1, x0, x1 = max(int(cy - ry) - 1, 0), min(int(cy + ry) + 2, h), max(int(cx - rx) - 1, 0), min(int(cx + rx) + 2, w)
        sel = ((yy[y0:y1, x0:x1] - cy) / ry) ** 2 + ((xx[y0:y1, x0:x1] - cx) / rx) ** 2 <= 1
        lab[y0:y1, x0:x1][sel] = v
    return lab


def stat(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def apart(a, b):
    """the two spreads do not touch"""
    return a["max"] < b["min"] or b["max"] < a["min"]


def one_config(dev, N, S, h, w, n, reps):
    rs = np.random.RandomState(1000 * n + h)
    labs = [grid_map(rs, h, w, n) for _ in range(N)]
    images = [torch.from_numpy(rs.randint(0, 256, (h, w, 3)).astype(np.uint8)).to(dev) for _ in range(N)]
    params = [sampleprep.draw_train_params(h, w, rs) for _ in range(N)]
    dlabs = [torch.from_numpy(lab).to(dev) for lab in labs]
    ids = np.arange(1, n + 1)
    bits = [BitMasks.from_dense((lab[None] == ids[:, None, None]).astype(np.uint8), dev) for lab in labs]
    full = np.concatenate([ids[:, None], np.tile([[0, 0, h, w]], (n, 1))], 1)

    def labels():
        return sampleprep.prepare_batch_full(images, [sampleprep.LabelSource(d, n=n) for d in dlabs], params, S, S, dev)

    def worst():
        return sampleprep.prepare_batch_full(images, [sampleprep.LabelSource(d, jobs=full) for d in dlabs], params, S, S, dev)

    def from_bits():
        return sampleprep.prepare_batch_full(images, bits, params, S, S, dev)

    def today():
        masks = []
        for d in dlabs:
            lab = d.cpu().numpy()
            masks.append(BitMasks.from_dense(lab[None] == ids[:, None, None], dev))
        return sampleprep.prepare_batch_full(images, masks, params, S, S, dev)

    stats = [labelmetrics.label_stats_host(lab, n) for lab in labs]

    def labels_boxes_known():
        return sampleprep.prepare_batch_full(images, [sampleprep.LabelSource(d, n=n, stats=s) for d, s in zip(dlabs, stats)], params, S, S, dev)

    routes = {"labels": labels, "labels_boxes_known": labels_boxes_known, "bits": from_bits, "today": today}
    a, b = labels(), from_bits()                                                 # warm-up, and the routes agree
    assert all(torch.equal(x, y) for x, y in zip(a.warped, b.warped)) and all(torch.equal(x, y) for x, y in zip(a.gt, b.gt))
    torch.cuda.synchronize()
    wall = {k: [] for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall[k].append(1e3 * (time.perf_counter() - t0))

    # (b) the single launches, device events around the library call
    byte_masks = [torch.from_numpy((lab[None] == ids[:, None, None]).astype(np.uint8)).to(dev) for lab in labs] if n * h * w * N <= 2 ** 31 else None

    def from_bytes():
        return sampleprep.prepare_batch_full(images, byte_masks, params, S, S, dev)

    launches = {"warp_labels": (labels, "kg_sp_warp_labels"), "warp_labels_full_boxes": (worst, "kg_sp_warp_labels"),
                "warp_masks_bits": (from_bits, "kg_sp_warp_masks")}
    if byte_masks is not None:
        launches["warp_masks_bytes"] = (from_bytes, "kg_sp_warp_masks")
    real_call, hit = _lib.call, []

    def timed_call(name, *args, **kw):
        if name != hit[0]:
            return real_call(name, *args, **kw)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); real_call(name, *args, **kw); e1.record()
        hit.append((e0, e1))
    nbytes = N * n * S * S
    src_t = torch.empty(nbytes, dtype=torch.uint8, device=dev).random_(0, 2)
    dst_t = torch.empty_like(src_t)
    kern = {k: [] for k in list(launches) + ["fill_torch_zeros", "d2d_copy"]}
    sampleprep._lib.call = timed_call
    try:
        for fn, _ in launches.values():
            hit[:] = ["-"]
            fn()                                                                 # warm-up of every launch
        for _ in range(reps):
            for k, (fn, name) in launches.items():
                hit[:] = [name]
                fn()
                torch.cuda.synchronize()
                kern[k].append(hit[1][0].elapsed_time(hit[1][1]))
            for k in ("fill_torch_zeros", "d2d_copy"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if k == "d2d_copy":
                    dst_t.copy_(src_t)
                else:
                    z = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
                e1.record()
                torch.cuda.synchronize()
                kern[k].append(e0.elapsed_time(e1))
                z = None
    finally:
        sampleprep._lib.call = real_call
    wall_s = {k: stat(v) for k, v in wall.items()}
    kern_s = {k: stat(v) for k, v in kern.items()}
    for k, v in kern_s.items():
        v["GB_per_s_over_out_bytes"] = nbytes / v["median"] / 1e6
    return {"source": [h, w], "instances_per_image": n, "out_bytes": nbytes,
            "prepare_batch_full_ms": wall_s,
            "labels_vs_bits_outside_spread": apart(wall_s["labels"], wall_s["bits"]),
            "labels_vs_today_outside_spread": apart(wall_s["labels"], wall_s["today"]),
            "single_launch_ms": kern_s,
            "warp_labels_vs_warp_masks_bits_outside_spread": apart(kern_s["warp_labels"], kern_s["warp_masks_bits"]),
            "warp_labels_vs_fill_outside_spread": apart(kern_s["warp_labels"], kern_s["fill_torch_zeros"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sampleprep_labels_bench: no GPU (this tool never falls back to the CPU)")
    dev = torch.device("cuda:0")
    res = {"config": {"batch": args.batch, "size": args.size, "reps": args.reps, "device": torch.cuda.get_device_name(0),
                      "method": "medians of alternating repeats with min and max; wall clock around a synchronisation for the routes, "
                                "device events around the library call for the single launches"},
           "cases": []}
    for (h, w) in ((520, 696), (1024, 1024)):
        for n in (37, 300):
            c = one_config(dev, args.batch, args.size, h, w, n, args.reps)
            print(json.dumps(c), flush=True)
            res["cases"].append(c)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
