#!/usr/bin/env python
"""Tiled whole-image inference on one MI355X -> profiles/tiling_bench.json.

Inputs: the calibrated weights and seeded uint8 images of 1040 x 1388 and 2048 x 2048 (tile 512, overlap 128, 8 tiles per predict call).
Per image, in alternating windows of one warmed-up process:
  a  predict_tiled (wall clock around a device synchronisation), and its parts by device events placed at the stage boundaries:
     cut | the predict chunks (with the host selection behind them) | the mask gathers and the label launch | stitch | table
  b  a plain loop of predict_instances over the same tiles in the same chunks: what a user had before tiling.py -- overlapping per-tile
     results, nothing joined.  a / b is reported, not asserted.
  c  kg_tile_cut and kg_tile_stitch alone (device events), each next to a device-to-device copy that moves the bytes it reads and
     writes, as a ratio
Every figure is the median of the repeats with their minimum and maximum.

    python tools/tiling_bench.py [--sizes 1040x1388,2048x2048] [--reps 5] [--out profiles/tiling_bench.json]
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

from kg_instance_segmentation_amd import KGnet, inference, tiling  # noqa: E402

STAGES = ("cut", "predict", "labels", "stitch", "table", "end")


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


def staged(model, img, **kw):
    """predict_tiled with a device event at every stage boundary -> (result, {stage: ms})"""
    ev = {}

    def mark(name):
        ev[name] = torch.cuda.Event(enable_timing=True)
        ev[name].record()
    r = tiling.predict_tiled(model, img, stage=mark, **kw)
    torch.cuda.synchronize()
    have = [s for s in STAGES if s in ev]                       # (an image without detections has no label / stitch / table stage)
    return r, {a: ev[a].elapsed_time(ev[b]) for a, b in zip(have[:-1], have[1:])}


def tile_loop(model, x, batch):
    out = []
    for a in range(0, len(x), batch):
        out += inference.predict_instances(model, x[a:a + batch])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1040x1388,2048x2048")
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiling_bench.json"))
    a = ap.parse_args()
    from oracle import weightgen
    dev = torch.device("cuda", 0)
    model = KGnet.resnet50(pretrained=False)
    model.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    model = model.to(dev).eval()
    kw = dict(tile=a.tile, overlap=a.overlap, batch=a.batch)
    res = {"probe": "tiling_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps, "tile": a.tile, "overlap": a.overlap, "batch": a.batch,
           "units": "ms (a, b: wall clock around a synchronisation; stages and c: device events)", "configs": []}
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        img = np.random.default_rng(H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
        p = tiling.plan(H, W, a.tile, a.overlap)
        img_d = torch.from_numpy(img).to(dev)
        x = tiling.cut_tiles(img_d, p)
        r, _ = staged(model, img, **kw)                                    # (also the warm-up of both routes)
        per_tile = tile_loop(model, x, a.batch)
        tile_labels = torch.stack([torch.zeros(a.tile, a.tile, dtype=torch.int32, device=dev) if g is None else g.labels for g in per_tile])
        labels = tiling.stitch(tile_labels, p)
        cut_bytes = img_d.numel() + x.numel() * 4
        stitch_bytes = tile_labels.numel() * 4 + labels.numel() * 4          # (an upper bound of the reads: a pixel outside the image is not read)
        bufs = {k: (torch.empty(b // 2, dtype=torch.uint8, device=dev), torch.empty(b // 2, dtype=torch.uint8, device=dev))
                for k, b in (("cut", cut_bytes), ("stitch", stitch_bytes))}
        ta, tb, tcut, tcutc, tst, tstc = [], [], [], [], [], []
        parts = {s: [] for s in STAGES[:-1]}
        for _ in range(a.reps):
            ta.append(wall(lambda: tiling.predict_tiled(model, img, **kw)))
            tb.append(wall(lambda: tile_loop(model, tiling.cut_tiles(img, p), a.batch)))
            for s, ms in staged(model, img, **kw)[1].items():
                parts[s].append(ms)
            tcut.append(events(lambda: tiling.cut_tiles(img_d, p)))
            tcutc.append(events(lambda: bufs["cut"][1].copy_(bufs["cut"][0])))
            tst.append(events(lambda: tiling.stitch(tile_labels, p)))
            tstc.append(events(lambda: bufs["stitch"][1].copy_(bufs["stitch"][0])))
        row = {"image": [H, W], "tiles": list(p.shape), "detections_per_tile": [0 if g is None else len(g) for g in per_tile], "instances": len(r),
               "a_predict_tiled": stat(ta), "a_stages": {s: stat(v) for s, v in parts.items() if v},
               "b_predict_instances_per_tile": stat(tb), "a_over_b": round(float(np.median(ta) / np.median(tb)), 4),
               "c_cut": stat(tcut), "c_cut_copy_same_bytes": stat(tcutc), "c_cut_bytes": int(cut_bytes),
               "c_cut_ratio_to_copy": round(float(np.median(tcut) / np.median(tcutc)), 3),
               "c_stitch": stat(tst), "c_stitch_copy_same_bytes": stat(tstc), "c_stitch_bytes": int(stitch_bytes),
               "c_stitch_ratio_to_copy": round(float(np.median(tst) / np.median(tstc)), 3)}
        print(json.dumps(row), file=sys.stderr, flush=True)
        res["configs"].append(row)
        del x, img_d, tile_labels, labels, bufs, per_tile, r
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
