#!/usr/bin/env python
"""Instance results on the device against the host route, on one MI355X -> profiles/instances_bench.json.

Inputs: predict()'s own outputs from the calibrated weights on a seeded random batch (as tools/batch_eval_probe.py), 512^2 and 1024^2,
N = 1 and 8.  Per configuration, in alternating windows of one warmed-up process:
  a  predict(packed=True) alone
  b  predict_instances: a + label maps and tables on the device + one copy of the tables
  c  the host route: a + masks.numpy() + instances.label_map_host per image (what a user had before instances.py)
  d  kg_instance_labels alone (label map + table) over the batch's masks, next to a device-to-device copy that moves the bytes it reads
     (the words) and writes (labels, table), as a ratio
a, b, c end on the host (c's last stage is host NumPy), so they are wall-clock times around a device synchronisation; d is timed with
device events.  Every figure is the median of the repeats with their minimum and maximum.

    python tools/instances_bench.py [--sizes 512,1024] [--ns 1,8] [--reps 5] [--out profiles/instances_bench.json]
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

from kg_instance_segmentation_amd import KGnet, inference, instances  # noqa: E402


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


def host_route(model, x):
    out = []
    for p in inference.predict(model, x, packed=True):
        out.append(None if p is None else instances.label_map_host(p[0].numpy()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--ns", default="1,8")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "instances_bench.json"))
    a = ap.parse_args()
    from oracle import weightgen
    dev = torch.device("cuda", 0)
    model = KGnet.resnet50(pretrained=False)
    model.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    model = model.to(dev).eval()
    res = {"probe": "instances_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps, "host_reps": a.host_reps,
           "units": "ms per call (a, b, c: wall clock around a synchronisation; d: device events)", "configs": []}
    for S in [int(v) for v in a.sizes.split(",")]:
        for n in [int(v) for v in a.ns.split(",")]:
            x = (torch.rand(n, 3, S, S, generator=torch.Generator().manual_seed(n)) - 0.5).to(dev)
            preds = inference.predict(model, x, packed=True)
            got = inference.predict_instances(model, x)
            ref = host_route(model, x)                                # (also the warm-up of all three routes)
            for g, r in zip(got, ref):
                assert (g is None) == (r is None) and (g is None or np.array_equal(g.labels.cpu().numpy(), r))
            parts = [p[0] for p in preds if p is not None]
            masks = instances.join_masks(parts)
            row_start = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
            ta, tb, tc, td, tcopy = [], [], [], [], []
            labels, table = instances.label_map(masks, row_start)
            moved = masks.nbytes + labels.numel() * 4 + table.numel() * 8
            src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            for rep in range(a.reps):
                ta.append(wall(lambda: inference.predict(model, x, packed=True)))
                tb.append(wall(lambda: inference.predict_instances(model, x)))
                if rep < a.host_reps:
                    tc.append(wall(lambda: host_route(model, x)))
                td.append(events(lambda: instances.label_map(masks, row_start)))
                tcopy.append(events(lambda: dst.copy_(src)))
            row = {"size": S, "N": n, "detections_per_image": [0 if p is None else len(p[0]) for p in preds],
                   "a_predict_packed": stat(ta), "b_predict_instances": stat(tb), "c_host_route": stat(tc),
                   "b_minus_a": round(float(np.median(tb) - np.median(ta)), 4), "b_over_c": round(float(np.median(tb) / np.median(tc)), 4),
                   "d_label_map_and_table": stat(td), "d_copy_same_bytes": stat(tcopy), "d_bytes": int(moved),
                   "d_ratio_to_copy": round(float(np.median(td) / np.median(tcopy)), 3),
                   "img_s": {"a": round(n / np.median(ta) * 1e3, 2), "b": round(n / np.median(tb) * 1e3, 2), "c": round(n / np.median(tc) * 1e3, 2)}}
            print(json.dumps(row), file=sys.stderr, flush=True)
            res["configs"].append(row)
            del x, preds, got, ref, masks, labels, table, src, dst
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
