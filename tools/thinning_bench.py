#!/usr/bin/env python
"""Instance midlines on one MI355X -> profiles/thinning_bench.json.

Inputs: the calibrated weights and seeded uint8 images of 1040 x 1388 and 2048 x 2048 (tile 512, overlap 128, 8 tiles per predict call).
Per map, in alternating windows of one warmed-up process:
  a  thinning.thin_instances (wall clock around a synchronisation) against the route a user has today with this project alone: the map
     copied back plus thinning.thin_host per id (midlines_host).  skimage.morphology.thin and cv2.ximgproc.thinning are not installed:
     neither was compared.
  b  predict_tiled(thin=True) against predict_tiled() in the same process
  c  kg_label_thin alone (device events over ten back-to-back calls: the entry, which is the clear of the map plus the kernel; the jobs
     already on the device), next to kg_label_measure on the same jobs, to a device-to-device copy of the map and to the clear alone
and the stated worst cases, as they come, on synthetic maps (thin as wall clock, the entry by device events, midlines_host as wall clock):
  square_250    ONE full 250 x 250 square: about 125 passes of one workgroup
  serpentine    ONE one-pixel path that fills a 123 x 123 box: a fixed point, one pass that deletes a corner or nothing
  one_pixel     512 x 512 distinct ids: 262 144 jobs of one pixel each
  crosses       a 2048 x 2048 sheet of crosses 40 pixels wide with arms 7 thick, each under an id of its own: process-like objects
Every figure is the median of the repeats with their minimum and maximum.

    python tools/thinning_bench.py [--sizes 1040x1388,2048x2048] [--reps 5] [--out profiles/thinning_bench.json]
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

from kg_instance_segmentation_amd import KGnet, _labelmaps, instances, labelmetrics, tiling  # noqa: E402
from kg_instance_segmentation_amd import measure as ms  # noqa: E402
from kg_instance_segmentation_amd import thinning as th  # noqa: E402


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


def host_copy(r):
    if isinstance(r, tiling.TiledInstances):
        return tiling.TiledInstances(r.labels.cpu().numpy(), r.dets, r.table, r.tile, r.origin, r.tile_masks)
    return instances.Instances(r.labels.cpu().numpy(), r.dets, r.table, r.masks)


def kernel(lab, jobs, dev, reps, inner=10):
    """c: the entry alone on the jobs thin_instances would launch"""
    jd = torch.from_numpy(np.ascontiguousarray(jobs, np.int32)).to(dev)
    other = torch.empty_like(lab)
    t = {"copy": [], "clear": [], "thin": [], "measure": []}
    for _ in range(reps):
        t["copy"].append(events(lambda: other.copy_(lab), inner))
        t["clear"].append(events(lambda: other.zero_(), inner))
        t["thin"].append(events(lambda: th.thin_rows(lab, jd, out=other), inner))
        if len(jobs):
            t["measure"].append(events(lambda: ms.measure_rows(lab, jd), inner))
    rows = th.thin_rows(lab, jd)[1].cpu().numpy()
    h, w = jobs[:, 4] - jobs[:, 2], jobs[:, 5] - jobs[:, 3]
    out = {"jobs": len(jobs), "jobs_that_do_not_fit": int(rows[:, 8].sum()), "box_pixels": int((h * w).sum()), "passes_max": int(rows[:, 7].max(initial=0)),
           "passes_sum": int(rows[:, 7].sum()), "copy_of_the_map": stat(t["copy"]), "clear_of_the_map": stat(t["clear"]), "label_thin_entry": stat(t["thin"])}
    out["kernel_alone"] = round(float(np.median(t["thin"])) - float(np.median(t["clear"])), 4)
    if t["measure"]:
        out["label_measure_same_jobs"] = stat(t["measure"])
    return out


def map_instances(lab, n, dev):
    d = torch.from_numpy(lab).to(dev)
    stats = labelmetrics.label_stats(d, n)
    jobs = np.concatenate([np.arange(1, n + 1)[:, None], stats[:, 1:]], 1)
    table = tiling.table_from_labels(d, jobs).cpu().numpy()
    dets = np.concatenate([stats[:, 1:].astype(np.float32), np.ones((n, 1), np.float32)], 1)
    return instances.Instances(d, dets, table, None)


def measure_map(name, r, dev, reps, res, model=None, img_d=None, kw=None):
    n = len(r)
    got = th.thin_instances(r)
    want = th.thin_instances(host_copy(r))
    assert got == want and np.array_equal(got.skel.cpu().numpy(), want.skel)
    row = {"map": name, "image": list(r.labels.shape), "instances": n, "midline_pixels": int(got.pixels().sum()), "ends": int(got.ends().sum()),
           "junctions": int(got.junctions().sum()), "length_sum": round(float(got.lengths().sum()), 3)}
    t = {k: [] for k in ("device", "host", "pred", "pred_thin")}
    for _ in range(reps):
        t["device"].append(wall(lambda: th.thin_instances(r)))
        t["host"].append(wall(lambda: th.thin_instances(host_copy(r))))
        if model is not None:
            t["pred"].append(wall(lambda: tiling.predict_tiled(model, img_d, **kw)))
            t["pred_thin"].append(wall(lambda: tiling.predict_tiled(model, img_d, thin=True, **kw)))
    med = {k: float(np.median(v)) for k, v in t.items() if v}
    row.update({"a_thin_instances": stat(t["device"]), "a_copy_back_plus_thin_host": stat(t["host"]), "a_host_over_device": round(med["host"] / med["device"], 3)})
    if model is not None:
        row.update({"b_predict_tiled": stat(t["pred"]), "b_predict_tiled_thin": stat(t["pred_thin"]),
                    "b_thin_over_plain": round(med["pred_thin"] / med["pred"], 4)})
    H, W = r.labels.shape
    row.update({"c_" + k: v for k, v in kernel(r.labels, _labelmaps.instance_jobs(r, 0, 0, H, W), dev, reps).items()})
    print(json.dumps(row), file=sys.stderr, flush=True)
    res["configs"].append(row)


def crosses_map(H, W, size=40, arm=7):
    one = np.zeros((size, size), bool)
    a = (size - arm) // 2
    one[a:a + arm, :] = True
    one[:, a:a + arm] = True
    cell = size + 4
    lab = np.zeros((H, W), np.int32)
    n = 0
    for cy in range(0, H - cell + 1, cell):
        for cx in range(0, W - cell + 1, cell):
            n += 1
            lab[cy + 2:cy + 2 + size, cx + 2:cx + 2 + size][one] = n
    return lab, n


def worst_cases(dev, reps):
    out = {}

    def case(name, lab, jobs, host_reps):
        jobs = np.asarray(jobs, np.int64)
        d = torch.from_numpy(lab).to(dev)
        jd = torch.from_numpy(jobs.astype(np.int32)).to(dev)
        got, mid = th.thin(d, jobs=jobs)
        other = torch.empty_like(d)
        row = {"map": list(lab.shape), "jobs": len(jobs), "passes_max": int(mid.rows[:, 7].max()), "midline_pixels": int(mid.rows[:, 1].sum()),
               "wall_thin": stat([wall(lambda: th.thin(d, jobs=jobs)) for _ in range(reps)]),
               "label_thin_entry": stat([events(lambda: th.thin_rows(d, jd, out=other), 3) for _ in range(reps)]),
               "copy_of_the_map": stat([events(lambda: other.copy_(d), 3) for _ in range(reps)])}
        if host_reps:
            seen = []
            row["wall_midlines_host"] = stat([wall(lambda: seen.append(th.midlines_host(lab, jobs))) for _ in range(host_reps)])
            assert np.array_equal(seen[-1][0], got.cpu().numpy()) and np.array_equal(seen[-1][1].rows[:, :8], mid.rows[:, :8])
        out[name] = row
        print(name, json.dumps(row), file=sys.stderr, flush=True)
    lab = np.zeros((256, 256), np.int32)
    lab[3:253, 3:253] = 1
    case("square_250", lab, [[0, 1, 3, 3, 253, 253]], reps)
    n = 123
    lab = np.zeros((n, n), np.int32)
    lab[0::2] = 1
    lab[1::4, n - 1] = 1
    lab[3::4, 0] = 1
    case("serpentine_123", lab, [[0, 1, 0, 0, n, n]], reps)
    S = 512
    lab = np.arange(1, S * S + 1, dtype=np.int32).reshape(S, S)
    yy, xx = np.mgrid[0:S, 0:S]
    jobs = np.stack([np.zeros(S * S, np.int64), lab.reshape(-1), yy.reshape(-1), xx.reshape(-1), yy.reshape(-1) + 1, xx.reshape(-1) + 1], 1)
    case("one_pixel_512_distinct_jobs", lab, jobs, 0)
    lab, k = crosses_map(2048, 2048)
    d = torch.from_numpy(lab).to(dev)
    stats = labelmetrics.label_stats(d, k)
    case("crosses_40_wide", lab, _labelmaps.jobs_from_stats(stats), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1040x1388,2048x2048")
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thinning_bench.json"))
    a = ap.parse_args()
    from oracle import weightgen
    dev = torch.device("cuda", 0)
    model = KGnet.resnet50(pretrained=False)
    model.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    model = model.to(dev).eval()
    kw = dict(tile=a.tile, overlap=a.overlap, batch=a.batch)
    res = {"probe": "thinning_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps, "tile": a.tile, "overlap": a.overlap, "batch": a.batch,
           "host_route": "labels.cpu().numpy() + thinning.thin_host per id (midlines_host)",
           "units": "ms (a, b, wall_*: wall clock around a synchronisation; c and the worst cases' entry: device events)",
           "not_measured": ["skimage.morphology.thin (not installed)", "cv2.ximgproc.thinning (not installed)", "more than one image per launch",
                            "max_passes > 0", "a box that does not fit (the host route of thin)"],
           "configs": []}
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        img_d = torch.from_numpy(np.random.default_rng(H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
        r = tiling.predict_tiled(model, img_d, **kw)                          # (also the warm-up)
        measure_map("predict_tiled", r, dev, a.reps, res, model, img_d, kw)
        del r, img_d
        torch.cuda.empty_cache()
    res["worst_cases"] = worst_cases(dev, a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
