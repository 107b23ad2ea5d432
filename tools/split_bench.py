#!/usr/bin/env python
"""Merged instances split on one MI355X -> profiles/split_bench.json.

Inputs: the calibrated weights and seeded uint8 images of 1040 x 1388 and 2048 x 2048 (tile 512, overlap 128, 8 tiles per predict call),
and a synthetic 2048 x 2048 map tiled with dumbbells (two discs of radius 8, 14 apart), because the seeded images hardly ever merge.
Per map, in alternating windows of one warmed-up process:
  a  split.split_instances (wall clock around a synchronisation) against
       host   the map copied back plus split.split_host
       scipy  the route a user has today: the map copied back, scipy.ndimage.distance_transform_edt, ndimage.label of the thresholded core
              and ndimage.watershed_ift on the inverted distance (skimage is not installed; skipped, and said so, where scipy does not
              import).  Its parts are NOT the same parts: it is timed, not compared.
  b  predict_tiled(split=d) against predict_tiled() in the same process (the network's images only)
  c  kg_label_split alone (device events: the entry, which is the copy of the map plus the kernel; the jobs and the rank map already on
     the device), next to that copy alone and to kg_label_measure on the same jobs
and the stated worst cases, on synthetic maps (regrow as wall clock, the entry by device events, regrow_host as wall clock):
  serpentine  ONE one-pixel path that fills a 123 x 123 box, a seed at each end: levels are about pixels / 2
  one_pixel   512 x 512 distinct ids: 262 144 jobs of one pixel each
  seeds_1000  one instance of 120 x 120 pixels with 1000 one-pixel seeds
Every figure is the median of the repeats with their minimum and maximum.

    python tools/split_bench.py [--sizes 1040x1388,2048x2048] [--reps 5] [--distance 3] [--out profiles/split_bench.json]
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

from kg_instance_segmentation_amd import KGnet, instances, labelmetrics, tiling  # noqa: E402
from kg_instance_segmentation_amd import measure as ms  # noqa: E402
from kg_instance_segmentation_amd import split as sp  # noqa: E402

try:
    from scipy import ndimage as ndi  # noqa: E402
except ImportError:                                                    # the scipy route is then not measured
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


def scipy_route(lab_d, d):
    """What a user does today -> the number of parts"""
    lab = lab_d.cpu().numpy()
    fg = lab > 0
    dist = ndi.distance_transform_edt(fg)
    markers, k = ndi.label(dist > d)
    inv = (dist.max() - dist) * (65535.0 / max(float(dist.max()), 1.0))
    parts = ndi.watershed_ift(inv.astype(np.uint16), markers.astype(np.int32))
    return int(len(np.unique(np.where(fg, parts, 0))) - 1)


def host_route(inst, d):
    return sp.split_host(inst.labels.cpu().numpy(), len(inst), d, table=inst.table)


def kernel(lab, n, table, d, dev, reps, inner=10):
    """c: the entry alone on the jobs split would launch"""
    rank, S = sp.seeds(lab, n, d)
    jobs, _ = sp.plan_jobs(S, np.asarray(table)[:, 1:6], None)
    jd = torch.from_numpy(jobs.astype(np.int32)).to(dev)
    mj = torch.from_numpy(np.ascontiguousarray(jobs[:, :6]).astype(np.int32)).to(dev)
    copy_to = torch.empty_like(lab)
    t = {"copy": [], "split": [], "measure": []}
    for _ in range(reps):
        t["copy"].append(events(lambda: copy_to.copy_(lab), inner))
        t["split"].append(events(lambda: sp.regrow_rows(lab, rank, jd), inner))
        if len(jobs):
            t["measure"].append(events(lambda: ms.measure_rows(lab, mj), inner))
    rows = sp.regrow_rows(lab, rank, jd)[1].cpu().numpy()
    h, w = jobs[:, 4] - jobs[:, 2], jobs[:, 5] - jobs[:, 3]
    out = {"jobs": len(jobs), "jobs_that_do_not_fit": int(rows[:, 3].sum()), "box_pixels": int((h * w).sum()), "levels_max": int(rows[:, 2].max(initial=0)),
           "levels_sum": int(rows[:, 2].sum()), "copy_of_the_map": stat(t["copy"]), "label_split_entry": stat(t["split"])}
    out["kernel_alone"] = round(float(np.median(t["split"])) - float(np.median(t["copy"])), 4)
    if t["measure"]:
        out["label_measure_same_jobs"] = stat(t["measure"])
    return out


def dumbbell_map(H, W):
    """The map tiled with dumbbells (r = 8, gap = 14), every second one transposed, each under an id of its own -> (map, n)"""
    yy, xx = np.mgrid[0:21, 0:35]
    one = ((yy - 10) ** 2 + (xx - 10) ** 2 <= 64) | ((yy - 10) ** 2 + (xx - 24) ** 2 <= 64)
    cell = 38
    lab = np.zeros((H, W), np.int32)
    n = 0
    for cy in range(0, H - cell + 1, cell):
        for cx in range(0, W - cell + 1, cell):
            n += 1
            t = one.T if n % 2 else one
            lab[cy + 1:cy + 1 + t.shape[0], cx + 1:cx + 1 + t.shape[1]][t] = n
    return lab, n


def map_instances(lab, n, dev):
    d = torch.from_numpy(lab).to(dev)
    stats = labelmetrics.label_stats(d, n)
    jobs = np.concatenate([np.arange(1, n + 1)[:, None], stats[:, 1:]], 1)
    table = tiling.table_from_labels(d, jobs).cpu().numpy()
    dets = np.concatenate([stats[:, 1:].astype(np.float32), np.ones((n, 1), np.float32)], 1)
    return instances.Instances(d, dets, table, None)


def measure_map(name, r, d, dev, reps, res, model=None, img_d=None, kw=None):
    n = len(r)
    got = sp.split_instances(r, d)
    want = host_route(r, d)
    assert np.array_equal(got.labels.cpu().numpy(), want[0]) and np.array_equal(got.table, want[1]) and np.array_equal(got.parent, want[2])
    row = {"map": name, "image": list(r.labels.shape), "instances": n, "distance": d, "instances_split": int(len(np.unique(got.parent[n:]))),
           "instances_after": len(got)}
    if ndi is not None:
        row["scipy_route_parts"] = scipy_route(r.labels, d)
    t = {k: [] for k in ("device", "host", "scipy", "pred", "pred_split")}
    for _ in range(reps):
        t["device"].append(wall(lambda: sp.split_instances(r, d)))
        t["host"].append(wall(lambda: host_route(r, d)))
        if ndi is not None:
            t["scipy"].append(wall(lambda: scipy_route(r.labels, d)))
        if model is not None:
            t["pred"].append(wall(lambda: tiling.predict_tiled(model, img_d, **kw)))
            t["pred_split"].append(wall(lambda: tiling.predict_tiled(model, img_d, split=d, **kw)))
    med = {k: float(np.median(v)) for k, v in t.items() if v}
    row.update({"a_split_instances": stat(t["device"]), "a_copy_back_plus_split_host": stat(t["host"]),
                "a_host_over_device": round(med["host"] / med["device"], 3)})
    if ndi is not None:
        row.update({"a_scipy_route": stat(t["scipy"]), "a_scipy_over_device": round(med["scipy"] / med["device"], 3)})
    if model is not None:
        row.update({"b_predict_tiled": stat(t["pred"]), "b_predict_tiled_split": stat(t["pred_split"]),
                    "b_split_over_plain": round(med["pred_split"] / med["pred"], 4)})
    row.update({"c_" + k: v for k, v in kernel(r.labels, n, r.table, d, dev, reps).items()})
    print(json.dumps(row), file=sys.stderr, flush=True)
    res["configs"].append(row)


def worst_cases(dev, reps):
    out = {}

    def case(name, lab, seeds, jobs, host_reps):
        d, s = torch.from_numpy(lab).to(dev), torch.from_numpy(seeds).to(dev)
        jd = torch.from_numpy(np.asarray(jobs, np.int32)).to(dev)
        got, rows = sp.regrow(d, s, jobs)
        copy_to = torch.empty_like(d)
        row = {"map": list(lab.shape), "jobs": len(jobs), "levels_max": int(rows[:, 2].max()),
               "wall_regrow": stat([wall(lambda: sp.regrow(d, s, jobs)) for _ in range(reps)]),
               "label_split_entry": stat([events(lambda: sp.regrow_rows(d, s, jd), 3) for _ in range(reps)]),
               "copy_of_the_map": stat([events(lambda: copy_to.copy_(d), 3) for _ in range(reps)])}
        if host_reps:
            seen = []
            row["wall_regrow_host"] = stat([wall(lambda: seen.append(sp.regrow_host(lab, seeds, jobs))) for _ in range(host_reps)])
            assert np.array_equal(seen[-1][0], got.cpu().numpy()) and np.array_equal(seen[-1][1][:, :3], rows[:, :3])
        out[name] = row
        print(name, json.dumps(row), file=sys.stderr, flush=True)
    n = 123
    lab = np.zeros((n, n), np.int32)
    lab[0::2] = 1
    lab[1::4, n - 1] = 1
    lab[3::4, 0] = 1
    seeds = np.zeros_like(lab)
    seeds[0, 0], seeds[n - 1, 0 if (n // 2) % 2 else n - 1] = 1, 2
    case("serpentine_123_two_seeds", lab, seeds, np.array([[0, 1, 0, 0, n, n, 2, 2]]), reps)
    S = 512
    lab = np.arange(1, S * S + 1, dtype=np.int32).reshape(S, S)
    yy, xx = np.mgrid[0:S, 0:S]
    jobs = np.stack([np.zeros(S * S, np.int64), lab.reshape(-1), yy.reshape(-1), xx.reshape(-1), yy.reshape(-1) + 1, xx.reshape(-1) + 1,
                     np.ones(S * S, np.int64), np.zeros(S * S, np.int64)], 1)
    case("one_pixel_512_distinct_jobs", lab, np.ones_like(lab), jobs, 0)
    lab = np.ones((120, 120), np.int32)
    seeds = np.zeros_like(lab)
    rng = np.random.default_rng(0)
    seeds.reshape(-1)[rng.permutation(lab.size)[:1000]] = rng.permutation(1000) + 1
    case("one_instance_1000_seeds", lab, seeds, np.array([[0, 1, 0, 0, 120, 120, 1000, 2]]), reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1040x1388,2048x2048")
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--distance", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_bench.json"))
    a = ap.parse_args()
    from oracle import weightgen
    dev = torch.device("cuda", 0)
    model = KGnet.resnet50(pretrained=False)
    model.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    model = model.to(dev).eval()
    kw = dict(tile=a.tile, overlap=a.overlap, batch=a.batch)
    res = {"probe": "split_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps, "tile": a.tile, "overlap": a.overlap, "batch": a.batch,
           "scipy_route": ("labels.cpu().numpy() + distance_transform_edt + label of the core + watershed_ift (other parts: timed, not compared)"
                           if ndi is not None else "not measured: scipy does not import"),
           "units": "ms (a, b, wall_*: wall clock around a synchronisation; c and the worst cases' entry: device events)",
           "not_measured": ["skimage.segmentation.watershed (not installed)", "more than one image per launch", "connectivity 8"],
           "configs": []}
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        img_d = torch.from_numpy(np.random.default_rng(H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
        r = tiling.predict_tiled(model, img_d, **kw)                          # (also the warm-up)
        measure_map("predict_tiled", r, a.distance, dev, a.reps, res, model, img_d, kw)
        del r, img_d
        torch.cuda.empty_cache()
    lab, n = dumbbell_map(2048, 2048)
    measure_map("dumbbells", map_instances(lab, n, dev), 5, dev, a.reps, res)
    res["worst_cases"] = worst_cases(dev, a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
