#!/usr/bin/env python
"""Instance outlines on one MI355X -> profiles/contours_bench.json.

Inputs: the calibrated weights and seeded uint8 images of 1040 x 1388 and 2048 x 2048 (tile 512, overlap 128, 8 tiles per predict call).
Per image, in alternating windows of one warmed-up process:
  a  contours.contours_instances on the predict_tiled result (wall clock around a synchronisation) against the route a user has without
     it: labels.cpu().numpy() followed by a per-id tracer over the ids 1 .. n.  cv2 and skimage are not installed where this was
     measured, so the per-id tracer is contours.contours_host (NumPy masks, a Python loop per crack)
  b  predict_tiled(contours=True) against predict_tiled() in the same process
  c  kg_label_contour_counts and kg_label_contours alone (device events; tables already on the device, rows left there), next to a
     device-to-device copy of the map
and the stated worst cases, on synthetic maps (contours as wall clock, both kernels by device events):
  comb          250 x 250, ONE ring of 62 504 cracks that one lane walks
  diamond       251 pixels: the radius-10 diamond (221 pixels) with 30 more along its rim, where most candidates walk far before they
                abort
  random        250 x 250 Bernoulli(0.6) mask, one job
  checkerboard  512 x 512 distinct ids: 262 144 jobs of one pixel each
Every figure is the median of the repeats with their minimum and maximum.

    python tools/contours_bench.py [--sizes 1040x1388,2048x2048] [--reps 5] [--out profiles/contours_bench.json]
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
from kg_instance_segmentation_amd import contours as ct  # noqa: E402
from kg_instance_segmentation_amd._labelmaps import instance_jobs  # noqa: E402


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


def device_tables(lab, jobs, dev):
    """The two job tables of the raw entries, on the device, with R and V"""
    cnt = ct.contour_counts(lab, jobs).cpu().numpy()
    table = np.concatenate([np.asarray(jobs, np.int64), np.cumsum(cnt[:, :2], 0) - cnt[:, :2]], 1)
    return (torch.from_numpy(np.ascontiguousarray(jobs, np.int32)).to(dev), torch.from_numpy(table.astype(np.int32)).to(dev),
            int(cnt[:, 0].sum()), int(cnt[:, 1].sum()), int(cnt[:, 2].sum()))


def kernels(lab, jobs, dev, reps, inner=10):
    cnt_table, row_table, R, V, cracks = device_tables(lab, jobs, dev)
    rings, verts = torch.empty(R, 4, dtype=torch.int64, device=dev), torch.empty(V, 2, dtype=torch.int32, device=dev)
    copy_to = torch.empty_like(lab)
    t = {"copy": [], "counts": [], "rows": []}
    for _ in range(reps):
        t["copy"].append(events(lambda: copy_to.copy_(lab), inner))
        t["counts"].append(events(lambda: ct.contour_counts(lab, cnt_table), inner))
        t["rows"].append(events(lambda: ct.contour_rows(lab, row_table, R, V, rings, verts), inner))
    med = {k: float(np.median(v)) for k, v in t.items()}
    return {"jobs": len(cnt_table), "rings": R, "vertices": V, "cracks": cracks, "copy_of_the_map": stat(t["copy"]),
            "label_contour_counts": stat(t["counts"]), "label_contours": stat(t["rows"]),
            "counts_to_map_copy": round(med["counts"] / med["copy"], 3), "contours_to_map_copy": round(med["rows"] / med["copy"], 3)}


def diamond(pixels):
    """The largest diamond with at most `pixels` pixels, plus the pixels that are missing, added in raster order along its rim"""
    r = 0
    while 2 * (r + 1) * (r + 2) + 1 <= pixels:
        r += 1
    yy, xx = np.mgrid[-r - 1:r + 2, -r - 1:r + 2]
    dist = np.abs(yy) + np.abs(xx)
    lab = (dist <= r).astype(np.int32)
    rim = np.flatnonzero((dist == r + 1).reshape(-1))[:pixels - int(lab.sum())]
    lab.reshape(-1)[rim] = 1
    return lab


def worst_cases(dev, reps):
    out = {}

    def case(name, lab, jobs, host_reps):
        d = torch.from_numpy(lab).to(dev)
        got = ct.contours(d, jobs=jobs)
        host, traced = [], []
        for _ in range(host_reps):
            host.append(wall(lambda: traced.append(ct.contours_host(d.cpu().numpy(), jobs))))
            assert traced.pop() == got                                # both routes give the same rings
        out[name] = {"map": list(lab.shape), "wall_contours": stat([wall(lambda: ct.contours(d, jobs=jobs)) for _ in range(reps)]),
                     "wall_host_route": stat(host), "host_route_repeats": host_reps,
                     **kernels(d, jobs, dev, reps, inner=3)}
        print(name, json.dumps(out[name]), file=sys.stderr, flush=True)
    S = 250
    lab = np.zeros((S, S), np.int32)
    lab[:, ::2] = 1
    lab[0, :] = 1
    case("comb_250_one_ring", lab, np.array([[0, 1, 0, 0, S, S]]), reps)
    lab = np.pad(diamond(251), 1)
    assert lab.sum() == 251
    case("diamond_251_pixels", lab, np.array([[0, 1, 0, 0, *lab.shape]]), reps)
    lab = (np.random.default_rng(0).random((S, S)) < 0.6).astype(np.int32)
    case("random_250_bernoulli_0.6", lab, np.array([[0, 1, 0, 0, S, S]]), reps)
    S = 512
    lab = np.arange(1, S * S + 1, dtype=np.int32).reshape(S, S)
    yy, xx = np.mgrid[0:S, 0:S]
    jobs = np.stack([np.zeros(S * S, np.int64), lab.reshape(-1), yy.reshape(-1), xx.reshape(-1), yy.reshape(-1) + 1, xx.reshape(-1) + 1], 1)
    case("checkerboard_512_distinct_one_pixel_jobs", lab, jobs, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1040x1388,2048x2048")
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contours_bench.json"))
    a = ap.parse_args()
    from oracle import weightgen
    dev = torch.device("cuda", 0)
    model = KGnet.resnet50(pretrained=False)
    model.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    model = model.to(dev).eval()
    kw = dict(tile=a.tile, overlap=a.overlap, batch=a.batch)
    res = {"probe": "contours_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps, "tile": a.tile, "overlap": a.overlap, "batch": a.batch,
           "host_route": "labels.cpu().numpy() + contours.contours_host (cv2 / skimage not installed)",
           "units": "ms (a, b, wall_*: wall clock around a synchronisation; c and the worst cases' kernels: device events)", "configs": []}
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        img_d = torch.from_numpy(np.random.default_rng(H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
        r = tiling.predict_tiled(model, img_d, **kw)                          # (also the warm-up)
        n = len(r)
        jobs = instance_jobs(r, 0, 0, H, W)

        def host_route():
            return ct.contours_host(r.labels.cpu().numpy(), jobs)
        got = ct.contours_instances(r)
        assert got == host_route() and np.array_equal(got.areas(), np.asarray(r.table)[:, 1])     # both routes give the same rings
        row = {"image": [H, W], "instances": n, "map_bytes": 4 * H * W}
        t = {k: [] for k in ("device", "host", "pred", "pred_contours")}
        for _ in range(a.reps):
            t["pred"].append(wall(lambda: tiling.predict_tiled(model, img_d, **kw)))
            t["pred_contours"].append(wall(lambda: tiling.predict_tiled(model, img_d, contours=True, **kw)))
            t["device"].append(wall(lambda: ct.contours_instances(r)))
            t["host"].append(wall(host_route))
        med = {k: float(np.median(v)) for k, v in t.items()}
        k = kernels(r.labels[None], jobs, dev, a.reps)
        row.update({"a_contours_instances": stat(t["device"]), "a_host_route": stat(t["host"]), "a_host_over_device": round(med["host"] / med["device"], 3),
                    "b_predict_tiled": stat(t["pred"]), "b_predict_tiled_contours": stat(t["pred_contours"]),
                    "b_contours_over_plain": round(med["pred_contours"] / med["pred"], 4), **{"c_" + key: v for key, v in k.items()}})
        print(json.dumps(row), file=sys.stderr, flush=True)
        res["configs"].append(row)
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
