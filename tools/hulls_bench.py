#!/usr/bin/env python
"""Convex hulls on one MI355X -> profiles/hulls_bench.json.

Inputs: the calibrated weights and seeded uint8 images of 1040 x 1388 and 2048 x 2048 (tile 512, overlap 128, 8 tiles per predict call).
Per image, in alternating windows of one warmed-up process:
  a  hulls.hulls_instances on the predict_tiled result (wall clock around a synchronisation) against the route a user has without it:
     labels.cpu().numpy(), scipy.ndimage.find_objects, and per id scipy.spatial.ConvexHull of the pixel corners of its box (skipped, and
     said so, where scipy does not import)
  b  predict_tiled(hulls=True) against predict_tiled() in the same process
  c  kg_label_hulls alone (device events; the table already on the device, rows and slabs left there), next to a device-to-device copy
     of the map
and the stated worst cases, on synthetic maps (hulls as wall clock, the kernel by device events):
  tall      ONE instance in a box of 4095 rows x 16 columns, one piece: every lane scans all 4096 lattice lines, the O(lines^2) envelope
  one_pixel 512 x 512 distinct ids: 262 144 jobs of one pixel each
Every figure is the median of the repeats with their minimum and maximum.

    python tools/hulls_bench.py [--sizes 1040x1388,2048x2048] [--reps 5] [--out profiles/hulls_bench.json]
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
from kg_instance_segmentation_amd import hulls as hl  # noqa: E402
from kg_instance_segmentation_amd._labelmaps import instance_jobs  # noqa: E402

try:
    from scipy import ndimage as ndi, spatial  # noqa: E402
except ImportError:                                                    # the host side is then not measured
    ndi = spatial = None


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


def scipy_route(lab_d, n):
    """What a user does today: the map copied back, the boxes of the ids, one ConvexHull per id -> (convex areas, vertex counts)"""
    lab = lab_d.cpu().numpy()
    area, count = np.zeros(n), np.zeros(n, np.int64)
    for k, sl in enumerate(ndi.find_objects(lab, max_label=n)):
        if sl is None:
            continue
        ys, xs = np.nonzero(lab[sl] == k + 1)
        pts = np.unique(np.concatenate([np.stack([xs + sl[1].start + b, ys + sl[0].start + a], 1) for a in (0, 1) for b in (0, 1)]), axis=0)
        q = spatial.ConvexHull(pts)
        area[k], count[k] = q.volume, len(q.vertices)
    return area, count


def kernel(lab, jobs, dev, reps, inner=10):
    j = np.asarray(jobs, np.int64)
    h, w = j[:, 4] - j[:, 2], j[:, 5] - j[:, 3]
    cap = np.where((h > 0) & (w > 0), 2 * (h + 1), 0)
    V = int(cap.sum())
    table = torch.from_numpy(np.concatenate([j, (np.cumsum(cap) - cap)[:, None], cap[:, None]], 1).astype(np.int32)).to(dev)
    rows, verts = torch.empty(len(j), 10, dtype=torch.int64, device=dev), torch.empty(V, 2, dtype=torch.int32, device=dev)
    copy_to = torch.empty_like(lab)
    t = {"copy": [], "hulls": []}
    for _ in range(reps):
        t["copy"].append(events(lambda: copy_to.copy_(lab), inner))
        t["hulls"].append(events(lambda: hl.hull_rows(lab, table, V, rows, verts), inner))
    r = rows.cpu().numpy()
    return {"jobs": len(j), "pieces_over_4095_rows": int((r[:, 9] == 1).sum()), "vertices": int(r[:, 1].sum()), "slab_vertices": V,
            "copy_of_the_map": stat(t["copy"]), "label_hulls": stat(t["hulls"]),
            "hulls_to_map_copy": round(float(np.median(t["hulls"])) / float(np.median(t["copy"])), 3)}


def worst_cases(dev, reps):
    out = {}

    def case(name, lab, jobs, host_reps):
        d = torch.from_numpy(lab).to(dev)
        got = hl.hulls(d, jobs=jobs)
        row = {"map": list(lab.shape), "wall_hulls": stat([wall(lambda: hl.hulls(d, jobs=jobs)) for _ in range(reps)])}
        if spatial is not None and host_reps:
            n = int(lab.max())
            host, seen = [], []
            for _ in range(host_reps):
                host.append(wall(lambda: seen.append(scipy_route(d, n))))
            area, count = seen[-1]
            assert np.array_equal(count, got.rows[:, 1]) and np.allclose(area, got.convex_areas(), rtol=1e-9)
            row.update({"wall_scipy_route": stat(host), "scipy_route_repeats": host_reps})
        row.update(kernel(d[None], hl.band_jobs(jobs)[0], dev, reps, inner=3))
        out[name] = row
        print(name, json.dumps(row), file=sys.stderr, flush=True)
    H, W = 4095, 16                                                    # 65 520 pixels: one piece at the default max_job_pixels
    y = np.arange(H)[:, None]
    lab = (np.abs(np.arange(W)[None, :] - 7.5) <= 1 + 7 * np.sin(np.pi * (y + 0.5) / H)).astype(np.int32)
    case("tall_4095_rows_one_instance", lab, np.array([[0, 1, 0, 0, H, W]]), reps)
    S = 512
    lab = np.arange(1, S * S + 1, dtype=np.int32).reshape(S, S)
    yy, xx = np.mgrid[0:S, 0:S]
    jobs = np.stack([np.zeros(S * S, np.int64), lab.reshape(-1), yy.reshape(-1), xx.reshape(-1), yy.reshape(-1) + 1, xx.reshape(-1) + 1], 1)
    case("one_pixel_512_distinct_jobs", lab, jobs, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1040x1388,2048x2048")
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hulls_bench.json"))
    a = ap.parse_args()
    from oracle import weightgen
    dev = torch.device("cuda", 0)
    model = KGnet.resnet50(pretrained=False)
    model.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    model = model.to(dev).eval()
    kw = dict(tile=a.tile, overlap=a.overlap, batch=a.batch)
    res = {"probe": "hulls_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps, "tile": a.tile, "overlap": a.overlap, "batch": a.batch,
           "host_route": ("labels.cpu().numpy() + scipy.ndimage.find_objects + scipy.spatial.ConvexHull per id" if spatial is not None
                          else "not measured: scipy does not import"),
           "units": "ms (a, b, wall_*: wall clock around a synchronisation; c and the worst cases' kernel: device events)",
           "not_measured": ["skimage.measure.regionprops (not installed)", "more than one image per launch", "the host merge of banded jobs alone"],
           "configs": []}
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        img_d = torch.from_numpy(np.random.default_rng(H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
        r = tiling.predict_tiled(model, img_d, **kw)                          # (also the warm-up)
        n = len(r)
        jobs = instance_jobs(r, 0, 0, H, W)
        got = hl.hulls_instances(r)
        assert np.array_equal(got.areas(), np.asarray(r.table)[:, 1])
        row = {"image": [H, W], "instances": n, "map_bytes": 4 * H * W, "hull_vertices": int(len(got.verts)),
               "largest_box": [int((jobs[:, 4] - jobs[:, 2]).max(initial=0)), int((jobs[:, 5] - jobs[:, 3]).max(initial=0))]}
        if spatial is not None:
            area, count = scipy_route(r.labels, n)
            assert np.array_equal(count, got.rows[:, 1]) and np.allclose(area, got.convex_areas(), rtol=1e-9)     # both routes give the same hulls
        t = {k: [] for k in ("device", "host", "pred", "pred_hulls")}
        for _ in range(a.reps):
            t["pred"].append(wall(lambda: tiling.predict_tiled(model, img_d, **kw)))
            t["pred_hulls"].append(wall(lambda: tiling.predict_tiled(model, img_d, hulls=True, **kw)))
            t["device"].append(wall(lambda: hl.hulls_instances(r)))
            if spatial is not None:
                t["host"].append(wall(lambda: scipy_route(r.labels, n)))
        med = {k: float(np.median(v)) for k, v in t.items() if v}
        row.update({"a_hulls_instances": stat(t["device"]), "b_predict_tiled": stat(t["pred"]), "b_predict_tiled_hulls": stat(t["pred_hulls"]),
                    "b_hulls_over_plain": round(med["pred_hulls"] / med["pred"], 4)})
        if spatial is not None:
            row.update({"a_scipy_route": stat(t["host"]), "a_scipy_over_device": round(med["host"] / med["device"], 3)})
        row.update({"c_" + key: v for key, v in kernel(r.labels[None], hl.band_jobs(jobs)[0], dev, a.reps).items()})
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
