#!/usr/bin/env python
"""Per-instance measurements on one MI355X -> profiles/measure_bench.json.

Inputs: the calibrated weights and seeded uint8 images of 1040 x 1388 and 2048 x 2048 (tile 512, overlap 128, 8 tiles per predict call).
Per image, in alternating windows of one warmed-up process:
  a  measure.measure_instances on the predict_tiled result against its uploaded image (wall clock around a synchronisation), against
     the host route -- the map copied back, then measure.measure_host -- and, where scipy can be imported, against the route a user has
     today: the map copied back, scipy.ndimage.find_objects, then per id the ndimage sums inside its box
  b  kg_label_measure alone (device events; jobs and image already on the device, rows left there), next to a device-to-device copy of
     the bytes it reads: 4 per box pixel plus C per pixel of an instance (the neighbour rows it touches again are not counted)
  c  predict_tiled(measure=True) against predict_tiled() in the same process
Every figure is the median of the repeats with their minimum and maximum.

    python tools/measure_bench.py [--sizes 1040x1388,2048x2048] [--reps 5] [--out profiles/measure_bench.json]
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
from kg_instance_segmentation_amd import measure as ms  # noqa: E402


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


def scipy_route(ndi, lab, n, img):
    """area, centre of mass and per channel sum, sum of squares, min, max of every id inside its box (no edges, no second moments:
    ndimage has no one-call equivalent)"""
    out = np.zeros((n, 3 + 4 * img.shape[2]), np.float64)
    for i, sl in enumerate(ndi.find_objects(lab, n), 1):
        if sl is None:
            continue
        sel = lab[sl] == i
        out[i - 1, 0] = ndi.sum(sel)
        out[i - 1, 1:3] = ndi.center_of_mass(sel)
        for c in range(img.shape[2]):
            v = img[sl][..., c].astype(np.int64)
            out[i - 1, 3 + 4 * c:7 + 4 * c] = ndi.sum(v, sel), ndi.sum(v * v, sel), ndi.minimum(v, sel), ndi.maximum(v, sel)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1040x1388,2048x2048")
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "measure_bench.json"))
    a = ap.parse_args()
    try:
        import scipy.ndimage as ndi
    except ImportError:
        ndi = None
    from oracle import weightgen
    dev = torch.device("cuda", 0)
    model = KGnet.resnet50(pretrained=False)
    model.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    model = model.to(dev).eval()
    kw = dict(tile=a.tile, overlap=a.overlap, batch=a.batch)
    res = {"probe": "measure_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps, "tile": a.tile, "overlap": a.overlap, "batch": a.batch,
           "scipy": ndi is not None, "units": "ms (a, c: wall clock around a synchronisation; b: device events)", "configs": []}
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        img = np.random.default_rng(H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
        img_d = torch.from_numpy(img).to(dev)
        r = tiling.predict_tiled(model, img_d, **kw)                          # (also the warm-up)
        n = len(r)
        lab_h = r.labels.cpu().numpy()
        got = ms.measure_instances(r, img_d)
        assert np.array_equal(got.raw, ms.measure_host(lab_h, n, img))       # both routes count the same
        jobs = ms.jobs_from_stats(r.table[:, 1:6])
        jobs_d = torch.from_numpy(jobs).to(dev)
        box = np.maximum(jobs[:, 4] - jobs[:, 2], 0).astype(np.int64) * np.maximum(jobs[:, 5] - jobs[:, 3], 0)
        nbytes = int(4 * box.sum() + 3 * got.raw[:, 0].sum())
        bufs = (torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev), torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev))
        t = {k: [] for k in ("pred", "pred_measure", "device", "host", "scipy", "kernel", "kernel_geometry", "copy")}
        for _ in range(a.reps):
            t["pred"].append(wall(lambda: tiling.predict_tiled(model, img_d, **kw)))
            t["pred_measure"].append(wall(lambda: tiling.predict_tiled(model, img_d, measure=True, **kw)))
            t["device"].append(wall(lambda: ms.measure_instances(r, img_d)))
            t["host"].append(wall(lambda: ms.measure_host(r.labels.cpu().numpy(), n, img)))
            if ndi is not None:
                t["scipy"].append(wall(lambda: scipy_route(ndi, r.labels.cpu().numpy(), n, img)))
            t["kernel"].append(events(lambda: ms.measure_rows(r.labels, jobs_d, img_d)))
            t["kernel_geometry"].append(events(lambda: ms.measure_rows(r.labels, jobs_d)))
            t["copy"].append(events(lambda: bufs[1].copy_(bufs[0])))
        med = {k: float(np.median(v)) for k, v in t.items() if v}
        row = {"image": [H, W], "instances": n, "box_pixels": int(box.sum()), "instance_pixels": int(got.raw[:, 0].sum()),
               "median_box_side": round(float(np.sqrt(np.median(box[box > 0]))), 1) if (box > 0).any() else None,
               "a_measure_instances": stat(t["device"]), "a_host_route": stat(t["host"]),
               "a_host_over_device": round(med["host"] / med["device"], 3),
               "a_scipy_route": stat(t["scipy"]) if t["scipy"] else None,
               "a_scipy_over_device": round(med["scipy"] / med["device"], 3) if t["scipy"] else None,
               "b_bytes_read": nbytes, "b_copy_of_those_bytes": stat(t["copy"]),
               "b_label_measure_c3_u8": stat(t["kernel"]), "b_label_measure_ratio_to_copy": round(med["kernel"] / med["copy"], 3),
               "b_label_measure_geometry_only": stat(t["kernel_geometry"]),
               "c_predict_tiled": stat(t["pred"]), "c_predict_tiled_measure": stat(t["pred_measure"]),
               "c_measure_over_plain": round(med["pred_measure"] / med["pred"], 4)}
        print(json.dumps(row), file=sys.stderr, flush=True)
        res["configs"].append(row)
        del r, bufs, img_d, jobs_d
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
