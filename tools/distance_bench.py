#!/usr/bin/env python
"""Nearest-other-label distance maps on one MI355X -> profiles/distance_bench.json.

Inputs: the calibrated weights and seeded uint8 images of 1040 x 1388 and 2048 x 2048 (tile 512, overlap 128, 8 tiles per predict call).
Per image, in alternating windows of one warmed-up process:
  a  distance.expand_instances on the predict_tiled result at distances 4, 16 and 64, and distance.inscribed at max_d2 = 4096 (wall clock
     around a synchronisation), against the route a user has today, where scipy can be imported: the map copied back,
     scipy.ndimage.distance_transform_edt(return_indices=True) of the background, the expansion from its indices, and for the inscribed
     circle one more transform of the foreground and the ndimage maximum per id
  b  kg_label_distance (both outputs) and kg_label_regrow (expand) alone per radius (device events; the map on the device, outputs left
     there), next to a device-to-device copy of the bytes they read and write (4 in and 8 out per pixel; 4 and 4 for regrow), on the
     predicted map and on the two worst cases: a map of zeros with ONE source pixel (no scan can stop early anywhere near it, and every
     tile beyond its reach is skipped) and a checkerboard (every scan ends at distance 1)
  c  predict_tiled(expand=8, measure=True) against predict_tiled(measure=True) in the same process
Every figure is the median of the repeats with their minimum and maximum.

    python tools/distance_bench.py [--sizes 1040x1388,2048x2048] [--reps 5] [--out profiles/distance_bench.json]
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
from kg_instance_segmentation_amd import distance as dt  # noqa: E402

RADII = (4, 16, 64)


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


def scipy_expand(ndi, lab, dist):
    edt, idx = ndi.distance_transform_edt(lab == 0, return_indices=True)
    return np.where(edt <= dist, lab[idx[0], idx[1]], 0)


def scipy_inscribed(ndi, lab, n):
    """the largest inner distance per id and where: the background's transform cannot tell two touching ids apart, so every id's boundary
    is cut first (a 4-neighbour difference), then one transform and the ndimage maximum per id"""
    edge = np.zeros(lab.shape, bool)
    edge[:-1] |= lab[:-1] != lab[1:]; edge[1:] |= lab[1:] != lab[:-1]
    edge[:, :-1] |= lab[:, :-1] != lab[:, 1:]; edge[:, 1:] |= lab[:, 1:] != lab[:, :-1]
    edt = ndi.distance_transform_edt(~edge)
    ids = np.arange(1, n + 1)
    return ndi.maximum(edt, lab, ids), ndi.maximum_position(edt, lab, ids)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1040x1388,2048x2048")
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distance_bench.json"))
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
    res = {"probe": "distance_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps, "tile": a.tile, "overlap": a.overlap, "batch": a.batch,
           "kernel_tile": [dt.TILE_H, dt.TILE_W], "scipy": ndi is not None,
           "units": "ms (a, c: wall clock around a synchronisation; b: device events)", "configs": []}
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        img = np.random.default_rng(H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
        img_d = torch.from_numpy(img).to(dev)
        r = tiling.predict_tiled(model, img_d, **kw)                          # (also the warm-up)
        n = len(r)
        lab_h = r.labels.cpu().numpy()
        one = torch.zeros(H, W, dtype=torch.int32, device=dev)
        one[H // 2, W // 2] = 1
        yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
        maps = {"predicted": r.labels, "one_source": one, "checkerboard": ((yy + xx) % 2 + 1).to(torch.int32).contiguous()}
        for d in RADII:                                                       # warm-up, and both routes agree where scipy has no tie to break
            dt.expand_instances(r, d)
        dt.inscribed(r.labels, n, stats=r.table[:, 1:6])
        bufs = {k: (torch.empty(k * H * W, dtype=torch.int32, device=dev), torch.empty(k * H * W, dtype=torch.int32, device=dev)) for k in (1, 2)}
        t = {}

        def add(key, v):
            t.setdefault(key, []).append(v)
        for _ in range(a.reps):
            add("pred_measure", wall(lambda: tiling.predict_tiled(model, img_d, measure=True, **kw)))
            add("pred_expand_measure", wall(lambda: tiling.predict_tiled(model, img_d, measure=True, expand=8, **kw)))
            for d in RADII:
                add(f"expand_{d}", wall(lambda: dt.expand_instances(r, d)))
                if ndi is not None:
                    add(f"scipy_expand_{d}", wall(lambda: scipy_expand(ndi, r.labels.cpu().numpy(), d)))
                for name, m in maps.items():
                    add(f"distance_{name}_{d}", events(lambda: dt.distance(m, d * d)))
                    add(f"regrow_{name}_{d}", events(lambda: dt.expand_labels(m, d)))
            add("inscribed", wall(lambda: dt.inscribed(r.labels, n, stats=r.table[:, 1:6])))
            if ndi is not None:
                add("scipy_inscribed", wall(lambda: scipy_inscribed(ndi, r.labels.cpu().numpy(), n)))
            add("copy_12", events(lambda: (bufs[1][1].copy_(bufs[1][0]), bufs[2][1].copy_(bufs[2][0]))))     # 4 read + 8 written per pixel
            add("copy_8", events(lambda: bufs[1][1].copy_(bufs[1][0])))                                      # 4 read + 4 written per pixel
        med = {k: float(np.median(v)) for k, v in t.items()}
        row = {"image": [H, W], "instances": n, "foreground_share": round(float((lab_h != 0).mean()), 4),
               "b_copy_4_in_8_out": stat(t["copy_12"]), "b_copy_4_in_4_out": stat(t["copy_8"]),
               "c_predict_tiled_measure": stat(t["pred_measure"]), "c_predict_tiled_expand8_measure": stat(t["pred_expand_measure"]),
               "c_expand_over_plain": round(med["pred_expand_measure"] / med["pred_measure"], 4),
               "a_inscribed_4096": stat(t["inscribed"]), "a_scipy_inscribed": stat(t["scipy_inscribed"]) if ndi is not None else None}
        for d in RADII:
            row[f"a_expand_instances_{d}"] = stat(t[f"expand_{d}"])
            if ndi is not None:
                row[f"a_scipy_expand_{d}"] = stat(t[f"scipy_expand_{d}"])
                row[f"a_scipy_over_device_{d}"] = round(med[f"scipy_expand_{d}"] / med[f"expand_{d}"], 2)
            for name in maps:
                row[f"b_distance_{name}_{d}"] = stat(t[f"distance_{name}_{d}"])
                row[f"b_distance_{name}_{d}_over_copy"] = round(med[f"distance_{name}_{d}"] / med["copy_12"], 2)
                row[f"b_regrow_{name}_{d}"] = stat(t[f"regrow_{name}_{d}"])
                row[f"b_regrow_{name}_{d}_over_copy"] = round(med[f"regrow_{name}_{d}"] / med["copy_8"], 2)
        print(json.dumps(row), file=sys.stderr, flush=True)
        res["configs"].append(row)
        del r, bufs, img_d, maps, one
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
