#!/usr/bin/env python
"""Label-map clean-up on one MI355X -> profiles/components_bench.json.

Inputs: the calibrated weights and seeded uint8 images of 1040 x 1388 and 2048 x 2048 (tile 512, overlap 128, 8 tiles per predict call).
Per image, in alternating windows of one warmed-up process:
  a  components.clean_instances on the predict_tiled result (wall clock around a synchronisation), against the host route -- the map
     copied back, then components.clean_host -- and, where scipy can be imported, against the route a user has today: the map copied
     back, scipy.ndimage.find_objects, then per id scipy.ndimage.label inside its box, the largest piece kept, binary_fill_holes
  b  kg_label_components (6 launches), kg_component_stats (3) and kg_component_remap (1), each entry alone (device events), next to a
     device-to-device copy of one map (the entry reads one map and writes at most one), as a ratio.  The launches of one entry are not
     separated: they are not exported one by one.
  c  predict_tiled(clean={...}) against predict_tiled() in the same process
  d  kg_label_components on the stated worst cases: ONE serpentine over the whole image (the longest chain across every seam) and a
     checkerboard of one id (4: the largest possible component count; 8: one component, every pixel a run of its own)
Every figure is the median of the repeats with their minimum and maximum.

    python tools/components_bench.py [--sizes 1040x1388,2048x2048] [--reps 5] [--out profiles/components_bench.json]
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
from kg_instance_segmentation_amd import components as cc  # noqa: E402

POLICY = dict(keep="largest", min_area=4, fill_holes=True)


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


def scipy_route(ndi, lab, n):
    """keep the largest piece of every id (8-connectivity), drop pieces below min_area, fill its holes -- inside the id's box"""
    out = np.zeros_like(lab)
    eight = ndi.generate_binary_structure(2, 2)
    for i, sl in enumerate(ndi.find_objects(lab, n), 1):
        if sl is None:
            continue
        part, k = ndi.label(lab[sl] == i, eight)
        area = np.bincount(part.reshape(-1))[1:]
        best = int(np.argmax(area)) + 1
        if area[best - 1] >= POLICY["min_area"]:
            keep = ndi.binary_fill_holes(part == best)
            out[sl][keep & ((lab[sl] == 0) | (part == best))] = i
    return out


def serpentine(H, W):
    lab = np.zeros((H, W), np.int32)
    lab[0::2] = 1
    odd = np.arange(1, H, 2)
    lab[odd, np.where((odd // 2) % 2 == 0, W - 1, 0)] = 1
    return lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1040x1388,2048x2048")
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_bench.json"))
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
    res = {"probe": "components_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps, "tile": a.tile, "overlap": a.overlap, "batch": a.batch,
           "policy": POLICY, "scipy": ndi is not None, "units": "ms (a, c: wall clock around a synchronisation; b, d: device events)", "configs": []}
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        img = np.random.default_rng(H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
        r = tiling.predict_tiled(model, img, **kw)                           # (also the warm-up)
        n = len(r)
        lab_h = r.labels.cpu().numpy()
        cleaned = cc.clean_instances(r, **POLICY)
        want = cc.clean_host(lab_h, n, table=r.table, **POLICY)
        assert np.array_equal(cleaned.labels.cpu().numpy(), want[0]) and np.array_equal(cleaned.table, want[1])     # both routes decide the same
        comp, ncomp = cc.components(r.labels, 8, 4)
        stats, start = cc.component_stats(r.labels, comp, ncomp)
        newval = torch.from_numpy(np.ascontiguousarray(stats[:, 0].astype(np.int32))).to(dev)
        bufs = (torch.empty(H * W, dtype=torch.int32, device=dev), torch.empty(H * W, dtype=torch.int32, device=dev))
        worst = {"serpentine": torch.from_numpy(serpentine(H, W)).to(dev),
                 "checkerboard": torch.from_numpy(((np.add.outer(np.arange(H), np.arange(W)) % 2)).astype(np.int32)).to(dev)}
        t = {k: [] for k in ("pred", "pred_clean", "clean", "host", "scipy", "comp", "stats", "remap", "copy")}
        tw = {(k, c): [] for k in worst for c in (4, 8)}
        for _ in range(a.reps):
            t["pred"].append(wall(lambda: tiling.predict_tiled(model, img, **kw)))
            t["pred_clean"].append(wall(lambda: tiling.predict_tiled(model, img, clean=POLICY, **kw)))
            t["clean"].append(wall(lambda: cc.clean_instances(r, **POLICY)))
            t["host"].append(wall(lambda: cc.clean_host(r.labels.cpu().numpy(), n, table=r.table, **POLICY)))
            if ndi is not None:
                t["scipy"].append(wall(lambda: scipy_route(ndi, r.labels.cpu().numpy(), n)))
            t["comp"].append(events(lambda: cc.components(r.labels, 8, 4)))
            t["stats"].append(events(lambda: stats_only(r.labels, comp, start)))
            t["remap"].append(events(lambda: cc.remap(comp, start, newval)))
            t["copy"].append(events(lambda: bufs[1].copy_(bufs[0])))
            for (k, c) in tw:
                tw[(k, c)].append(events(lambda: cc.components(worst[k], c, 0), inner=3))
        med = {k: float(np.median(v)) for k, v in t.items() if v}
        row = {"image": [H, W], "instances": n, "components_8_bg4": int(start[-1]), "pixels_changed": int((want[0] != lab_h).sum()),
               "a_clean_instances": stat(t["clean"]), "a_host_route": stat(t["host"]),
               "a_host_over_device": round(med["host"] / med["clean"], 3),
               "a_scipy_route": stat(t["scipy"]) if t["scipy"] else None,
               "a_scipy_over_device": round(med["scipy"] / med["clean"], 3) if t["scipy"] else None,
               "b_copy_one_map": stat(t["copy"]), "b_map_bytes": H * W * 4,
               "b_label_components": stat(t["comp"]), "b_label_components_ratio_to_copy": round(med["comp"] / med["copy"], 3),
               "b_component_stats": stat(t["stats"]), "b_component_stats_ratio_to_copy": round(med["stats"] / med["copy"], 3),
               "b_component_remap": stat(t["remap"]), "b_component_remap_ratio_to_copy": round(med["remap"] / med["copy"], 3),
               "c_predict_tiled": stat(t["pred"]), "c_predict_tiled_clean": stat(t["pred_clean"]),
               "c_clean_over_plain": round(med["pred_clean"] / med["pred"], 4)}
        for (k, c), v in tw.items():
            row[f"d_{k}_conn{c}"] = stat(v)
            row[f"d_{k}_conn{c}_over_seeded"] = round(float(np.median(v)) / med["comp"], 3)
        print(json.dumps(row), file=sys.stderr, flush=True)
        res["configs"].append(row)
        del r, comp, ncomp, newval, bufs, worst, cleaned
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def stats_only(labels, comp, start):
    """kg_component_stats alone: no read-back of ncomp, no copy of the stats"""
    from kg_instance_segmentation_amd import _lib
    H, W = labels.shape
    total = int(start[-1])
    out = torch.empty(total, 9, dtype=torch.int32, device=labels.device)
    _lib.call("kg_component_stats", _lib.ptr(labels), _lib.ptr(comp), 1, H, W, start.ctypes.data, total, _lib.ptr(out) if total else None, _lib.stream_ptr())
    return out


if __name__ == "__main__":
    main()
