#!/usr/bin/env python
"""Per-instance intensity quantiles on one MI355X -> profiles/intensity_bench.json.

Inputs: the calibrated weights and seeded uint8 images of 1040 x 1388 and 2048 x 2048 (tile 512, overlap 128, 8 tiles per predict call),
the 3-channel uint8 source image as the intensity image.  Per image, in alternating windows of one warmed-up process:
  a  intensity.quantiles_instances on the predict_tiled result against its uploaded image (wall clock around a synchronisation), against
     the route a user has today: the map copied back, scipy.ndimage.find_objects (the boxes of the instance table where scipy does not
     import, and said so), then np.percentile per id and channel
  b  predict_tiled(quantiles=True, measure=True) against predict_tiled(measure=True) in the same process
  c  kg_label_quantiles alone (device events; table, jobs and image already on the device, rows left there), next to kg_label_measure on
     the same jobs and image -- it walks the same pixels once -- and next to a device-to-device copy of the bytes one walk reads: 4 per box
     pixel plus C per pixel of an instance
  d  the same with the image widened to uint16 (value * 257: both bytes vary), which prices the second walk
and the stated worst cases, kernel by device events and quantiles() as wall clock:
  constant   the image of c set to one value: every lane of a wave adds to ONE LDS address
  one_object one 250 x 250 object: 62 500 pixels walked by one workgroup (twice for uint16)
  one_pixel  512 x 512 distinct ids: 262 144 jobs of one pixel each
Every figure is the median of the repeats with their minimum and maximum.

    python tools/intensity_bench.py [--sizes 1040x1388,2048x2048] [--reps 5] [--out profiles/intensity_bench.json]
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
from kg_instance_segmentation_amd import intensity as iq  # noqa: E402
from kg_instance_segmentation_amd import measure as ms  # noqa: E402

try:
    from scipy import ndimage as ndi  # noqa: E402
except ImportError:
    ndi = None

PCT = [float(f) * 100 for f in iq.DEFAULT_Q]


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


def host_route(lab_d, table, img):
    """What a user does today: the map copied back, the boxes of the ids, np.percentile per id and channel -> float64 [n, C, Q]"""
    lab = lab_d.cpu().numpy()
    n = len(table)
    if ndi is not None:
        boxes = ndi.find_objects(lab, max_label=n)
    else:
        boxes = [(slice(int(t[2]), int(t[4])), slice(int(t[3]), int(t[5]))) if t[1] > 0 else None for t in table]
    out = np.full((n, img.shape[2], len(PCT)), np.nan)
    for k, sl in enumerate(boxes):
        if sl is None:
            continue
        sel = lab[sl] == k + 1
        for c in range(img.shape[2]):
            out[k, c] = np.percentile(img[sl][..., c][sel], PCT)
    return out


def kernels(lab, jobs, img_d, reps, inner=10):
    """device events of kg_label_quantiles, kg_label_measure and a copy of the bytes one walk reads, for one image tensor"""
    dev = lab.device
    jobs_d = torch.from_numpy(np.ascontiguousarray(jobs, np.int32)).to(dev)
    qd = torch.from_numpy(iq.q_table(None)).to(dev)
    j = np.asarray(jobs, np.int64)
    box = np.maximum(j[:, 4] - j[:, 2], 0) * np.maximum(j[:, 5] - j[:, 3], 0)
    rows = iq.quantile_rows(lab, jobs_d, img_d, qd).cpu().numpy()
    nbytes = int(4 * box.sum() + img_d.shape[-1] * img_d.element_size() * rows[:, 0, 0].sum())
    bufs = (torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev), torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev))
    t = {"quantiles": [], "measure": [], "copy": []}
    for _ in range(reps):
        t["quantiles"].append(events(lambda: iq.quantile_rows(lab, jobs_d, img_d, qd), inner))
        t["measure"].append(events(lambda: ms.measure_rows(lab, jobs_d, img_d), inner))
        t["copy"].append(events(lambda: bufs[1].copy_(bufs[0]), inner))
    med = {k: float(np.median(v)) for k, v in t.items()}
    return {"jobs": len(j), "box_pixels": int(box.sum()), "instance_pixels": int(rows[:, 0, 0].sum()), "bytes_of_one_walk": nbytes,
            "label_quantiles": stat(t["quantiles"]), "label_measure": stat(t["measure"]), "copy_of_those_bytes": stat(t["copy"]),
            "quantiles_over_measure": round(med["quantiles"] / med["measure"], 3), "quantiles_over_copy": round(med["quantiles"] / med["copy"], 3)}


def widen(img_d):
    """uint8 device image -> the same as 16-bit values v * 257 (int16 storage, read unsigned)"""
    return (img_d.to(torch.int32) * 257).to(torch.int16)


def worst_cases(dev, reps):
    out = {}

    def case(name, lab, jobs, img):
        d, di = torch.from_numpy(lab).to(dev), torch.from_numpy(img).to(dev)
        row = {"map": list(lab.shape)}
        for tag, im in (("u8", di), ("u16", widen(di))):
            got = iq.quantiles(d, jobs=jobs, image=im)
            assert got.counts().sum() > 0
            row["wall_quantiles_" + tag] = stat([wall(lambda: iq.quantiles(d, jobs=jobs, image=im)) for _ in range(reps)])
            row["kernel_" + tag] = kernels(d[None], jobs, im[None], reps, inner=3)
        out[name] = row
        print(name, json.dumps(row), file=sys.stderr, flush=True)
    S = 250
    lab = np.zeros((256, 256), np.int32)
    lab[3:3 + S, 2:2 + S] = 1
    img = np.random.default_rng(5).integers(0, 256, (256, 256, 3), dtype=np.uint8)
    case("one_object_250x250", lab, np.array([[0, 1, 3, 2, 3 + S, 2 + S]]), img)
    S = 512
    lab = np.arange(1, S * S + 1, dtype=np.int32).reshape(S, S)
    yy, xx = np.mgrid[0:S, 0:S]
    jobs = np.stack([np.zeros(S * S, np.int64), lab.reshape(-1), yy.reshape(-1), xx.reshape(-1), yy.reshape(-1) + 1, xx.reshape(-1) + 1], 1)
    case("one_pixel_512x512_jobs", lab, jobs, np.random.default_rng(6).integers(0, 256, (S, S, 3), dtype=np.uint8))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1040x1388,2048x2048")
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intensity_bench.json"))
    a = ap.parse_args()
    from oracle import weightgen
    dev = torch.device("cuda", 0)
    model = KGnet.resnet50(pretrained=False)
    model.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    model = model.to(dev).eval()
    kw = dict(tile=a.tile, overlap=a.overlap, batch=a.batch)
    res = {"probe": "intensity_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps, "tile": a.tile, "overlap": a.overlap, "batch": a.batch,
           "quantiles": [str(f) for f in iq.DEFAULT_Q],
           "host_route": "labels.cpu().numpy() + " + ("scipy.ndimage.find_objects" if ndi is not None else "the boxes of the instance table (scipy does not import)")
                         + " + np.percentile per id and channel",
           "units": "ms (a, b, wall_*: wall clock around a synchronisation; c, d and the worst cases' kernels: device events over back-to-back calls)",
           "not_measured": ["the split of kg_label_quantiles' time between the walk, the LDS atomics and the scan / select",
                            "skimage.measure.regionprops and CellProfiler (not installed)", "more than one image per launch",
                            "the histogram route of jobs above max_job_pixels", "histograms()", "uint16 images with 12-bit content"],
           "configs": []}
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        img = np.random.default_rng(H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
        img_d = torch.from_numpy(img).to(dev)
        r = tiling.predict_tiled(model, img_d, **kw)                          # (also the warm-up)
        n = len(r)
        got = iq.quantiles_instances(r, img_d)
        assert np.array_equal(got.counts(), np.asarray(r.table)[:, 1])
        np.testing.assert_allclose(got.linear(), host_route(r.labels, r.table, img), rtol=1e-9)      # both routes give the same quantiles
        jobs = ms.jobs_from_stats(np.asarray(r.table)[:, 1:6])
        t = {k: [] for k in ("device", "host", "pred", "pred_q")}
        for _ in range(a.reps):
            t["pred"].append(wall(lambda: tiling.predict_tiled(model, img_d, measure=True, **kw)))
            t["pred_q"].append(wall(lambda: tiling.predict_tiled(model, img_d, measure=True, quantiles=True, **kw)))
            t["device"].append(wall(lambda: iq.quantiles_instances(r, img_d)))
            t["host"].append(wall(lambda: host_route(r.labels, r.table, img)))
        med = {k: float(np.median(v)) for k, v in t.items()}
        box = np.maximum(jobs[:, 4] - jobs[:, 2], 0).astype(np.int64) * np.maximum(jobs[:, 5] - jobs[:, 3], 0)
        row = {"image": [H, W], "instances": n, "map_bytes": 4 * H * W,
               "median_box_side": round(float(np.sqrt(np.median(box[box > 0]))), 1) if (box > 0).any() else None,
               "jobs_above_max_job_pixels": int((box > 65536).sum()),
               "a_quantiles_instances": stat(t["device"]), "a_host_route": stat(t["host"]), "a_host_over_device": round(med["host"] / med["device"], 3),
               "b_predict_tiled_measure": stat(t["pred"]), "b_predict_tiled_measure_quantiles": stat(t["pred_q"]),
               "b_quantiles_over_plain": round(med["pred_q"] / med["pred"], 4),
               "c_u8": kernels(r.labels[None], jobs, img_d[None], a.reps), "d_u16": kernels(r.labels[None], jobs, widen(img_d)[None], a.reps),
               "worst_constant_u8": kernels(r.labels[None], jobs, torch.full_like(img_d, 93)[None], a.reps),
               "worst_constant_u16": kernels(r.labels[None], jobs, widen(torch.full_like(img_d, 93))[None], a.reps)}
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
