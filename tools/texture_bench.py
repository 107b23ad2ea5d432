#!/usr/bin/env python
"""Per-instance texture (co-occurrence matrices, Haralick features) on one MI355X -> profiles/texture_bench.json.

Inputs: the calibrated weights and seeded uint8 images of 1040 x 1388 and 2048 x 2048 (tile 512, overlap 128, 8 tiles per predict call),
the 3-channel uint8 source image as the intensity image.  Per image, in alternating windows of one warmed-up process:
  a  texture.texture_instances on the predict_tiled result against its uploaded image (wall clock around a synchronisation) at L = 16,
     d = 1 and at L = 32, d = (1, 3), against the route a user has today: the map copied back, scipy.ndimage.find_objects (the boxes of the
     instance table where scipy does not import, and said so), then a NumPy co-occurrence count per id, channel, distance and direction.
     mahotas and skimage are not installed, so their haralick / graycomatrix are not what is timed.
  b  predict_tiled(texture={...}) against predict_tiled without it in the same process
  c  kg_label_glcm alone (device events over ten back-to-back calls; jobs and image already on the device, rows left there), next to
     kg_label_measure on the same boxes and image, next to a device-to-device copy of the bytes one walk reads -- per kernel job 5 bytes
     (a label and one byte of the pixel) per pixel of the staged rectangle (h + d) x (w + 2 d) -- and, separately, the copy back of the
     rows (4 L^2 ints per kernel job; wall clock, the copy synchronises)
and the stated worst cases, kernel by device events and glcm() as wall clock:
  constant    the image of c set to one value: every atomic of a direction lands on ONE LDS address
  one_object  one 250 x 250 object, as one job (direct from global memory) and in 63-row bands (staged)
  one_pixel   512 x 512 distinct ids: 262 144 jobs of one pixel each
Every figure is the median of the repeats with their minimum and maximum.

    python tools/texture_bench.py [--sizes 1040x1388,2048x2048] [--reps 5] [--out profiles/texture_bench.json]
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
from kg_instance_segmentation_amd import texture as tx  # noqa: E402
from kg_instance_segmentation_amd.labelmetrics import split_jobs  # noqa: E402

try:
    from scipy import ndimage as ndi  # noqa: E402
except ImportError:
    ndi = None

CONFIGS = (("L16_d1", 16, (1,)), ("L32_d1_3", 32, (1, 3)))


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


def host_route(lab_d, table, img, L, ds):
    """What a user does today: the map copied back, the boxes of the ids, a NumPy co-occurrence count per id, channel, distance and
    direction inside the id's box -> int64 [n, C, D, 4, L, L]"""
    lab = lab_d.cpu().numpy()
    n, C = len(table), img.shape[2]
    if ndi is not None:
        boxes = ndi.find_objects(lab, max_label=n)
    else:
        boxes = [(slice(int(t[2]), int(t[4])), slice(int(t[3]), int(t[5]))) if t[1] > 0 else None for t in table]
    out = np.zeros((n, C, len(ds), 4, L, L), np.int64)
    for k, sl in enumerate(boxes):
        if sl is None:
            continue
        sel = lab[sl] == k + 1
        h, w = sel.shape
        lev = img[sl].astype(np.int64) * L // 256
        for a, d in enumerate(ds):
            for q, (oy, ox) in enumerate(tx.OFFSETS):
                dy, dx = oy * d, ox * d
                if h <= dy or w <= abs(dx):
                    continue
                cen = (slice(0, h - dy), slice(max(-dx, 0), w - max(dx, 0)))
                par = (slice(dy, h), slice(max(dx, 0), w - max(-dx, 0)))
                both = sel[cen] & sel[par]
                for c in range(C):
                    out[k, c, a, q] = np.bincount(lev[cen][..., c][both] * L + lev[par][..., c][both], minlength=L * L).reshape(L, L)
    return out


def kernel_jobs(jobs6, C, L, ds, cap=65536):
    pieces, owner = split_jobs(np.asarray(jobs6, np.int64), cap)
    m = len(jobs6)
    return tx.texture_jobs(pieces, tuple(range(C)), ds, np.zeros((m, C), np.int64), np.full((m, C), 256, np.int64), owner), pieces


def kernels(lab, jobs6, img_d, L, ds, reps, inner=10, cap=65536):
    """device events of kg_label_glcm, kg_label_measure and a copy of the bytes one walk reads; wall clock of the rows' copy back"""
    dev = lab.device
    C = img_d.shape[-1]
    j10, pieces = kernel_jobs(jobs6, C, L, ds, cap)
    jd = torch.from_numpy(np.ascontiguousarray(j10, np.int32)).to(dev)
    j6d = torch.from_numpy(np.ascontiguousarray(pieces, np.int32)).to(dev)
    h, w, d = np.maximum(j10[:, 4] - j10[:, 2], 0), np.maximum(j10[:, 5] - j10[:, 3], 0), j10[:, 7]
    live = (h > 0) & (w > 0)
    nbytes = int((5 * (h + d) * (w + 2 * d))[live].sum())
    staged = int(((h + d) * (w + 2 * d) <= tx.STAGE_CELLS)[live].sum())
    rows = tx.glcm_rows(lab, jd, img_d, L)
    bufs = (torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev), torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev))
    t = {"glcm": [], "measure": [], "copy": [], "rows_back": []}
    for _ in range(reps):
        t["glcm"].append(events(lambda: tx.glcm_rows(lab, jd, img_d, L), inner))
        t["measure"].append(events(lambda: ms.measure_rows(lab, j6d, img_d), inner))
        t["copy"].append(events(lambda: bufs[1].copy_(bufs[0]), inner))
        t["rows_back"].append(wall(lambda: rows.cpu()))
    med = {k: float(np.median(v)) for k, v in t.items()}
    return {"kernel_jobs": len(j10), "staged_jobs": staged, "direct_jobs": int(live.sum()) - staged, "pairs": int(rows.sum().item()),
            "bytes_of_one_walk": nbytes, "row_bytes": int(rows.numel() * 4),
            "label_glcm": stat(t["glcm"]), "label_measure_same_boxes": stat(t["measure"]), "copy_of_those_bytes": stat(t["copy"]),
            "rows_copy_back_wall": stat(t["rows_back"]),
            "glcm_over_measure": round(med["glcm"] / med["measure"], 3), "glcm_over_copy": round(med["glcm"] / med["copy"], 3)}


def worst_cases(dev, reps):
    out = {}

    def case(name, lab, jobs, img, cap=65536, whole=True):
        d, di = torch.from_numpy(lab).to(dev), torch.from_numpy(img).to(dev)
        row = {"map": list(lab.shape), "channels": img.shape[2], "max_job_pixels": cap}
        if whole:                                                            # glcm() end to end: upload, launch, copy back, bands added
            assert np.array_equal(tx.glcm(d, jobs=jobs, image=di, max_job_pixels=cap).counts, tx.glcm_host(lab, jobs, img).counts)
            row["wall_glcm_L16_d1"] = stat([wall(lambda: tx.glcm(d, jobs=jobs, image=di, max_job_pixels=cap)) for _ in range(reps)])
        row["kernel_L16_d1"] = kernels(d[None], jobs, di[None], 16, (1,), reps, inner=3, cap=cap)
        out[name] = row
        print(name, json.dumps(row), file=sys.stderr, flush=True)
    S = 250
    lab = np.zeros((256, 256), np.int32)
    lab[3:3 + S, 2:2 + S] = 1
    img = np.random.default_rng(5).integers(0, 256, (256, 256, 3), dtype=np.uint8)
    job = np.array([[0, 1, 3, 2, 3 + S, 2 + S]])
    case("one_object_250x250_direct", lab, job, img, 2 ** 30)
    case("one_object_250x250_staged_bands", lab, job, img, 63 * S)
    case("one_object_250x250_constant_direct", lab, job, np.full_like(img, 93), 2 ** 30)
    case("one_object_250x250_constant_staged_bands", lab, job, np.full_like(img, 93), 63 * S)
    S = 512
    lab = np.arange(1, S * S + 1, dtype=np.int32).reshape(S, S)
    yy, xx = np.mgrid[0:S, 0:S]
    jobs = np.stack([np.zeros(S * S, np.int64), lab.reshape(-1), yy.reshape(-1), xx.reshape(-1), yy.reshape(-1) + 1, xx.reshape(-1) + 1], 1)
    # one channel, kernel and copy back only: the rows are 1 GiB, and glcm() would hold them twice more on the host
    case("one_pixel_512x512_jobs", lab, jobs, np.random.default_rng(6).integers(0, 256, (S, S, 1), dtype=np.uint8), whole=False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1040x1388,2048x2048")
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture_bench.json"))
    a = ap.parse_args()
    from oracle import weightgen
    dev = torch.device("cuda", 0)
    model = KGnet.resnet50(pretrained=False)
    model.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    model = model.to(dev).eval()
    kw = dict(tile=a.tile, overlap=a.overlap, batch=a.batch)
    res = {"probe": "texture_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps, "tile": a.tile, "overlap": a.overlap, "batch": a.batch,
           "host_route": "labels.cpu().numpy() + " + ("scipy.ndimage.find_objects" if ndi is not None else "the boxes of the instance table (scipy does not import)")
                         + " + a NumPy co-occurrence count (shifted slices, np.bincount) per id, channel, distance and direction",
           "units": "ms (a, b, wall_*, rows_copy_back_wall: wall clock around a synchronisation; c and the worst cases' kernels: device events over back-to-back calls)",
           "not_measured": ["mahotas.features.haralick, skimage.feature.graycomatrix / graycoprops and CellProfiler (not installed)",
                            "the split of kg_label_glcm's time between staging, the pair reads and the LDS atomics",
                            "uint16 images", "range=\"object\" (one more kg_label_measure launch and copy back)", "more than one image per launch",
                            "haralick() / props() on the host (float64 NumPy over the rows)", "a ballot fold of equal bins within a wave (not built)"],
           "configs": []}
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        img = np.random.default_rng(H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
        img_d = torch.from_numpy(img).to(dev)
        r = tiling.predict_tiled(model, img_d, **kw)                          # (also the warm-up)
        n = len(r)
        jobs = ms.jobs_from_stats(np.asarray(r.table)[:, 1:6])
        box = np.maximum(jobs[:, 4] - jobs[:, 2], 0).astype(np.int64) * np.maximum(jobs[:, 5] - jobs[:, 3], 0)
        row = {"image": [H, W], "instances": n, "map_bytes": 4 * H * W,
               "median_box_side": round(float(np.sqrt(np.median(box[box > 0]))), 1) if (box > 0).any() else None,
               "jobs_above_max_job_pixels": int((box > 65536).sum())}
        for tag, L, ds in CONFIGS:
            tkw = {"levels": L, "distance": ds}
            got = tx.texture_instances(r, img_d, **tkw)
            assert np.array_equal(got.counts, host_route(r.labels, r.table, img, L, ds))     # both routes give the same matrices
            t = {k: [] for k in ("device", "host", "pred", "pred_t")}
            for _ in range(a.reps):
                t["pred"].append(wall(lambda: tiling.predict_tiled(model, img_d, **kw)))
                t["pred_t"].append(wall(lambda: tiling.predict_tiled(model, img_d, texture=tkw, **kw)))
                t["device"].append(wall(lambda: tx.texture_instances(r, img_d, **tkw)))
                t["host"].append(wall(lambda: host_route(r.labels, r.table, img, L, ds)))
            med = {k: float(np.median(v)) for k, v in t.items()}
            row[tag] = {"a_texture_instances": stat(t["device"]), "a_host_route": stat(t["host"]), "a_host_over_device": round(med["host"] / med["device"], 3),
                        "b_predict_tiled": stat(t["pred"]), "b_predict_tiled_texture": stat(t["pred_t"]),
                        "b_texture_over_plain": round(med["pred_t"] / med["pred"], 4),
                        "c_kernel": kernels(r.labels[None], jobs, img_d[None], L, ds, a.reps),
                        "worst_constant_kernel": kernels(r.labels[None], jobs, torch.full_like(img_d, 93)[None], L, ds, a.reps)}
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
