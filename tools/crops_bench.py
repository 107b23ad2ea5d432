#!/usr/bin/env python
"""Instance crops (fixed-size patches and masks per id) on one MI355X -> profiles/crops_bench.json.

Inputs: the calibrated weights and seeded uint8 images of 1040 x 1388 and 2048 x 2048 (tile 512, overlap 128, 8 tiles per predict call),
the 3-channel uint8 source image as the image to crop; 64 x 64 patches, the default square window.  Per image, in alternating windows of
one warmed-up process:
  a  crops.crops_instances on the predict_tiled result against its uploaded image (wall clock around a synchronisation), against the
     route a user has today: the map and the image copied back, scipy.ndimage.find_objects, per id the box slice resized with PIL
     (bilinear for the image, nearest for the mask) -- and, separately, with scipy.ndimage.zoom(order=1) --, stacked and uploaded; and
     against the device route in torch: a per-instance loop of slice + F.interpolate, and ONE batched F.affine_grid + F.grid_sample over
     a float copy of the image.  Neither torch route has the mask or a defined edge rule (a window over the frame is clamped or
     zero-padded as torch decides), and the host route resizes the box anisotropically without context: they are what the time is
     compared with, not what the pixels are compared with.
  b  predict_tiled(crops=True) against predict_tiled without it in the same process
  c  kg_label_crops alone (device events over ten back-to-back calls; table and image already on the device, outputs left there), next
     to a device-to-device copy of the bytes it writes (patches and masks)
and the stated worst cases, kernel by device events next to the copy of the bytes written:
  wide_window   2000-pixel windows down to 32 x 32 on a 2048 x 2048 map: every tap is its own cache line
  large_output  256 jobs at 256 x 256 with four uint16 channels
  one_pixel     512 x 512 distinct ids: 262 144 one-pixel jobs at 8 x 8
Every figure is the median of the repeats with their minimum and maximum.

    python tools/crops_bench.py [--sizes 1040x1388,2048x2048] [--reps 5] [--out profiles/crops_bench.json]
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
import torch.nn.functional as F  # noqa: E402

from kg_instance_segmentation_amd import KGnet, _labelmaps, tiling  # noqa: E402
from kg_instance_segmentation_amd import crops as cr  # noqa: E402
from kg_instance_segmentation_amd import measure as ms  # noqa: E402

try:
    from scipy import ndimage as ndi  # noqa: E402
except ImportError:
    ndi = None
try:
    from PIL import Image  # noqa: E402
except ImportError:
    Image = None

SIZE = 64


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


def boxes_of(lab, table):
    n = len(table)
    if ndi is not None:
        return ndi.find_objects(lab, max_label=n)
    return [(slice(int(t[2]), int(t[4])), slice(int(t[3]), int(t[5]))) if t[1] > 0 else None for t in table]


def host_route(lab_d, img_d, table, dev, resize):
    """What a user does today: map and image copied back, the boxes of the ids, per id the box slice resized, stacked, uploaded"""
    lab, img = lab_d.cpu().numpy(), img_d.cpu().numpy()
    n, C = len(table), img.shape[2]
    patches, masks = np.zeros((n, SIZE, SIZE, C), np.uint8), np.zeros((n, SIZE, SIZE), np.uint8)
    for k, sl in enumerate(boxes_of(lab, table)):
        if sl is None:
            continue
        px, mk = img[sl], (lab[sl] == k + 1).astype(np.uint8)
        if resize == "pil":
            patches[k] = np.asarray(Image.fromarray(px).resize((SIZE, SIZE), Image.BILINEAR))
            masks[k] = np.asarray(Image.fromarray(mk).resize((SIZE, SIZE), Image.NEAREST))
        else:
            h, w = mk.shape
            patches[k] = ndi.zoom(px, (SIZE / h, SIZE / w, 1), order=1, grid_mode=True, mode="nearest")
            masks[k] = ndi.zoom(mk, (SIZE / h, SIZE / w), order=0, grid_mode=True, mode="nearest")
    return torch.from_numpy(np.ascontiguousarray(patches.transpose(0, 3, 1, 2))).to(dev), torch.from_numpy(masks).to(dev)


def torch_loop(img_f, table):
    """the device route in torch, per instance: the box slice of a float copy + F.interpolate (no mask, the box without context)"""
    out = [F.interpolate(img_f[:, :, int(t[2]):int(t[4]), int(t[3]):int(t[5])], size=(SIZE, SIZE), mode="bilinear", align_corners=False)
           for t in table if t[1] > 0]
    return torch.cat(out) if out else img_f.new_zeros((0, img_f.shape[1], SIZE, SIZE))


def torch_grid(img_f, table, dev):
    """the device route in torch, batched: one F.affine_grid + F.grid_sample over the float image (no mask, zero padding)"""
    t = np.asarray(table, np.float64)
    t = t[t[:, 1] > 0]
    H, W = img_f.shape[2:]
    side = np.maximum(t[:, 4] - t[:, 2], t[:, 5] - t[:, 3])
    cy, cx = (t[:, 2] + t[:, 4]) / 2, (t[:, 3] + t[:, 5]) / 2
    theta = np.zeros((len(t), 2, 3), np.float32)
    theta[:, 0, 0], theta[:, 0, 2] = side / W, 2 * cx / W - 1
    theta[:, 1, 1], theta[:, 1, 2] = side / H, 2 * cy / H - 1
    grid = F.affine_grid(torch.from_numpy(theta).to(dev), (len(t), img_f.shape[1], SIZE, SIZE), align_corners=False)
    return F.grid_sample(img_f.expand(len(t), -1, -1, -1), grid, mode="bilinear", padding_mode="zeros", align_corners=False)


def kernel(lab, img, table, size, reps, mode="linear", masked=False, inner=10):
    """device events of kg_label_crops alone and of a device-to-device copy of the bytes it writes"""
    OH, OW = size
    jd = _labelmaps.upload_jobs(table, lab.device)
    flags = cr._flags("crops_bench", mode, masked)
    p, k = cr._launch(lab, img, jd, OH, OW, flags, 0, True)
    nbytes = p.numel() * p.element_size() + k.numel()
    bufs = (torch.empty(nbytes, dtype=torch.uint8, device=lab.device), torch.empty(nbytes, dtype=torch.uint8, device=lab.device))
    del p, k
    t = {"crops": [], "copy": []}
    for _ in range(reps):
        t["crops"].append(events(lambda: cr._launch(lab, img, jd, OH, OW, flags, 0, True), inner))
        t["copy"].append(events(lambda: bufs[1].copy_(bufs[0]), inner))
    med = {k: float(np.median(v)) for k, v in t.items()}
    return {"jobs": int(len(table)), "size": [OH, OW], "channels": int(img.shape[3]), "elem_bytes": int(img.element_size()), "mode": mode,
            "bytes_written": int(nbytes), "label_crops": stat(t["crops"]), "copy_of_those_bytes": stat(t["copy"]),
            "written_GBps": round(nbytes / med["crops"] / 1e6, 1), "copy_GBps": round(nbytes / med["copy"] / 1e6, 1),
            "crops_over_copy": round(med["crops"] / med["copy"], 3)}


def worst_cases(dev, reps):
    out = {}
    rng = np.random.default_rng(11)
    S = 2048
    lab = torch.from_numpy(rng.integers(0, 50, (1, S, S)).astype(np.int32)).to(dev)
    img3 = torch.from_numpy(rng.integers(0, 256, (1, S, S, 3), dtype=np.uint8)).to(dev)
    m = 1024
    y1, x1 = rng.integers(0, 48, m), rng.integers(0, 48, m)
    boxes = np.stack([np.zeros(m, np.int64), rng.integers(0, 50, m), y1, x1, y1 + 2000, x1 + 2000], 1)
    out["wide_window_2000_to_32"] = kernel(lab, img3, cr.affine_jobs(boxes, 32), (32, 32), reps, inner=3)
    img4 = torch.from_numpy(rng.integers(0, 65536, (1, S, S, 4)).astype(np.uint16).view(np.int16)).to(dev)
    m = 256
    y1, x1 = rng.integers(0, S - 256, m), rng.integers(0, S - 256, m)
    boxes = np.stack([np.zeros(m, np.int64), rng.integers(0, 50, m), y1, x1, y1 + 256, x1 + 256], 1)
    out["large_output_256_jobs_256x256_4ch_uint16"] = kernel(lab, img4, cr.affine_jobs(boxes, 256), (256, 256), reps, inner=3)
    boxes[:, 4:6] = boxes[:, 2:4] + 181                                       # the same outputs from ragged steps: 181 -> 256, turned
    out["large_output_rotated_181_to_256"] = kernel(lab, img4, cr.affine_jobs(boxes, 256, angle=rng.uniform(-3, 3, m), side=181.0), (256, 256), reps, inner=3)
    S = 512
    lab1 = torch.arange(1, S * S + 1, dtype=torch.int32, device=dev).view(1, S, S)
    img1 = torch.from_numpy(rng.integers(0, 256, (1, S, S, 3), dtype=np.uint8)).to(dev)
    yy, xx = np.mgrid[0:S, 0:S]
    boxes = np.stack([np.zeros(S * S, np.int64), np.arange(1, S * S + 1), yy.reshape(-1), xx.reshape(-1), yy.reshape(-1) + 1, xx.reshape(-1) + 1], 1)
    out["one_pixel_262144_jobs_8x8"] = kernel(lab1, img1, cr.affine_jobs(boxes, 8), (8, 8), reps, inner=3)
    for k, v in out.items():
        print(k, json.dumps(v), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1040x1388,2048x2048")
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crops_bench.json"))
    a = ap.parse_args()
    from oracle import weightgen
    dev = torch.device("cuda", 0)
    model = KGnet.resnet50(pretrained=False)
    model.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    model = model.to(dev).eval()
    kw = dict(tile=a.tile, overlap=a.overlap, batch=a.batch)
    res = {"probe": "crops_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps, "tile": a.tile, "overlap": a.overlap, "batch": a.batch,
           "patch": [SIZE, SIZE],
           "host_route": "labels.cpu().numpy() + image.cpu().numpy() + "
                         + ("scipy.ndimage.find_objects" if ndi is not None else "the boxes of the instance table (scipy does not import)")
                         + " + per id the box slice resized (PIL bilinear / nearest; scipy.ndimage.zoom order 1 / 0) + stack + upload",
           "torch_routes": "per-instance slice + F.interpolate; one batched F.affine_grid + F.grid_sample over a float copy of the image."
                           "  Neither has the mask or a defined edge rule",
           "units": "ms (a, b: wall clock around a synchronisation; c and the worst cases: device events over back-to-back calls)",
           "not_measured": ["an LDS-staged source footprint (not built)", "uint16 images outside the worst cases", "mode=\"nearest\" and masked=True",
                            "angle=\"major\" (one more kg_label_measure launch and copy back)", "more than one image per launch",
                            "the split of kg_label_crops' time between the taps, the arithmetic and the stores",
                            "OpenCV's resize on the host route (not installed)", "a second network consuming the patches"],
           "configs": []}
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        img = np.random.default_rng(H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
        img_d = torch.from_numpy(img).to(dev)
        r = tiling.predict_tiled(model, img_d, **kw)                          # (also the warm-up)
        n = len(r)
        table = np.asarray(r.table)
        got = cr.crops_instances(r, img_d, SIZE)
        wp, wm = cr.crops_host(r.labels.cpu().numpy(), got.jobs, img, SIZE)
        assert np.array_equal(got.patches.cpu().numpy(), wp) and np.array_equal(got.masks.cpu().numpy(), wm)     # the device equals the host statement
        img_f = img_d.permute(2, 0, 1)[None].float().contiguous()
        for fn in (lambda: host_route(r.labels, img_d, table, dev, "pil"), lambda: torch_loop(img_f, table), lambda: torch_grid(img_f, table, dev)):
            fn()                                                                # warm-up of every route
        t = {k: [] for k in ("device", "host_pil", "host_zoom", "loop", "grid", "float_copy", "pred", "pred_c")}
        for _ in range(a.reps):
            t["pred"].append(wall(lambda: tiling.predict_tiled(model, img_d, **kw)))
            t["pred_c"].append(wall(lambda: tiling.predict_tiled(model, img_d, crops=True, **kw)))
            t["device"].append(wall(lambda: cr.crops_instances(r, img_d, SIZE)))
            if Image is not None:
                t["host_pil"].append(wall(lambda: host_route(r.labels, img_d, table, dev, "pil")))
            if ndi is not None:
                t["host_zoom"].append(wall(lambda: host_route(r.labels, img_d, table, dev, "zoom")))
            t["float_copy"].append(wall(lambda: img_d.permute(2, 0, 1)[None].float().contiguous()))
            t["loop"].append(wall(lambda: torch_loop(img_f, table)))
            t["grid"].append(wall(lambda: torch_grid(img_f, table, dev)))
        med = {k: float(np.median(v)) for k, v in t.items() if v}
        box = np.maximum(table[:, 4] - table[:, 2], 0) * np.maximum(table[:, 5] - table[:, 3], 0)
        row = {"image": [H, W], "instances": n, "map_bytes": 4 * H * W,
               "median_box_side": round(float(np.sqrt(np.median(box[box > 0]))), 1) if (box > 0).any() else None,
               "a_crops_instances": stat(t["device"]),
               "a_host_route_pil": stat(t["host_pil"]) if t["host_pil"] else None, "a_host_route_zoom": stat(t["host_zoom"]) if t["host_zoom"] else None,
               "a_torch_float_copy_of_the_image": stat(t["float_copy"]), "a_torch_loop_interpolate": stat(t["loop"]),
               "a_torch_batched_grid_sample": stat(t["grid"]),
               "a_host_pil_over_device": round(med["host_pil"] / med["device"], 2) if "host_pil" in med else None,
               "a_host_zoom_over_device": round(med["host_zoom"] / med["device"], 2) if "host_zoom" in med else None,
               "a_torch_loop_over_device": round(med["loop"] / med["device"], 2), "a_torch_grid_over_device": round(med["grid"] / med["device"], 2),
               "b_predict_tiled": stat(t["pred"]), "b_predict_tiled_crops": stat(t["pred_c"]), "b_crops_over_plain": round(med["pred_c"] / med["pred"], 4),
               "c_kernel": kernel(r.labels[None], img_d[None], got.jobs, (SIZE, SIZE), a.reps)}
        print(json.dumps(row), file=sys.stderr, flush=True)
        res["configs"].append(row)
        del r, img_d, img_f, got
        torch.cuda.empty_cache()
    res["worst_cases"] = worst_cases(dev, a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
