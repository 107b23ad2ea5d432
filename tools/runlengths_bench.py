#!/usr/bin/env python
"""Run-length lists on one MI355X -> profiles/runlengths_bench.json.

Inputs: the calibrated weights and seeded uint8 images of 1040 x 1388 and 2048 x 2048 (tile 512, overlap 128, 8 tiles per predict call).
Per image, in alternating windows of one warmed-up process:
  a  runlengths.runs_instances on the predict_tiled result (wall clock around a synchronisation) against the route a user has without
     it: labels.cpu().numpy() followed by instances.rle_encode over the ids 1 .. n
  b  runlengths.paint of those runs (wall clock) against instances.rle_decode of the same dict followed by an upload of the map
  c  predict_tiled(runs=True) against predict_tiled() in the same process
  d  kg_label_run_counts, kg_label_runs and kg_runs_paint alone (device events; tables already on the device, rows left there), next to a
     device-to-device copy of the map
and the stated worst cases, on synthetic maps (runs as wall clock, both kernels by device events):
  stripes       ONE instance whose every pixel is its own run: horizontal stripes one pixel high over a 250 x 250 box
  checkerboard  512 x 512 pixels of two values: two jobs of 131072 one-pixel runs each, in column bands of 65536 pixels
Every figure is the median of the repeats with their minimum and maximum.

    python tools/runlengths_bench.py [--sizes 1040x1388,2048x2048] [--reps 5] [--out profiles/runlengths_bench.json]
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

from kg_instance_segmentation_amd import KGnet, instances, tiling  # noqa: E402
from kg_instance_segmentation_amd import runlengths as rl  # noqa: E402
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


def device_tables(lab, jobs, dev, max_job_pixels=65536):
    """The two job tables of the raw entries, on the device, and R"""
    pieces, _ = rl.split_columns(jobs, max_job_pixels)
    cnt = rl.run_counts(lab, pieces).cpu().numpy().astype(np.int64)
    table = np.concatenate([pieces.astype(np.int64), np.cumsum(cnt, 0) - cnt], 1)
    return torch.from_numpy(pieces).to(dev), torch.from_numpy(table.astype(np.int32)).to(dev), int(cnt[:, 0].sum())


def kernels(lab, jobs, dev, reps):
    cnt_table, row_table, R = device_tables(lab[None] if lab.dim() == 2 else lab, jobs, dev)
    out = torch.empty(R, 2, dtype=torch.int32, device=dev)
    return {"pieces": len(cnt_table), "runs": R,
            "label_run_counts": stat([events(lambda: rl.run_counts(lab, cnt_table)) for _ in range(reps)]),
            "label_runs": stat([events(lambda: rl.run_rows(lab, row_table, R, out)) for _ in range(reps)])}


def worst_cases(dev, reps):
    out = {}
    S = 250
    lab = np.zeros((S + 2, S + 2), np.int32)
    lab[1:-1:2, 1:-1] = 1
    d = torch.from_numpy(lab).to(dev)
    job = np.array([[0, 1, 1, 1, S + 1, S + 1]])
    want = rl.runs_host(lab, job)
    assert want.counts().tolist() == [S * S // 2] and rl.runs(d, jobs=job) == want
    out["stripes_250_one_instance"] = {"wall_runs": stat([wall(lambda: rl.runs(d, jobs=job)) for _ in range(reps)]),
                                       "wall_host_route": stat([wall(lambda: instances.rle_encode(d.cpu().numpy(), ids=[1])) for _ in range(reps)]),
                                       **kernels(d, job, dev, reps)}
    S = 512
    lab = ((np.add.outer(np.arange(S), np.arange(S)) % 2) + 1).astype(np.int32)
    d = torch.from_numpy(lab).to(dev)
    jobs = np.array([[0, 1, 0, 0, S, S], [0, 2, 0, 0, S, S]])
    got = rl.runs(d, jobs=jobs)
    assert got == rl.runs_host(lab, jobs) and got.counts().sum() == S * S - (S - 1)
    out["checkerboard_512_two_values"] = {"wall_runs": stat([wall(lambda: rl.runs(d, jobs=jobs)) for _ in range(reps)]),
                                          "wall_host_route": stat([wall(lambda: instances.rle_encode(d.cpu().numpy(), ids=[1, 2])) for _ in range(reps)]),
                                          **kernels(d, jobs, dev, reps)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1040x1388,2048x2048")
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "runlengths_bench.json"))
    a = ap.parse_args()
    from oracle import weightgen
    dev = torch.device("cuda", 0)
    model = KGnet.resnet50(pretrained=False)
    model.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    model = model.to(dev).eval()
    kw = dict(tile=a.tile, overlap=a.overlap, batch=a.batch)
    res = {"probe": "runlengths_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps, "tile": a.tile, "overlap": a.overlap, "batch": a.batch,
           "units": "ms (a, b, c, wall_*: wall clock around a synchronisation; d and the worst cases' kernels: device events)", "configs": []}
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        img_d = torch.from_numpy(np.random.default_rng(H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
        r = tiling.predict_tiled(model, img_d, **kw)                          # (also the warm-up)
        n = len(r)
        ids = range(1, n + 1)

        def host_encode():
            return instances.rle_encode(r.labels.cpu().numpy(), ids=ids)

        def host_decode(enc):
            return torch.from_numpy(instances.rle_decode(enc, H, W)).to(dev)
        runs = rl.runs_instances(r)
        enc = host_encode()
        assert all(np.array_equal(runs.of(k), enc[k + 1]) for k in range(n))                    # both routes give the same lists
        assert torch.equal(rl.paint(runs, H, W, dev), r.labels) and torch.equal(host_decode(enc), r.labels)
        jobs = instance_jobs(r, 0, 0, H, W)
        cnt_table, row_table, R = device_tables(r.labels[None], jobs, dev)
        rows_out = torch.empty(R, 2, dtype=torch.int32, device=dev)
        paint_rows = torch.from_numpy(rl._paint_rows("bench", runs, H, W, None)[0].astype(np.int32)).to(dev)
        paint_out, copy_to = torch.empty_like(r.labels), torch.empty_like(r.labels)
        from kg_instance_segmentation_amd._lib import call, ptr, stream_ptr
        row = {"image": [H, W], "instances": n, "runs": R, "map_bytes": 4 * H * W, "pieces": len(cnt_table)}
        t = {k: [] for k in ("device", "host", "paint", "decode", "pred", "pred_runs", "copy", "counts", "rows", "paint_kernel")}
        for _ in range(a.reps):
            t["pred"].append(wall(lambda: tiling.predict_tiled(model, img_d, **kw)))
            t["pred_runs"].append(wall(lambda: tiling.predict_tiled(model, img_d, runs=True, **kw)))
            t["device"].append(wall(lambda: rl.runs_instances(r)))
            t["host"].append(wall(host_encode))
            t["paint"].append(wall(lambda: rl.paint(runs, H, W, dev)))
            t["decode"].append(wall(lambda: host_decode(enc)))
            t["copy"].append(events(lambda: copy_to.copy_(r.labels)))
            t["counts"].append(events(lambda: rl.run_counts(r.labels, cnt_table)))
            t["rows"].append(events(lambda: rl.run_rows(r.labels, row_table, R, rows_out)))
            t["paint_kernel"].append(events(lambda: call("kg_runs_paint", ptr(paint_rows), len(paint_rows), H, W, 0, ptr(paint_out), stream_ptr())))
        med = {k: float(np.median(v)) for k, v in t.items()}
        row.update({"a_runs_instances": stat(t["device"]), "a_host_route": stat(t["host"]), "a_host_over_device": round(med["host"] / med["device"], 3),
                    "b_paint": stat(t["paint"]), "b_rle_decode_and_upload": stat(t["decode"]), "b_host_over_device": round(med["decode"] / med["paint"], 3),
                    "c_predict_tiled": stat(t["pred"]), "c_predict_tiled_runs": stat(t["pred_runs"]), "c_runs_over_plain": round(med["pred_runs"] / med["pred"], 4),
                    "d_copy_of_the_map": stat(t["copy"]), "d_label_run_counts": stat(t["counts"]), "d_label_runs": stat(t["rows"]),
                    "d_runs_paint": stat(t["paint_kernel"]), "d_both_run_kernels_to_map_copy": round((med["counts"] + med["rows"]) / med["copy"], 3),
                    "d_paint_to_map_copy": round(med["paint_kernel"] / med["copy"], 3)})
        print(json.dumps(row), file=sys.stderr, flush=True)
        res["configs"].append(row)
        del r, img_d, copy_to, paint_out
        torch.cuda.empty_cache()
    res["worst_cases"] = worst_cases(dev, a.reps)
    print(json.dumps(res["worst_cases"]), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
