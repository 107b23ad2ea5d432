#!/usr/bin/env python
"""Linking label maps on one MI355X -> profiles/linking_bench.json.

Inputs: the calibrated weights and seeded uint8 images of 1040 x 1388 and 2048 x 2048 (tile 512, overlap 128, 8 tiles per predict call).
Frame 0 is predict_tiled's label map; frame t is frame 0 with every instance moved by two pixels down and right t times (torch.roll), so
consecutive frames overlap heavily and every frame holds the same n ids.  Per image, for stacks of 2 and 8 frames, in alternating
windows of one warmed-up process (wall clock around a synchronisation):
  a  linking.track (kg_label_stats per frame, ONE kg_label_overlaps launch for all pairs, host links, one kg_component_remap) against
     - the route a user has today: the stack copied back, and per consecutive pair np.unique over the pair keys of the pixels where
       both maps are non-zero, with np.bincount for the areas (it stops at the pair counts: no links, no relabelled stack);
     - the existing device route at zero shift: labelmetrics.label_stats per frame, then labelmetrics.contingency per pair with those
       tables (it stops at the pair counts too).
     All three find the same pairs and pixel counts (asserted).
  b  kg_label_overlaps alone for the pair (frame 0, frame 1): device events over ten back-to-back calls, jobs already on the device,
     rows left there, 8 slots -- next to a device-to-device copy of the two maps it reads
and the stated worst cases, on synthetic maps (wall clock, and the number of launches):
  wide   one 250 x 250 instance over 1000 distinct partner values: rounds of launches
  tiny   512 x 512 one-pixel jobs, one partner value each
Every figure is the median of the repeats with their minimum and maximum.

    python tools/linking_bench.py [--sizes 1040x1388,2048x2048] [--reps 5] [--out profiles/linking_bench.json]
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

from kg_instance_segmentation_amd import KGnet, _labelmaps, tiling  # noqa: E402
from kg_instance_segmentation_amd import labelmetrics as lm  # noqa: E402
from kg_instance_segmentation_amd import linking as lk  # noqa: E402

SLOTS = 8


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


def host_route(stack_d, n):
    """What a user does today: the stack copied back; per consecutive pair (a, b, pixels) in lexicographic order, and the areas"""
    stack = stack_d.cpu().numpy()
    out = []
    for t in range(len(stack) - 1):
        a, b = stack[t].astype(np.int64), stack[t + 1].astype(np.int64)
        both = (a > 0) & (b > 0)
        key, cnt = np.unique(a[both] * (n + 1) + b[both], return_counts=True)
        out.append((np.stack([key // (n + 1), key % (n + 1), cnt], 1), np.bincount(stack[t + 1].reshape(-1), minlength=n + 1)[1:]))
    return out


def contingency_route(stack_d, n):
    """The existing device route at zero shift: stats per frame, contingency per pair"""
    stats = [lm.label_stats(stack_d[t], n) for t in range(len(stack_d))]
    return [lm.contingency(stack_d[t], stack_d[t + 1], n, n, stats[t], stats[t + 1]) for t in range(len(stack_d) - 1)]


def counted(fn):
    """fn() with the kg_label_overlaps launches counted"""
    real, calls = lk.overlaps_rows, []

    def rows(*a, **k):
        calls.append(1)
        return real(*a, **k)
    lk.overlaps_rows = rows
    try:
        return fn(), len(calls)
    finally:
        lk.overlaps_rows = real


def worst_cases(dev, reps):
    out = {}
    S, K = 250, 1000
    a = np.ones((S, S), np.int32)
    b = (2 + (np.arange(S * S, dtype=np.int64) * 7919) % K).astype(np.int32).reshape(S, S)
    da, db = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    job = np.array([[0, 1, 0, 0, S, S, 0, 0, 0]])
    want = lk.overlaps_host(a, b, job)
    assert len(want.values) == K and want.pixels.sum() == S * S
    for slots in (SLOTS, 64):
        got, launches = counted(lambda: lk.overlaps(da, db, jobs=job, slots=slots))
        assert got == want
        out[f"wide_1000_values_slots_{slots}"] = {"launches": launches, "wall": stat([wall(lambda: lk.overlaps(da, db, jobs=job, slots=slots)) for _ in range(reps)])}
    S = 512
    a = np.arange(1, S * S + 1, dtype=np.int32).reshape(S, S)
    da = torch.from_numpy(a).to(dev)
    db = torch.roll(da, (1, 1), (0, 1)).contiguous()
    ys, xs = np.divmod(np.arange(S * S), S)
    jobs = np.stack([np.zeros(S * S, np.int64), np.arange(1, S * S + 1), ys, xs, ys + 1, xs + 1] + [np.zeros(S * S, np.int64)] * 3, 1)
    table = torch.from_numpy(np.concatenate([jobs, np.zeros((S * S, 2), np.int64)], 1).astype(np.int32)).to(dev)
    got, launches = counted(lambda: lk.overlaps(da, db, jobs=jobs))
    assert np.array_equal(got.values, db.cpu().numpy().reshape(-1)) and (got.pixels == 1).all() and (got.area == 1).all()
    out["tiny_512x512_one_pixel_jobs"] = {"jobs": S * S, "launches": launches, "wall": stat([wall(lambda: lk.overlaps(da, db, jobs=jobs)) for _ in range(reps)]),
                                          "kernel": stat([events(lambda: lk.overlaps_rows(da, db, table, SLOTS)) for _ in range(reps)])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1040x1388,2048x2048")
    ap.add_argument("--frames", default="2,8")
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linking_bench.json"))
    a = ap.parse_args()
    from oracle import weightgen
    dev = torch.device("cuda", 0)
    model = KGnet.resnet50(pretrained=False)
    model.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    model = model.to(dev).eval()
    kw = dict(tile=a.tile, overlap=a.overlap, batch=a.batch)
    res = {"probe": "linking_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps, "tile": a.tile, "overlap": a.overlap, "batch": a.batch,
           "slots": SLOTS, "move_per_frame": [2, 2], "units": "ms (a, worst cases: wall clock around a synchronisation; b, kernel: device events)",
           "configs": []}
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        img_d = torch.from_numpy(np.random.default_rng(H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
        r = tiling.predict_tiled(model, img_d, **kw)
        n = len(r)
        row = {"image": [H, W], "instances": n, "map_bytes": 4 * H * W, "stacks": []}
        for T in (int(v) for v in a.frames.split(",")):
            stack = torch.stack([torch.roll(r.labels, (2 * t, 2 * t), (0, 1)) for t in range(T)]).contiguous()
            counts = [n] * T
            tr, launches = counted(lambda: lk.track(stack, counts, slots=SLOTS))                       # (also the warm-up)
            pairs = [(t, t + 1) for t in range(T - 1)]
            ov = lk.overlaps(stack, stack, counts, pairs=pairs, slots=SLOTS)
            host, cont = host_route(stack, n), contingency_route(stack, n)
            for t in range(T - 1):                                                                      # the three routes count the same pixels
                mine = ov.slice(t * n, (t + 1) * n).pairs()
                assert np.array_equal(mine, host[t][0]) and np.array_equal(mine[:, :2], cont[t].pairs) and np.array_equal(mine[:, 2], cont[t].inter)
            ts = {k: [] for k in ("track", "host", "contingency")}
            for _ in range(a.reps):
                ts["track"].append(wall(lambda: lk.track(stack, counts, slots=SLOTS)))
                ts["host"].append(wall(lambda: host_route(stack, n)))
                ts["contingency"].append(wall(lambda: contingency_route(stack, n)))
            med = {k: float(np.median(v)) for k, v in ts.items()}
            row["stacks"].append({"frames": T, "tracks": len(tr), "pairs_that_meet": len(ov.values), "max_partners": int(np.diff(ov.indptr).max()) if n else 0,
                                  "overlaps_launches": launches, "a_track": stat(ts["track"]), "a_host_route": stat(ts["host"]),
                                  "a_stats_and_contingency": stat(ts["contingency"]), "a_host_over_track": round(med["host"] / med["track"], 3),
                                  "a_contingency_over_track": round(med["contingency"] / med["track"], 3)})
            if T == 2:
                stats = lm.label_stats(stack[0], n)
                jobs = np.concatenate([_labelmaps.jobs_from_stats(stats, 0).astype(np.int64), np.tile([[1, 0, 0, 0, 0]], (n, 1))], 1)
                table = torch.from_numpy(jobs.astype(np.int32)).to(dev)
                copy_to = torch.empty_like(stack)
                tk, tc = [], []
                for _ in range(a.reps):
                    tk.append(events(lambda: lk.overlaps_rows(stack, stack, table, SLOTS)))
                    tc.append(events(lambda: copy_to.copy_(stack)))
                row.update({"b_label_overlaps": stat(tk), "b_copy_of_the_two_maps": stat(tc),
                            "b_ratio_to_copy": round(float(np.median(tk)) / float(np.median(tc)), 3)})
                del copy_to, table
            del stack
        print(json.dumps(row), file=sys.stderr, flush=True)
        res["configs"].append(row)
        del r, img_d
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
