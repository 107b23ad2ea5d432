#!/usr/bin/env python
"""The touching-neighbour graph on one MI355X -> profiles/neighbours_bench.json.

Inputs: the calibrated weights and seeded uint8 images of 1040 x 1388 and 2048 x 2048 (tile 512, overlap 128, 8 tiles per predict call).
Per image, for connectivity 4 and 8, with and without expand=8, in alternating windows of one warmed-up process:
  a  neighbours.neighbours_instances on the predict_tiled result (wall clock around a synchronisation) against the host route a user has
     today: the map copied back, shifted comparisons (down and right, and the two diagonals under connectivity 8), np.unique over the
     pair keys.  With expand=8 both routes start from the same device map: the device route expands it inside the call, the host route
     gets the expanded map from distance.expand_labels and copies that back.
  b  kg_label_neighbours alone (device events; jobs already on the device, rows left there, 16 slots), next to a device-to-device copy of
     the map
  c  predict_tiled(neighbours=True) against predict_tiled() in the same process (connectivity 4, no expansion)
and the stated worst cases, on synthetic maps (wall clock, and the number of launches):
  hub           one 250 x 250 instance ringed by 1000 single pixels of distinct ids: 1000 neighbours, rounds of launches
  checkerboard  512 x 512 pixels of distinct ids: 262144 one-pixel jobs of 4 (8) neighbours each
Every figure is the median of the repeats with their minimum and maximum.

    python tools/neighbours_bench.py [--sizes 1040x1388,2048x2048] [--reps 5] [--out profiles/neighbours_bench.json]
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
from kg_instance_segmentation_amd import neighbours as nb  # noqa: E402


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


def host_route(lab, connectivity):
    """Undirected pairs (a < b) with their side and corner counts from a host map: shifted comparisons and np.unique over the pair keys"""
    lab = lab.astype(np.int64)
    top = int(lab.max()) + 1

    def keys(shifts):
        ks = []
        for a, b in shifts:
            sel = (a != b) & (a != 0) & (b != 0)
            ks.append(np.minimum(a[sel], b[sel]) * top + np.maximum(a[sel], b[sel]))
        return np.unique(np.concatenate(ks), return_counts=True)
    sk, sc = keys([(lab[:-1], lab[1:]), (lab[:, :-1], lab[:, 1:])])
    if connectivity == 8:
        ck, cc = keys([(lab[:-1, :-1], lab[1:, 1:]), (lab[:-1, 1:], lab[1:, :-1])])
    else:
        ck, cc = sk[:0], sc[:0]
    k = np.union1d(sk, ck)
    out = np.zeros((len(k), 4), np.int64)
    out[:, 0], out[:, 1] = k // top, k % top
    out[np.searchsorted(k, sk), 2] = sc
    out[np.searchsorted(k, ck), 3] = cc
    return out


def counted(fn):
    """fn() with the kg_label_neighbours launches counted"""
    real, calls = nb.neighbours_rows, []

    def rows(*a, **k):
        calls.append(1)
        return real(*a, **k)
    nb.neighbours_rows = rows
    try:
        return fn(), len(calls)
    finally:
        nb.neighbours_rows = real


def worst_cases(dev, reps):
    out = {}
    S = 250
    lab = np.zeros((S + 2, S + 2), np.int32)
    lab[1:-1, 1:-1] = 1
    ring = [(0, x) for x in range(1, S + 1)] + [(S + 1, x) for x in range(1, S + 1)] + [(y, 0) for y in range(1, S + 1)] + [(y, S + 1) for y in range(1, S + 1)]
    for k, (y, x) in enumerate(ring):
        lab[y, x] = 2 + (k * 7919) % 1000
    d = torch.from_numpy(lab).to(dev)
    job = np.array([[0, 1, 0, 0, S + 2, S + 2]])
    want = nb.neighbours_host(lab, job)
    assert want.degree().tolist() == [1000]
    for slots in (16, 64):
        got, launches = counted(lambda: nb.neighbours(d, jobs=job, slots=slots))
        assert got == want
        out[f"hub_1000_neighbours_slots_{slots}"] = {"launches": launches, "wall": stat([wall(lambda: nb.neighbours(d, jobs=job, slots=slots)) for _ in range(reps)])}
    S = 512
    lab = np.arange(1, S * S + 1, dtype=np.int32).reshape(S, S)
    d = torch.from_numpy(lab).to(dev)
    ys, xs = np.divmod(np.arange(S * S), S)
    jobs = np.stack([np.zeros(S * S, np.int64), np.arange(1, S * S + 1), ys, xs, ys + 1, xs + 1], 1)
    table = torch.from_numpy(np.concatenate([jobs, np.zeros((S * S, 2), np.int64)], 1).astype(np.int32)).to(dev)
    for c in (4, 8):
        got, launches = counted(lambda: nb.neighbours(d, jobs=jobs, connectivity=c))
        assert got.degree().sum() == (4 * S * S - 4 * S if c == 4 else 8 * S * S - 12 * S + 4) and got.degree().max() == c
        out[f"checkerboard_512_connectivity_{c}"] = {"jobs": S * S, "launches": launches,
                                                     "wall": stat([wall(lambda: nb.neighbours(d, jobs=jobs, connectivity=c)) for _ in range(reps)]),
                                                     "kernel": stat([events(lambda: nb.neighbours_rows(d, table, 16, c)) for _ in range(reps)])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1040x1388,2048x2048")
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--expand", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbours_bench.json"))
    a = ap.parse_args()
    from oracle import weightgen
    dev = torch.device("cuda", 0)
    model = KGnet.resnet50(pretrained=False)
    model.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    model = model.to(dev).eval()
    kw = dict(tile=a.tile, overlap=a.overlap, batch=a.batch)
    res = {"probe": "neighbours_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps, "tile": a.tile, "overlap": a.overlap, "batch": a.batch,
           "expand": a.expand, "slots": 16, "units": "ms (a, c, worst cases: wall clock around a synchronisation; b, kernel: device events)", "configs": []}
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        img_d = torch.from_numpy(np.random.default_rng(H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
        r = tiling.predict_tiled(model, img_d, **kw)                          # (also the warm-up)
        n = len(r)
        copy_to = torch.empty_like(r.labels)
        row = {"image": [H, W], "instances": n, "map_bytes": 4 * H * W, "graphs": []}
        legs = [(c, e) for c in (4, 8) for e in (None, a.expand)]
        maps = {None: r.labels, a.expand: dt.expand_labels(r.labels, a.expand)}
        tables = {}
        for c, e in legs:
            g, launches = counted(lambda: nb.neighbours_instances(r, connectivity=c, expand=e))
            assert np.array_equal(g.pairs(), host_route(maps[e].cpu().numpy(), c))             # both routes find the same pairs and counts
            jobs = nb._instance_jobs(r, 0, 0 if e is None else e, H, W)
            tables[(c, e)] = torch.from_numpy(np.concatenate([jobs, np.zeros((n, 2), np.int64)], 1).astype(np.int32)).to(dev)
            row["graphs"].append({"connectivity": c, "expand": e, "pairs": len(g.pairs()), "max_degree": int(g.degree().max()) if n else 0,
                                  "mean_degree": round(float(g.degree().mean()), 2) if n else 0, "launches": launches})
        t = {(k, c, e): [] for k in ("device", "host", "kernel") for c, e in legs}
        t.update({k: [] for k in ("pred", "pred_neighbours", "copy")})
        for _ in range(a.reps):
            t["pred"].append(wall(lambda: tiling.predict_tiled(model, img_d, **kw)))
            t["pred_neighbours"].append(wall(lambda: tiling.predict_tiled(model, img_d, neighbours=True, **kw)))
            t["copy"].append(events(lambda: copy_to.copy_(r.labels)))
            for c, e in legs:
                t[("device", c, e)].append(wall(lambda: nb.neighbours_instances(r, connectivity=c, expand=e)))
                src = (lambda: r.labels) if e is None else (lambda: dt.expand_labels(r.labels, e))
                t[("host", c, e)].append(wall(lambda: host_route(src().cpu().numpy(), c)))
                t[("kernel", c, e)].append(events(lambda: nb.neighbours_rows(maps[e], tables[(c, e)], 16, c)))
        med = {k: float(np.median(v)) for k, v in t.items()}
        for gr in row["graphs"]:
            c, e = gr["connectivity"], gr["expand"]
            gr.update({"a_neighbours_instances": stat(t[("device", c, e)]), "a_host_route": stat(t[("host", c, e)]),
                       "a_host_over_device": round(med[("host", c, e)] / med[("device", c, e)], 3),
                       "b_label_neighbours": stat(t[("kernel", c, e)]), "b_ratio_to_map_copy": round(med[("kernel", c, e)] / med["copy"], 3)})
        row.update({"b_copy_of_the_map": stat(t["copy"]), "c_predict_tiled": stat(t["pred"]), "c_predict_tiled_neighbours": stat(t["pred_neighbours"]),
                    "c_neighbours_over_plain": round(med["pred_neighbours"] / med["pred"], 4)})
        print(json.dumps(row), file=sys.stderr, flush=True)
        res["configs"].append(row)
        del r, img_d, maps, tables, copy_to
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
