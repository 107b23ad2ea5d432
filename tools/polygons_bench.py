#!/usr/bin/env python
"""Polygon annotations to a device label map on one MI355X -> profiles/polygons_bench.json.

Inputs: the calibrated weights and seeded uint8 images of 1040 x 1388 and 2048 x 2048 (tile 512, overlap 128, 8 tiles per predict call);
the polygons are polygons.from_contours of the predict_tiled(contours=True) result.  Per image, in alternating windows of one warmed-up
process:
  a  polygons.fill end to end (wall clock around a synchronisation) and its three stages apart: edge_table, tile_lists (both host only)
     and upload + launch (upload_tables + fill_tables)
  b  the route a user has today: PIL ImageDraw.polygon per instance into a host map (outer rings with the id, holes with 0; PIL's own edge
     rule, so the map differs along the outlines) plus the upload.  cv2 and skimage are not installed where this was measured
  c  polygons.fill_host
  d  kg_polygons_fill alone (device events over ten back-to-back calls; tables on the device), without and with cover, next to a
     device-to-device copy of the map it writes
and the stated worst cases (fill as wall clock, the kernel by device events, the PIL route where it applies):
  giant_part      ONE part of about 5000 edges that covers the whole 2048 x 2048 map: every tile stages every chunk
  stacked_discs   2000 discs of 64 edges stacked on one tile
  pixel_squares   a 512 x 512 map of one-pixel squares: 262 144 rows
Every figure is the median of the repeats with their minimum and maximum.

    python tools/polygons_bench.py [--sizes 1040x1388,2048x2048] [--reps 5] [--out profiles/polygons_bench.json]
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

from kg_instance_segmentation_amd import KGnet, ops, tiling  # noqa: E402
from kg_instance_segmentation_amd import polygons as pg  # noqa: E402

try:
    from PIL import Image, ImageDraw
except ImportError:                                                   # the file says so
    Image = None


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


def pil_route(p, H, W, dev):
    """ImageDraw.polygon per instance into an int32 host map, then the upload.  A ring is an outer ring when its shoelace area is
    positive on the screen (the orientation contours.py gives), else a hole, drawn with 0 after the outer rings of its row."""
    im = Image.new("I", (W, H), 0)
    draw = ImageDraw.Draw(im)
    for k in range(len(p)):
        rings = [r for part in p.of(k) for r in part if len(r) >= 3]
        area = [float(np.sum(r[:, 0] * np.roll(r[:, 1], -1) - np.roll(r[:, 0], -1) * r[:, 1])) for r in rings]
        for r, a2 in sorted(zip(rings, area), key=lambda ra: ra[1] <= 0):
            draw.polygon(r.reshape(-1).tolist(), fill=k + 1 if a2 > 0 else 0)
    return ops.h2d(np.asarray(im, np.int32), dev)


def kernel_alone(p, H, W, dev, reps, inner=10):
    edges, items, tile_ptr, nimg = pg.tables(p, H, W)
    de, di, dp = pg.upload_tables(edges, items, tile_ptr, dev)
    out, cover = torch.empty(1, H, W, dtype=torch.int32, device=dev), torch.empty(1, H, W, dtype=torch.int32, device=dev)
    t = {"copy": [], "fill": [], "fill_cover": []}
    for _ in range(reps):
        t["copy"].append(events(lambda: cover.copy_(out), inner))
        t["fill"].append(events(lambda: pg.fill_tables(de, di, dp, 1, H, W, 0, out=out), inner))
        t["fill_cover"].append(events(lambda: pg.fill_tables(de, di, dp, 1, H, W, 0, out=out, cover=cover), inner))
    med = {k: float(np.median(v)) for k, v in t.items()}
    per_tile = np.diff(tile_ptr)
    return {"edges": len(edges), "items": len(items), "tiles": len(per_tile), "items_per_tile_max": int(per_tile.max()),
            "copy_of_the_map": stat(t["copy"]), "polygons_fill": stat(t["fill"]), "polygons_fill_with_cover": stat(t["fill_cover"]),
            "fill_to_map_copy": round(med["fill"] / med["copy"], 3), "fill_with_cover_to_map_copy": round(med["fill_cover"] / med["copy"], 3)}


def stages(p, H, W, dev, reps, with_host, with_pil):
    """The windows a .. c of one polygon set -> a dict of stats"""
    t = {k: [] for k in ("fill", "edge_table", "tile_lists", "upload_launch", "pil", "host")}
    values, rows, pimg, nimg = pg._per_part("bench", p, None, None, None)
    for _ in range(reps):
        t["fill"].append(wall(lambda: pg.fill(p, H, W, dev)))
        t0 = time.perf_counter()
        edges, ranges, boxes = pg.edge_table(p)
        t1 = time.perf_counter()
        items, tile_ptr = pg.tile_lists(ranges, boxes, values, rows, H, W, pimg, nimg)
        t2 = time.perf_counter()
        t["edge_table"].append((t1 - t0) * 1e3); t["tile_lists"].append((t2 - t1) * 1e3)
        t["upload_launch"].append(wall(lambda: pg.fill_tables(*pg.upload_tables(edges, items, tile_ptr, dev), 1, H, W)))
        if with_pil and Image is not None:
            t["pil"].append(wall(lambda: pil_route(p, H, W, dev)))
        if with_host:
            t["host"].append(wall(lambda: pg.fill_host(p, H, W)))
    out = {"a_fill": stat(t["fill"]), "a_edge_table": stat(t["edge_table"]), "a_tile_lists": stat(t["tile_lists"]),
           "a_upload_and_launch": stat(t["upload_launch"])}
    if t["pil"]:
        out["b_pil_route"] = stat(t["pil"])
        out["b_pil_over_fill"] = round(float(np.median(t["pil"]) / np.median(t["fill"])), 3)
    elif with_pil:
        out["b_pil_route"] = "PIL does not import here"
    if t["host"]:
        out["c_fill_host"] = stat(t["host"])
    return out


def worst_cases(dev, reps):
    out = {}

    def case(name, p, H, W, with_pil, check_host):
        got = pg.fill(p, H, W, dev)
        if check_host:
            assert np.array_equal(got.cpu().numpy(), pg.fill_host(p, H, W))
        out[name] = {"map": [H, W], "rows": len(p), **stages(p, H, W, dev, reps, False, with_pil), **{"d_" + k: v for k, v in
                                                                                                      kernel_alone(p, H, W, dev, reps, inner=3).items()}}
        print(name, json.dumps(out[name]), file=sys.stderr, flush=True)
    S = 2048
    n = 5000                                                          # a saw-toothed rim just outside the map: every centre is inside
    a = 2 * np.pi * np.arange(n) / n + 0.05
    r = np.where(np.arange(n) % 2 == 0, 1.6, 1.5) * S
    case("giant_part_5000_edges_over_2048", pg.from_rings([[[np.stack([S / 2 + r * np.cos(a), S / 2 + r * np.sin(a)], 1)]]]), S, S, True, False)
    rng = np.random.default_rng(0)
    ang = 2 * np.pi * np.arange(64) / 64 + 0.05
    discs = [[[np.stack([96 + rng.uniform(-3, 3) + 12 * np.cos(ang), 48 + rng.uniform(-3, 3) + 12 * np.sin(ang)], 1)]] for _ in range(2000)]
    stacked = pg.from_rings(discs)
    assert int((np.diff(pg.tables(stacked, 256, 256)[2]) > 0).sum()) == 1         # one tile holds them all
    case("stacked_2000_discs_on_one_tile", stacked, 256, 256, True, True)
    S = 512
    yy, xx = np.mgrid[0:S, 0:S]
    x, y = xx.reshape(-1).astype(np.float64), yy.reshape(-1).astype(np.float64)
    verts = np.stack([np.stack([x, y], 1), np.stack([x + 1, y], 1), np.stack([x + 1, y + 1], 1), np.stack([x, y + 1], 1)], 1).reshape(-1, 2)
    m = S * S
    squares = pg.Polygons(np.arange(m + 1), np.arange(m + 1), 4 * np.arange(m + 1), verts)
    got = pg.fill(squares, S, S, dev)
    assert torch.equal(got, torch.arange(1, m + 1, dtype=torch.int32, device=dev).view(S, S))
    case("pixel_squares_512_262144_rows", squares, S, S, False, False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1040x1388,2048x2048")
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polygons_bench.json"))
    a = ap.parse_args()
    from oracle import weightgen
    dev = torch.device("cuda", 0)
    model = KGnet.resnet50(pretrained=False)
    model.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    model = model.to(dev).eval()
    kw = dict(tile=a.tile, overlap=a.overlap, batch=a.batch)
    res = {"probe": "polygons_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps, "tile": a.tile, "overlap": a.overlap, "batch": a.batch,
           "host_route": "PIL %s ImageDraw.polygon per instance + upload (cv2 / skimage not installed)" % Image.__version__ if Image else
           "PIL does not import here: no host rasteriser measured",
           "units": "ms (a, b, c: wall clock around a synchronisation; d: device events over back-to-back calls)",
           "not_measured": "the split of the kernel's time between staging, the crossing tests and the list walk", "configs": []}
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        img_d = torch.from_numpy(np.random.default_rng(H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
        r = tiling.predict_tiled(model, img_d, contours=True, **kw)           # (also the warm-up)
        p = pg.from_contours(r.contours)
        assert torch.equal(pg.fill(p, H, W, dev), r.labels)                   # the round trip is exact
        assert np.array_equal(pg.fill_host(p, H, W), r.labels.cpu().numpy())
        row = {"image": [H, W], "instances": len(r), "rings": len(p.vert_ptr) - 1, "map_bytes": 4 * H * W}
        if Image is not None:
            row["b_pil_pixels_that_differ"] = int((pil_route(p, H, W, dev) != r.labels).sum().item())
        row.update(stages(p, H, W, dev, a.reps, True, True))
        row.update({"d_" + k: v for k, v in kernel_alone(p, H, W, dev, a.reps).items()})
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
