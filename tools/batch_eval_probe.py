#!/usr/bin/env python
"""Batched inference probe: detect_batch ms per image against a loop of detect() on the same head maps, and predict() end-to-end
img/s (float32 host masks as the reference returns them, and device_u8=True), for N in {1, 4, 8, 16} at 512^2 (also 256^2 and
1024^2).  Head maps: bench.eval_inputs (GT-derived, ~300 instances per image, a different seed per image); predict: the calibrated
weights on a random batch.  Prints one JSON line.

    python tools/batch_eval_probe.py [--sizes 512,256,1024] [--ns 1,4,8,16] [--reps 3]
    python tools/batch_eval_probe.py --trace N [--size 512]     one warm-up + one detect_batch of N images (for a kernel-trace run)
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

import bench  # noqa: E402
from kg_instance_segmentation_amd import KGnet, inference, postprocessing as kpp  # noqa: E402


def head_batch(S, n, dev):
    decs = [bench.eval_inputs(S, 300, 500 + i)[0] for i in range(n)]
    return [[torch.from_numpy(np.concatenate([d[l][k] for d in decs], 0)).to(dev) for k in range(3)] for l in range(4)]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,256,1024")
    ap.add_argument("--ns", default="1,4,8,16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--size", type=int, default=512)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    if a.trace:
        dec = head_batch(a.size, a.trace, dev)
        kpp.detect_batch(dec)
        torch.cuda.synchronize()
        kpp.detect_batch(dec)
        torch.cuda.synchronize()
        print(json.dumps({"trace": a.trace, "size": a.size, "detect_batch_calls": 2}))
        return
    from oracle import weightgen
    model = KGnet.resnet50(pretrained=False)
    model.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    model = model.to(dev).eval()
    ns = [int(v) for v in a.ns.split(",")]
    res = {"probe": "batch_eval", "reps": a.reps, "budget_bytes": kpp.BATCH_WORKSPACE_BYTES, "sizes": {}}
    for S in [int(v) for v in a.sizes.split(",")]:
        dec_all = head_batch(S, max(ns), dev)
        per = kpp.image_workspace_bytes([tuple(d[0].shape[-2:]) for d in dec_all])
        row = {"workspace_bytes_per_image": per, "images_per_chunk": kpp.plan_chunks(max(ns), per, kpp.BATCH_WORKSPACE_BYTES)[0][1],
               "detect_batch_ms_per_img": {}, "detect_loop_ms_per_img": {}, "predict_img_s": {}, "predict_u8_img_s": {}, "boxes_per_img": None}
        for n in ns:
            dec = [[t[:n] for t in d] for d in dec_all]
            got = kpp.detect_batch(dec)
            loop = [kpp.detect([[t[i:i + 1] for t in d] for d in dec]) for i in range(n)]
            assert all((g is None and r is None) or (g is not None and r is not None and np.array_equal(g, r)) for g, r in zip(got, loop))
            row["boxes_per_img"] = int(np.mean([0 if g is None else len(g) for g in got]))
            row["detect_batch_ms_per_img"][n] = round(timed(lambda: kpp.detect_batch(dec), a.reps) / n, 3)
            row["detect_loop_ms_per_img"][n] = round(timed(lambda: [kpp.detect([[t[i:i + 1] for t in d] for d in dec]) for i in range(n)],
                                                           a.reps) / n, 3)
            x = (torch.rand(n, 3, S, S, generator=torch.Generator().manual_seed(n)) - 0.5).to(dev)
            row["predict_img_s"][n] = round(n / timed(lambda: inference.predict(model, x), a.reps) * 1e3, 2)
            row["predict_u8_img_s"][n] = round(n / timed(lambda: inference.predict(model, x, device_u8=True), a.reps) * 1e3, 2)
            del x
            print(S, n, row["detect_batch_ms_per_img"][n], row["detect_loop_ms_per_img"][n], row["predict_img_s"][n], row["predict_u8_img_s"][n], file=sys.stderr, flush=True)
        res["sizes"][S] = row
        del dec_all
        kpp._BatchWorkspace.cache.clear()
        torch.cuda.empty_cache()
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
