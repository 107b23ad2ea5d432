#!/usr/bin/env python
"""Measures sampleprep.prepare_batch on the GPU (README "Training samples on the device").

    python tools/sampleprep_bench.py [--batch 8] [--size 512] [--boxes 300] [--src 520x696] [--reps 50] [--bench-json FILE] [--out FILE]

Configuration: N images of `--src` pixels, `--boxes` instances each as bit-packed device masks, train-pipeline parameters drawn with a
seeded generator (every batch of the timed window reuses the same sources and parameters).  Reported:
  (a) ms per batch of prepare_batch end to end (host clock around calls that end in the batch's stream synchronise, after warm-up), and
      its split into image / masks / boxes / targets from device events around the library calls in a run of its own;
  (b) the mask-warp kernel's achieved bytes/s over its output bytes (N * boxes * H * W), next to a device-to-device copy of the same
      number of bytes timed in the same run;
  (c) tests/sampleprep_ref.py (this repository's NumPy restatement, NOT OpenCV) on the host for one image;
  (d) with --bench-json (the JSON line `bench.py --gpus 1 --mode train` printed on the same machine): (a) over the train step.
There is no CPU fallback: without a GPU the tool fails."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

import numpy as np
import torch

from kg_instance_segmentation_amd import _lib, sampleprep
from kg_instance_segmentation_amd.bitmasks import BitMasks


def make_sample(rs, h, w, n):
    img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    masks = np.zeros((n, h, w), np.uint8)
    for j in range(n):
        a, b = rs.randint(12, max(14, h // 6)), rs.randint(12, max(14, w // 6))
        y, x = rs.randint(0, h - a + 1), rs.randint(0, w - b + 1)
        yy, xx = np.mgrid[0:a, 0:b]
        masks[j, y:y + a, x:x + b] = ((yy - (a / 2 - .5)) / (a / 2)) ** 2 + ((xx - (b / 2 - .5)) / (b / 2)) ** 2 <= 1
    return img, masks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--boxes", type=int, default=300)
    ap.add_argument("--src", default="520x696")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bench-json", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--profile-run", action="store_true", help="one warm-up batch and one more, nothing else (for tools/sampleprep_trace.sh)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sampleprep_bench: no GPU (this tool never falls back to the CPU)")
    dev = torch.device("cuda:0")
    h, w = (int(v) for v in args.src.split("x"))
    N, S, n = args.batch, args.size, args.boxes
    rs = np.random.RandomState(0)
    samples = [make_sample(rs, h, w, n) for _ in range(N)]
    images = [torch.from_numpy(s[0]).to(dev) for s in samples]
    masks = [BitMasks.from_dense(s[1], dev) for s in samples]
    params = [sampleprep.draw_train_params(h, w, rs) for _ in range(N)]

    def run():
        return sampleprep.prepare_batch(images, masks, params, S, S, dev)

    if args.profile_run:
        run()
        torch.cuda.synchronize()
        run()
        torch.cuda.synchronize()
        return
    for _ in range(args.warmup):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = run()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    times = np.array(times)
    kept = sum(int(m.shape[0]) for m in out[5])

    # split: device events around every library call, in a run of its own
    stage_of = {"kg_sp_image": "image", "kg_sp_warp_masks": "masks", "kg_sp_boxes": "boxes", "kg_gt_maps": "targets"}
    events, real_call = [], _lib.call

    def timed_call(name, *a, **k):
        if name not in stage_of:
            return real_call(name, *a, **k)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); real_call(name, *a, **k); e1.record()
        events.append((stage_of[name], e0, e1))
    _lib.call = timed_call
    split = {s: [] for s in stage_of.values()}
    try:
        for _ in range(max(10, args.reps // 5)):
            events.clear()
            run()
            torch.cuda.synchronize()
            acc = dict.fromkeys(split, 0.0)
            for s, e0, e1 in events:
                acc[s] += e0.elapsed_time(e1)
            for s in split:
                split[s].append(acc[s])
    finally:
        _lib.call = real_call
    split_ms = {s: float(np.median(v)) for s, v in split.items()}

    # (b) a device-to-device copy of the warp's output bytes, same run
    nbytes = N * n * S * S
    src_t = torch.empty(nbytes, dtype=torch.uint8, device=dev).random_(0, 2)
    dst_t = torch.empty_like(src_t)
    cp = []
    for i in range(25):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); dst_t.copy_(src_t); e1.record()
        torch.cuda.synchronize()
        if i >= 5:
            cp.append(e0.elapsed_time(e1))
    copy_ms = float(np.median(cp))

    # (c) the NumPy restatement on the host, one image
    import sampleprep_ref as ref
    t0 = time.perf_counter()
    ref.prepare_sample(samples[0][0], samples[0][1], params[0], S, S)
    ref_s = time.perf_counter() - t0

    res = {"config": {"batch": N, "size": S, "instances_per_image": n, "source": [h, w], "mask_source": "bit-packed device words", "reps": args.reps,
                      "kept_instances": kept},
           "prepare_batch_ms": {"median": float(np.median(times)), "min": float(times.min()), "p90": float(np.percentile(times, 90))},
           "split_ms_device_events": split_ms,
           "mask_warp": {"output_bytes": nbytes, "ms": split_ms["masks"], "GB_per_s_written": nbytes / split_ms["masks"] / 1e6,
                         "d2d_copy_ms": copy_ms, "d2d_copy_GB_per_s_written": nbytes / copy_ms / 1e6,
                         "fraction_of_copy_rate": copy_ms / split_ms["masks"]},
           "numpy_restatement_one_image_s": ref_s}
    if args.bench_json:
        line = [l for l in open(args.bench_json).read().splitlines() if l.startswith("{")][-1]
        b = json.loads(line)
        step_ms = 1e3 * N / float(b["value"])
        res["train_step"] = {"imgs_per_s": float(b["value"]), "step_ms_at_this_batch": step_ms,
                             "prepare_batch_over_train_step": float(np.median(times)) / step_ms}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
