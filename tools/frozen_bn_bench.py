"""Train step with frozen BatchNorm against the train-mode step, and kg_bn_bwd_frozen against a device-to-device copy.

    python tools/frozen_bn_bench.py [--steps 10] [--warmup 4] [--repeats 3] [--out profiles/frozen_bn_bench.json]

The bench configuration's train step (bench.py: 8 x 512^2, 300 boxes per image, default policy, fused Adam with prepack, the loss read
back every step, Python's cyclic collector parked) in three settings, each on its own seeded model:
  train_bn          train-mode BatchNorm (nothing frozen: the code path bench.py times)
  frozen_stats      model.freeze_bn(affine=False): running statistics, weight / bias trained (unfused: conv, bn_apply; one-pass backward)
  frozen_all_stem   model.freeze_bn() + requires_grad=False on conv1 / layer1 (conv -> BatchNorm as one launch, no backward below layer2)
The settings are timed in alternation, `--repeats` windows of `--steps` steps each, so that the spread of one setting's windows says how
large a difference between two settings has to be before it means anything.
Kernel: achieved bytes/s of kg_bn_bwd_frozen (with and without the dgamma / dbeta sums; bytes = what the algorithm has to move, computed
from the shapes) beside a device-to-device copy that moves the same number of bytes.  Needs a GPU; there is no fallback.
"""
import argparse
import gc
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def freeze_stem(m):
    m.freeze_bn()
    for n, p in m.named_parameters():
        if n.startswith(("conv1.", "layer1.")):
            p.requires_grad_(False)


SETTINGS = (("train_bn", lambda m: None), ("frozen_stats", lambda m: m.freeze_bn(affine=False)), ("frozen_all_stem", freeze_stem))


def step_bench(args, dev):
    import bench
    from kg_instance_segmentation_amd import KGnet
    from kg_instance_segmentation_amd.loss import DetectionLossAll
    from kg_instance_segmentation_amd.optim import Adam
    from kg_instance_segmentation_amd.seg_loss import SEG_loss
    x, gt, gt_masks, gt_boxes = bench.make_batch(args.batch, args.size, args.boxes, 100, dev)
    ldec, lseg = DetectionLossAll(kp_radius=5), SEG_loss(height=args.size, width=args.size)
    runs = {}
    for name, setup in SETTINGS:
        torch.manual_seed(1234)
        model = KGnet.resnet50(pretrained=False).to(dev).train()
        setup(model)
        opt = Adam(filter(lambda p: p.requires_grad, model.parameters()), lr=1e-4, prepack=model)

        def step(model=model, opt=opt):
            opt.zero_grad()
            p0, p1, p2, p3, pred = model(x, gt_boxes)
            l1 = ldec(p0, gt[0]) + ldec(p1, gt[1]) + ldec(p2, gt[2]) + ldec(p3, gt[3])
            l2 = lseg(pred, gt_masks, gt_boxes)
            loss = l1 if l2 is None else l1 + l2
            loss.backward()
            opt.step()
            return loss.item()          # train.py:156 reads the loss back every step
        for _ in range(args.warmup):
            step()
        runs[name] = {"step": step, "model": model, "windows_ms": [], "loss": None}
    for _ in range(args.repeats):
        for name, _ in SETTINGS:
            r = runs[name]
            gc.collect(); gc.freeze(); gc.disable()
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    r["loss"] = r["step"]()
                torch.cuda.synchronize()
                r["windows_ms"].append((time.perf_counter() - t0) / args.steps * 1e3)
            finally:
                gc.enable(); gc.unfreeze()
    out = {}
    for name, _ in SETTINGS:
        r = runs[name]
        w = r["windows_ms"]
        out[name] = {"step_ms_windows": [round(v, 3) for v in w], "step_ms_best": round(min(w), 3), "step_ms_median": round(sorted(w)[len(w) // 2], 3),
                     "spread_ms": round(max(w) - min(w), 3), "imgs_per_s_median": round(args.batch / (sorted(w)[len(w) // 2] * 1e-3), 2),
                     "last_loss": r["loss"], "grad_overflowed": bool(r["model"].grad_overflowed()),
                     "trainable_tensors": sum(1 for p in r["model"].parameters() if p.requires_grad)}
    return out


def kernel_bench(dev, M=8 * 128 * 128, C=256, reps=20):
    from kg_instance_segmentation_amd import ops
    g = torch.Generator().manual_seed(0)
    res = {"rows": M, "channels": C, "format": "IEEE-half rows: x 2 planes, dy 1 plane, dx 1 plane (the default policy's backbone)"}
    x, dy, dx = ops.alloc_pt(M, C, 2, dev, dtype=ops.F16), ops.alloc_pt(M, C, 1, dev, dtype=ops.F16), ops.alloc_pt(M, C, 1, dev, dtype=ops.F16)
    ops.f32_to_planes(torch.randn(M, C, generator=g).to(dev), x, C)
    ops.f32_to_planes(torch.randn(M, C, generator=g).to(dev), dy, C)
    scale, rm, rv = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev), torch.rand(C, device=dev) + 0.5
    dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)

    def timed(fn):
        for _ in range(3):
            fn()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / reps * 1e-3
    for name, fn, nbytes, launches in (("with_sums", lambda: ops.bn_bwd_frozen(x, dy, C, scale, rm, rv, dg, db, dx), M * C * 2 * (2 + 1 + 1),
                                        "two launches (stream + per-channel finalize)"),
                                       ("dx_only", lambda: ops.bn_bwd_frozen(None, dy, C, scale, None, None, None, None, dx), M * C * 2 * (1 + 1),
                                        "one launch")):
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        tk, tc = timed(fn), timed(lambda: dst.copy_(src))
        res[name] = {"bytes_moved": nbytes, "kernel_us": round(tk * 1e6, 2), "kernel_GBps": round(nbytes / tk / 1e9, 1),
                     "d2d_copy_us": round(tc * 1e6, 2), "d2d_copy_GBps": round(nbytes / tc / 1e9, 1), "kernel_over_copy": round(tc / tk, 3),
                     "note": launches + "; the copy reads and writes bytes_moved / 2 each"}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--boxes", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frozen_bn_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frozen_bn_bench.py measures on the GPU; none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = {"config": {k: getattr(args, k) for k in ("steps", "warmup", "repeats", "batch", "size", "boxes")}, "precision": "fp32 (default policy)",
           "device": torch.cuda.get_device_name(dev), "kernel": kernel_bench(dev), "step": step_bench(args, dev)}
    base = out["step"]["train_bn"]
    for name in ("frozen_stats", "frozen_all_stem"):
        out["step"][name]["median_ms_saved_vs_train_bn"] = round(base["step_ms_median"] - out["step"][name]["step_ms_median"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
