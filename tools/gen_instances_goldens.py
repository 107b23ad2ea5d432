#!/usr/bin/env python
"""Writes tests/golden/overlay.npz: the reference's own apply_mask (test.py:29-37), looped over the masks of an image in ascending order
with alpha = 0.8 as imshow_instance_segmentation does (test.py:171-185), on seeded images, masks and colours.  Data only: per case the
image, the masks (bit-packed rows, np.packbits little-endian along x), the colours, alpha and the blended image.

    PYTHONDONTWRITEBYTECODE=1 KG_REFERENCE=/path/to/reference python tools/gen_instances_goldens.py

Needs the reference checkout (KG_REFERENCE) and the shims of tools/gen_goldens.py: a stub `cv2` (test.py imports it, apply_mask does not
use it) and the removed `np.int` alias.
"""
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = os.environ.get("KG_REFERENCE")
if not REF or not os.path.exists(os.path.join(REF, "test.py")):
    raise SystemExit("gen_instances_goldens: set KG_REFERENCE to a checkout of the reference project")
sys.path.insert(1, REF)

import numpy as np

np.int = int
cv2 = types.ModuleType("cv2")
cv2.INTER_NEAREST = 0
sys.modules["cv2"] = cv2

import test as rtest  # noqa: E402  (the reference driver)


def shapes(rng, n, H, W, smax):
    """n seeded ellipses and rectangles as float32 {0, 1} masks [n, H, W] (what post_processing returns)"""
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((n, H, W), np.float32)
    for k in range(n):
        cy, cx = rng.integers(0, H), rng.integers(0, W)
        ry, rx = rng.integers(1, smax + 1), rng.integers(1, smax + 1)
        if k % 2:
            m[k] = (np.abs(yy - cy) <= ry) & (np.abs(xx - cx) <= rx)
        else:
            m[k] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
    return m


def case(name, H, W, n, seed, smax, alpha=0.8, edge_colors=False, pile=0):
    rng = np.random.default_rng(seed)
    image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    masks = shapes(rng, n, H, W, smax)
    colors = rng.random((n, 3))
    if edge_colors:                                   # 0.0, the largest double below 1.0, and values next to them
        colors[0] = 0.0, np.nextafter(1.0, 0.0), 1.0 - 2.0 ** -20
        colors[1] = np.nextafter(1.0, 0.0), 0.0, 2.0 ** -30
        image[:4, :4] = 200                           # 200 under a colour of 0 becomes 39, not 40
        masks[0, :4, :4] = 1
    if pile:                                          # one pixel under `pile` masks
        masks[:pile, H // 2, W // 3] = 1
    out = image.copy()
    for mask, color in zip(masks, colors):
        rtest.apply_mask(image=out, mask=mask, color=color, alpha=alpha)
    assert out.dtype == np.uint8
    depth = (masks != 0).sum(0).max()
    print(f"{name}: {H} x {W}, {n} masks, deepest pile {depth}, {np.count_nonzero(np.any(out != image, 2))} pixels changed")
    return {f"{name}.image": image, f"{name}.bits": np.packbits(masks != 0, axis=-1, bitorder="little"),
            f"{name}.colors": colors, f"{name}.alpha": np.float64(alpha), f"{name}.out": out}, depth


def main():
    out = {}
    d, _ = case("small", 37, 70, 9, 11, 12)
    out.update(d)
    d, _ = case("wide", 64, 128, 70, 12, 14)
    out.update(d)
    d, _ = case("edge", 37, 70, 9, 13, 12, edge_colors=True)
    out.update(d)
    d, depth = case("pile", 24, 70, 8, 14, 8, pile=6)
    assert depth >= 5
    out.update(d)
    assert out["edge.out"][0, 0, 0] == 39 or (out["edge.bits"][1:, 0, 0] & 1).any()
    path = os.path.join(ROOT, "tests", "golden", "overlay.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
