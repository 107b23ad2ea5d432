"""CPU: the sample preparation's host side (kg_instance_segmentation_amd.sampleprep) and its NumPy restatement (tests/sampleprep_ref.py)
against the reference's own outputs (tests/golden/sampleprep.npz, written by tools/gen_sampleprep_goldens.py from transforms.Compose,
BaseDataset.__getitem__ and collater) and against hand-computed vectors.  No kernel runs here."""
import hashlib
import os
import re

import numpy as np
import pytest

import sampleprep_ref as ref
from kg_instance_segmentation_amd import sampleprep
from oracle import preproc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("kg_sp_image", "kg_sp_warp_masks", "kg_sp_boxes")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(ROOT, "tests", "golden", "sampleprep.npz"))


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def observed_params(fx, tag, k):
    """SampleParams as the reference's run shows them: the draws in call order and the image shape after every transform."""
    if tag == "val":
        assert len(fx[f"{tag}.s{k}.draw_kind"]) == 0
        return sampleprep.identity_params()
    kind, val = list(fx[f"{tag}.s{k}.draw_kind"]), list(fx[f"{tag}.s{k}.draw_val"])
    shapes = fx[f"{tag}.s{k}.shapes"]
    h, w = (int(v) for v in shapes[0])

    def take(want):
        assert kind.pop(0) == want
        return val.pop(0)
    brightness = bool(take(0)); delta = take(1) if brightness else 0.0
    take(0)
    contrast = bool(take(0)); alpha = take(1) if contrast else 1.0
    swap = bool(take(0)); perm = sampleprep.PERMS[int(take(0))] if swap else (0, 1, 2)
    expand = take(0) == 0
    canvas, offset = (0, 0), (0, 0)
    if expand:
        take(1); y1 = take(1); x1 = take(1)
        canvas, offset = tuple(int(v) for v in shapes[2]), (int(y1), int(x1))       # the canvas as the reference allocated it
    else:
        assert tuple(shapes[2]) == (h, w)
    mirror_w = bool(take(0)); mirror_h = bool(take(0))
    assert not kind
    return sampleprep.SampleParams(brightness, delta, contrast, alpha, swap, perm, expand, canvas, offset, mirror_w, mirror_h)


def all_samples(fx):
    return [(f"t{t}", k) for t in range(len(fx["seeds"])) for k in (0, 1)] + [("val", 0), ("val", 1)]


def test_draw_train_params_equals_the_reference_draws(fx):
    for t, seed in enumerate(fx["seeds"]):
        np.random.seed(int(seed))
        for k in (0, 1):                                     # the reference prepared sample 0, then sample 1, under one seed
            h, w = fx[f"src{k}.img"].shape[:2]
            got = sampleprep.draw_train_params(h, w)
            assert got == observed_params(fx, f"t{t}", k), (seed, k)
    # a RandomState draws the same as the module-level generator
    np.random.seed(3)
    a = sampleprep.draw_train_params(40, 56)
    assert sampleprep.draw_train_params(40, 56, np.random.RandomState(3)) == a


def test_ref_reproduces_the_reference_outputs(fx):
    H, W = (int(v) for v in fx["hw"])
    full = 0
    for tag, k in all_samples(fx):
        p = observed_params(fx, tag, k)
        s = ref.prepare_sample(fx[f"src{k}.img"], fx[f"src{k}.masks"], p, H, W)
        pre = f"{tag}.s{k}."
        assert s["img"].dtype == np.float32 and np.array_equal(sha(s["img"]), fx[pre + "img_sha"]), pre
        for l in range(4):
            assert np.array_equal(s["bboxes"][l], fx[pre + f"bboxes{l}"]), (pre, l)
            assert np.array_equal(sha(s["gt"][l]), fx[pre + f"gt{l}_sha"]), (pre, l)
        assert s["gt_masks"].dtype == np.float32 and np.array_equal(s["gt_masks"], fx[pre + "gt_masks"].astype(np.float32)), pre
        assert s["gt_bboxes"].dtype == np.float32 and np.array_equal(s["gt_bboxes"], fx[pre + "gt_bboxes"]), pre
        if pre + "img" in fx.files:                          # the arrays stored in full
            full += 1
            assert np.array_equal(s["img"], fx[pre + "img"])
            assert all(np.array_equal(s["gt"][l], fx[pre + f"gt{l}"]) for l in range(4))
        # the composed index map is the reference's canvas / slicing / resize
        assert np.array_equal(s["warped"], ref.warp_masks_literal(fx[f"src{k}.masks"], p, H, W))
    assert full >= 4


def test_fixture_covers_every_route(fx):
    """The reference's outputs alone show every switch both ways and both box filters keeping and dropping."""
    ps = [observed_params(fx, f"t{t}", k) for t in range(len(fx["seeds"])) for k in (0, 1)]
    sw = np.array([p.switches() for p in ps])
    assert (sw.sum(0) >= 2).all() and ((~sw).sum(0) >= 2).all(), sw.sum(0)
    assert any(p.expand and (p.mirror_w or p.mirror_h) for p in ps)
    assert any(p.expand and p.canvas != fx[f"src{k}.img"].shape[:2] for p, k in zip(ps, [0, 1] * len(fx["seeds"])))
    kept1_dropped8 = dropped_gt = m_lt_n = 0
    for tag, k in all_samples(fx):
        pre = f"{tag}.s{k}."
        n, m = len(fx[f"src{k}.masks"]), len(fx[pre + "gt_bboxes"])
        kept1_dropped8 += len(fx[pre + "bboxes0"]) > len(fx[pre + "bboxes3"])
        m_lt_n += m < n
        # an instance whose warped mask is non-empty but fails |y2 - y1| > 2 and |x2 - x1| > 2 (dataset_base.py:53)
        p = observed_params(fx, tag, k)
        warped = ref.warp_masks_literal(fx[f"src{k}.masks"], p, *(int(v) for v in fx["hw"]))
        dropped_gt += int(warped.any((1, 2)).sum()) > m
    assert kept1_dropped8 >= 1 and dropped_gt >= 1 and m_lt_n >= 1, (kept1_dropped8, dropped_gt, m_lt_n)


def test_composed_index_map_by_hand():
    """5 x 7 mask, Expand to 8 x 11 at (2, 3), both mirrors, nearest resize to 6 x 6.
    rows: scale 8/6 -> canvas rows floor(d * 4/3) = 0 1 2 4 5 6, mirrored 7 - v = 7 6 5 3 2 1, minus 2 -> 5 4 3 1 0 -1: 5 is outside (h 5)
    cols: scale 11/6 -> floor(d * 11/6) = 0 1 3 5 7 9, mirrored 10 - v = 10 9 7 5 3 1, minus 3 -> 7 6 4 2 0 -2: 7 is outside (w 7)"""
    p = sampleprep.SampleParams(expand=True, canvas=(8, 11), offset=(2, 3), mirror_w=True, mirror_h=True)
    assert list(ref.source_index(5, 8, 2, True, 6)) == [-1, 4, 3, 1, 0, -1]
    assert list(ref.source_index(7, 11, 3, True, 6)) == [-1, 6, 4, 2, 0, -1]
    m = (np.arange(35).reshape(1, 5, 7) % 3 == 0).astype(np.uint8)
    want = np.zeros((1, 6, 6), np.uint8)
    for y, sy in enumerate([-1, 4, 3, 1, 0, -1]):
        for x, sx in enumerate([-1, 6, 4, 2, 0, -1]):
            if sy >= 0 and sx >= 0:
                want[0, y, x] = m[0, sy, sx]
    assert want.sum() > 0
    assert np.array_equal(ref.warp_masks(m, p, 6, 6), want)
    assert np.array_equal(ref.warp_masks_literal(m, p, 6, 6), want)
    # the rule's clamp: an upscale 3 -> 7 reads floor(d * 3/7) = 0 0 0 1 1 2 2
    assert list(ref.nearest_index(3, 7)) == [0, 0, 0, 1, 1, 2, 2]


def test_boxes_by_hand():
    m = np.zeros((4, 32, 32), np.uint8)
    m[0, 3:20, 5:30] = 1            # y 3..19, x 5..29: kept at scale 1 (16 > 11, 24 > 11); scale 2: y 2..9 -> 7, dropped
    m[1, 0:32, 0:32] = 1            # scale 2: 0..15 -> 15 > 11 kept; scale 4: 0..7 dropped
    m[2, 10:13, 10:20] = 1          # y2 - y1 = 2: dropped by the gt filter too
    bb, keep = ref.masks_to_bboxes(m, 1)
    assert list(keep) == [0, 1] and bb.dtype == np.float32
    assert bb[0].tolist() == [[5, 3], [29, 3], [5, 19], [29, 19], [17, 11]]
    bb2, keep2 = ref.masks_to_bboxes(m, 2)
    assert list(keep2) == [1] and bb2[0].tolist() == [[0, 0], [15, 0], [0, 15], [15, 15], [7.5, 7.5]]
    assert len(ref.masks_to_bboxes(m, 4)[0]) == 0 and ref.masks_to_bboxes(m, 8)[0].shape == (0, 5, 2)
    gm, gb, idx = ref.load_gt_masks_bboxes(m)
    assert list(idx) == [0, 1] and gb.tolist() == [[3, 5, 19, 29, 1], [0, 0, 31, 31, 1]] and gm.shape == (2, 32, 32)


def test_ref_ground_truth_equals_the_oracle(fx):
    H, W = (int(v) for v in fx["hw"])
    for pre in ("t0.s0.", "t3.s1.", "val.s1."):
        for l, sc in enumerate((1, 2, 4, 8)):
            bb = fx[pre + f"bboxes{l}"]
            assert np.array_equal(ref.ground_truth(bb, H // sc, W // sc), preproc.ground_truth(bb, H // sc, W // sc))
    rng = np.random.RandomState(0)                           # crowded, half-integer centres, keypoints on the border
    x1 = rng.randint(0, 40, 60); y1 = rng.randint(0, 40, 60); x2 = x1 + rng.randint(1, 24, 60); y2 = y1 + rng.randint(1, 24, 60)
    bb = np.stack([np.stack([x1, y1], 1), np.stack([x2, y1], 1), np.stack([x1, y2], 1), np.stack([x2, y2], 1),
                   np.stack([(x1 + x2) / 2, (y1 + y2) / 2], 1)], 1).astype(np.float32)
    assert np.array_equal(ref.ground_truth(bb, 64, 64), preproc.ground_truth(bb, 64, 64))


def test_entry_points_declared_in_header_and_bindings():
    from kg_instance_segmentation_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "kgnet_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib._SIGS, name
    assert build.SOURCES["sampleprep.hip"] == ["-ffp-contract=off"] and "sampleprep.hip" not in build.ROWS_SOURCES
    # the record table mirrors struct SpImage
    src = open(os.path.join(ROOT, "kg_instance_segmentation_amd", "csrc", "sampleprep.hip")).read()
    assert "sizeof(SpImage) == %d" % sampleprep._REC.itemsize in src


def test_parameter_validation():
    P = sampleprep.SampleParams
    assert sampleprep.identity_params().resolved(40, 56) == (0.0, 1.0, (0, 1, 2), 40, 56, 0, 0)
    assert P(expand=True, canvas=(50, 60), offset=(10, 4)).resolved(40, 56) == (0.0, 1.0, (0, 1, 2), 50, 60, 10, 4)
    # switched-off values are ignored, as the reference never draws them
    assert P(delta=9.0, alpha=0.7, perm=(2, 1, 0), canvas=(1, 1), offset=(5, 5)).resolved(40, 56) == (0.0, 1.0, (0, 1, 2), 40, 56, 0, 0)
    for bad in (P(expand=True, canvas=(50, 60), offset=(11, 4)), P(expand=True, canvas=(50, 60), offset=(0, 5)),
                P(expand=True, canvas=(39, 60), offset=(0, 0)), P(expand=True, canvas=(50, 60), offset=(-1, 0)),
                P(swap=True, perm=(0, 0, 2)), P(brightness=True, delta=float("nan"))):
        with pytest.raises(ValueError):
            bad.resolved(40, 56)


def test_prepare_batch_refuses_without_a_gpu_device():
    from kg_instance_segmentation_amd import _lib
    img = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(_lib.KGLibraryError):
        sampleprep.prepare_batch([img], [np.zeros((1, 8, 8), np.uint8)], [sampleprep.identity_params()], 8, 8, device="cpu")
