"""GPU: batched inference.  detect_batch (one launch per stage and scale for all images of a batch) against the C oracle and against
detect() image by image, bit for bit; the per-image fall-back paths of the Hough vote and of the grouping inside a batch; chunking
under a workspace budget; predict() end to end against the reference driver's per-image path assembled by hand."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from kg_instance_segmentation_amd import KGnet, inference, postprocessing as kpp  # noqa: E402
from oracle import postproc as op, synth, weightgen  # noqa: E402

DEV = "cuda"


def four_scales(S, n, seed):
    """synth.head_maps at the four scales of an S x S image: [[kp, short, mid] x 4] numpy [1,C,h,w]."""
    out = []
    for sc in (1, 2, 4, 8):
        h = S // sc
        kp, short, mid, _ = synth.head_maps(h, h, max(1, n // sc), seed * 10 + sc, smin=max(3, 14 // sc), smax=max(6, 40 // sc))
        out.append([kp, short, mid])
    return out


def zeros_like(dec):
    return [[np.zeros_like(a) for a in d] for d in dec]


def stack(decs):
    """per-image four-scale maps -> the batch on the GPU ([[kp, short, mid] x 4], leading dimension N)"""
    return [[torch.from_numpy(np.concatenate([dd[l][k] for dd in decs], 0)).to(DEV) for k in range(3)] for l in range(4)]


def same(got, ref):
    if ref is None:
        return got is None
    return got is not None and got.shape == ref.shape and np.array_equal(got, ref)


@pytest.fixture(scope="module")
def batch256():
    decs = [four_scales(256, 24 + 12 * i, 100 + i) for i in range(5)]
    decs[2] = zeros_like(decs[2])                                       # an image without any keypoint: its slot is None
    return decs, [op.detect(d, 0.5) for d in decs]


@pytest.mark.parametrize("S", [256, 512])
def test_detect_batch_vs_oracle_and_detect(batch256, S):
    if S == 256:
        decs, refs = batch256
    else:
        decs = [four_scales(512, 60, 200), zeros_like(four_scales(512, 1, 201)), four_scales(512, 120, 202)]
        refs = [op.detect(d, 0.5) for d in decs]
    dec = stack(decs)
    got = kpp.detect_batch(dec, 0.5)
    assert len(got) == len(decs)
    for i, (g, r) in enumerate(zip(got, refs)):
        one = kpp.detect([[t[i:i + 1] for t in d] for d in dec], 0.5)
        print(f"S={S} image {i}: {0 if r is None else len(r)} boxes")
        assert same(g, r), i
        assert same(one, r), i
    assert refs[2 if S == 256 else 1] is None
    assert sum(r is not None for r in refs) == len(refs) - 1


def test_detect_batch_chunked_equals_whole(batch256):
    decs, refs = batch256
    dec = stack(decs)
    per = kpp.image_workspace_bytes([tuple(d[0].shape[-2:]) for d in dec])
    assert len(kpp.plan_chunks(len(decs), per, 2 * per)) >= 3
    got = kpp.detect_batch(dec, 0.5, max_workspace_bytes=2 * per)
    assert all(same(g, r) for g, r in zip(got, refs))


def _tile_case_maps(case, seed):
    """one 160 x 192 scale as test_gpu_postproc's tile-formulation edge cases build it ("plain": the common path)"""
    rng = np.random.default_rng(seed)
    H, W = 160, 192
    kp = np.clip(rng.random((1, 5, H, W)), 0.05, 1).astype(np.float32)
    short = rng.normal(0, 0.6, (1, 10, H, W)).astype(np.float32)
    mid = rng.normal(0, 3, (1, 40, H, W)).astype(np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    if case == "tile_overflow":
        short[0, 0::2, 56:104, 76:124] = (100.3 - xx[56:104, 76:124]).astype(np.float32) + rng.uniform(0, 3, (48, 48)).astype(np.float32)
        short[0, 1::2, 56:104, 76:124] = (80.3 - yy[56:104, 76:124]).astype(np.float32) + rng.uniform(0, 3, (48, 48)).astype(np.float32)
    elif case == "far_list_overflow":
        short = rng.normal(0, 60, (1, 10, H, W)).astype(np.float32)
    return kp, short, mid


def test_mixed_fallback_batch_per_image():
    """Two images that make the tile formulation give up (tile overflow, far-list overflow) between two that keep it: every image's
    skeletons equal the oracle's, and the fall-back images' heat maps (N = 1 debug path) too -- the fall-back flags are per image."""
    cases = ["plain", "tile_overflow", "far_list_overflow", "plain"]
    maps = [_tile_case_maps(c, 31 + i) for i, c in enumerate(cases)]
    kp, short, mid = [torch.from_numpy(np.concatenate([m[k] for m in maps], 0)).to(DEV) for k in range(3)]
    skel, nsk = kpp.skeletons_batch_device(kp, short, mid)
    skel, nsk = skel.cpu().numpy(), nsk.cpu().numpy()
    for i, (c, m) in enumerate(zip(cases, maps)):
        ref = op.get_skeletons(*m)
        print(f"{c}: {len(ref)} skeletons")
        assert nsk[i] == len(ref) and np.array_equal(skel[i, :nsk[i]], ref), c
        if c != "plain":
            _, _, dbg = kpp.skeletons_device(*[torch.from_numpy(a).to(DEV) for a in m], debug=True)
            assert np.array_equal(dbg["heat"].cpu().numpy(), op.hough(m[0], m[1])), c


def test_general_grouping_path_in_a_batch():
    """An image with > 8192 peaks (the grouping kernel's general path) between two ordinary ones."""
    H, W = 384, 512
    rng = np.random.default_rng(13)
    heavy = ((rng.random((1, 5, H, W)) ** 2).astype(np.float32), (rng.normal(size=(1, 10, H, W)) * 2).astype(np.float32),
             (rng.normal(size=(1, 40, H, W)) * 6).astype(np.float32))
    plain = [synth.head_maps(H, W, 40, s)[:3] for s in (5, 6)]
    maps = [plain[0], heavy, plain[1]]
    kp, short, mid = [torch.from_numpy(np.concatenate([m[k] for m in maps], 0)).to(DEV) for k in range(3)]
    skel, nsk = kpp.skeletons_batch_device(kp, short, mid)
    skel, nsk = skel.cpu().numpy(), nsk.cpu().numpy()
    assert len(op.peaks(op.gauss(op.hough(heavy[0], heavy[1])))[0]) > 8192
    for i, m in enumerate(maps):
        ref = op.get_skeletons(*m)
        assert nsk[i] == len(ref) and np.array_equal(skel[i, :nsk[i]], ref), i


@pytest.fixture(scope="module")
def cal_model():
    m = KGnet.resnet50(pretrained=False)
    m.load_state_dict(weightgen.gen_state_dict(0, variant="cal"))
    return m.to(DEV).eval()


def _by_hand(model, dec, feats, S, sizes):
    """test.py:104-157 image by image on the batched forward_dec outputs: detect on the slices, ONE forward_seg with the boxes of
    every image, paste_masks (per output size), split by image"""
    N = dec[0][0].shape[0]
    dets = [kpp.detect([[t[i:i + 1] for t in d] for d in dec], 0.5) for i in range(N)]
    if all(d is None for d in dets):
        return [None] * N, dets
    with torch.no_grad():
        pred = model.forward_seg(feats, [d if d is not None else np.zeros((0, 5)) for d in dets])
    img = pred.kg_meta["img"]
    out = [None] * N
    for i in range(N):
        if dets[i] is None:
            continue
        h, w = sizes[i]
        masks, dd = kpp.paste_masks(pred, S, S, w, h, 0.5)
        rows = np.nonzero(img == i)[0]
        out[i] = [masks[rows], dd[rows]]
    return out, dets


def _equal(got, ref):
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        assert (g is None) == (r is None)
        if r is not None:
            assert g[0].shape == r[0].shape and np.array_equal(g[0], r[0])
            assert g[1].shape == r[1].shape and np.array_equal(g[1], r[1])


def test_predict_end_to_end(cal_model):
    S, N = 256, 4
    x = (torch.rand(N, 3, S, S, generator=torch.Generator().manual_seed(7)) - 0.5).to(DEV)
    with torch.no_grad():
        out = cal_model.forward_dec(x)
    dec, feats = list(out[:4]), out[4]
    assert not cal_model.training
    for sizes in ([(S, S)] * N, [(256, 256), (300, 200), (256, 256), (520, 696)]):
        ref, dets = _by_hand(cal_model, dec, feats, S, sizes)
        print("detections per image", [0 if d is None else len(d) for d in dets])
        assert any(d is not None for d in dets)
        _equal(inference.predict(cal_model, x, image_sizes=None if sizes[1] == (S, S) else sizes), ref)
        assert not cal_model.training
        # image 2 without any detection (its head maps zeroed): its slot is None, the others are unchanged
        decz = [[t.clone() for t in d] for d in dec]
        for d in decz:
            for t in d:
                t[2].zero_()
        refz, detz = _by_hand(cal_model, decz, feats, S, sizes)
        assert detz[2] is None
        gotz = inference.predict_from_heads(cal_model, decz, feats, S, S, image_sizes=sizes)
        _equal(gotz, refz)
        assert gotz[2] is None
        for i in (0, 1, 3):
            assert (gotz[i] is None) == (ref[i] is None)
            if ref[i] is not None:
                assert np.array_equal(gotz[i][1], ref[i][1])
