"""GPU: sampleprep.prepare_batch (csrc/sampleprep.hip) against the NumPy restatement tests/sampleprep_ref.py, BIT FOR BIT: image,
warped masks, keypoints, counts, gt_masks, gt_bboxes and the four target tensors -- on the reference fixture's inputs and on a generated
population (every combination of the six switches, 0 to 300 instances, mixed source sizes in one batch, byte / bit / host / float mask
sources), and one training step fed by either tuple.  There is no tolerance anywhere in this file."""
import hashlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sampleprep_ref as ref  # noqa: E402
from kg_instance_segmentation_amd import sampleprep  # noqa: E402
from kg_instance_segmentation_amd.bitmasks import BitMasks  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def make_sample(rs, h, w, n):
    """A decoded sample: uint8 image and n instance masks (rectangles and ellipses from 1 pixel to a third of the image)."""
    img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    masks = np.zeros((n, h, w), np.uint8)
    for j in range(n):
        big = rs.randint(4)
        a = rs.randint(1, 6) if big == 0 else rs.randint(6, max(8, h // (3 if big == 3 else 8)))
        b = rs.randint(1, 6) if big == 0 else rs.randint(6, max(8, w // (3 if big == 3 else 8)))
        y, x = rs.randint(0, h - a + 1), rs.randint(0, w - b + 1)
        if j % 3 == 0 and a > 4 and b > 4:
            yy, xx = np.mgrid[0:a, 0:b]
            masks[j, y:y + a, x:x + b] = ((yy - (a / 2 - .5)) / (a / 2)) ** 2 + ((xx - (b / 2 - .5)) / (b / 2)) ** 2 <= 1
        else:
            masks[j, y:y + a, x:x + b] = 1
    return img, masks


def make_params(rs, h, w, bits):
    """SampleParams with the six switches set from the bits of `bits`, the values drawn over the reference's ranges."""
    br, co, sw, ex, mw, mh = (bool(bits >> k & 1) for k in range(6))
    canvas, offset = (0, 0), (0, 0)
    if ex:
        r = rs.uniform(1, 2)
        canvas, offset = (int(h * r), int(w * r)), (int(rs.uniform(0, h * r - h)), int(rs.uniform(0, w * r - w)))
    return sampleprep.SampleParams(br, float(rs.uniform(-32, 32)), co, float(rs.uniform(0.5, 1.5)), sw, sampleprep.PERMS[rs.randint(6)], ex,
                                   canvas, offset, mw, mh)


def check_batch(b, images, masks, params, H, W, label):
    """Every array prepare_batch_full made against the restatement."""
    N = len(images)
    assert b.img.dtype == torch.float32 and tuple(b.img.shape) == (N, 3, H, W)
    img = b.img.cpu().numpy()
    gts = [g.cpu().numpy() for g in b.gt]
    for i in range(N):
        s = ref.prepare_sample(images[i], masks[i], params[i], H, W)
        tag = f"{label}[{i}] n={len(masks[i])} {params[i].switches()}"
        bad = int((img[i] != s["img"]).sum())
        print(f"[sampleprep {tag}] image mismatches {bad}, counts {s['counts'].tolist()}")
        assert bad == 0, tag
        assert b.warped[i].dtype == torch.uint8 and np.array_equal(b.warped[i].cpu().numpy(), s["warped"]), tag
        assert np.array_equal(b.counts[i], s["counts"]), (tag, b.counts[i], s["counts"])
        for l in range(4):
            assert np.array_equal(b.keypoints[i][l].cpu().numpy(), s["bboxes"][l]), (tag, l)
            assert gts[l][i].dtype == np.float32 and np.array_equal(gts[l][i], s["gt"][l]), (tag, l)
        assert b.instance_masks[i].is_cuda and np.array_equal(b.instance_masks[i].cpu().numpy().astype(np.float32), s["gt_masks"]), tag
        assert isinstance(b.gt_bboxes[i], np.ndarray) and b.gt_bboxes[i].dtype == np.float32 and np.array_equal(b.gt_bboxes[i], s["gt_bboxes"]), tag


def same_batches(a, b):
    assert torch.equal(a.img, b.img) and all(torch.equal(x, y) for x, y in zip(a.gt, b.gt)) and np.array_equal(a.counts, b.counts)
    for i in range(len(a.warped)):
        assert torch.equal(a.warped[i], b.warped[i]) and torch.equal(a.instance_masks[i], b.instance_masks[i])
        assert np.array_equal(a.gt_bboxes[i], b.gt_bboxes[i])
        assert all(torch.equal(x, y) for x, y in zip(a.keypoints[i], b.keypoints[i]))


def test_fixture_inputs_match_the_reference_outputs():
    fx = np.load(os.path.join(ROOT, "tests", "golden", "sampleprep.npz"))
    H, W = (int(v) for v in fx["hw"])
    images = [fx["src0.img"], fx["src1.img"]]
    masks = [fx["src0.masks"], fx["src1.masks"]]
    for t, seed in enumerate(fx["seeds"]):
        np.random.seed(int(seed))
        params = [sampleprep.draw_train_params(*im.shape[:2]) for im in images]
        b = sampleprep.prepare_batch_full(images, [torch.from_numpy(m).to(DEV) for m in masks], params, H, W, DEV)
        check_batch(b, images, masks, params, H, W, f"seed{seed}")
        tup = sampleprep.prepare_batch(images, masks, params, H, W, DEV)
        assert len(tup) == 7 and torch.equal(tup[0], b.img)
        for k in (0, 1):                                     # and the reference's own recorded outputs
            pre = f"t{t}.s{k}."
            assert np.array_equal(sha(tup[0][k].cpu().numpy()), fx[pre + "img_sha"])
            for l in range(4):
                assert np.array_equal(sha(tup[1 + l][k].cpu().numpy()), fx[pre + f"gt{l}_sha"])
                assert np.array_equal(b.keypoints[k][l].cpu().numpy(), fx[pre + f"bboxes{l}"])
            assert np.array_equal(tup[5][k].cpu().numpy(), fx[pre + "gt_masks"])
            assert np.array_equal(tup[6][k], fx[pre + "gt_bboxes"])
    val = sampleprep.prepare_batch(images, masks, [sampleprep.identity_params()] * 2, H, W, DEV)
    for k in (0, 1):
        assert np.array_equal(val[0][k].cpu().numpy(), fx[f"val.s{k}.img"])
        assert all(np.array_equal(val[1 + l][k].cpu().numpy(), fx[f"val.s{k}.gt{l}"]) for l in range(4))
        assert np.array_equal(val[6][k], fx[f"val.s{k}.gt_bboxes"])


SIZES_512 = ((256, 320), (520, 696), (1024, 1024))
COUNTS = (37, 0, 300, 1)


def population_batch(bi):
    """Batch bi of 8: batches 0..5 -> 512 x 512 from mixed source sizes, 6..7 -> 256 x 256 from 360 x 360 (one 520 x 696 among them);
    image q = 8 bi + i carries switch combination q, so the 64 images cover all 2^6."""
    rs = np.random.RandomState(100 + bi)
    H = W = 512 if bi < 6 else 256
    images, masks, params = [], [], []
    for i in range(8):
        q = 8 * bi + i
        h, w = SIZES_512[(q + bi) % 3] if bi < 6 else ((360, 360) if i != 5 else (520, 696))
        n = COUNTS[(q + q // 8) % 4]
        if n == 300 and (h, w) == (1024, 1024) and i % 2:
            n = 37                                           # (keeps the host restatement's memory in check)
        img, m = make_sample(rs, h, w, n)
        images.append(img); masks.append(m); params.append(make_params(rs, h, w, q))
    return images, masks, params, H, W


@pytest.mark.parametrize("bi", range(8))
def test_population_matches_the_restatement(bi):
    images, masks, params, H, W = population_batch(bi)
    assert len({im.shape[:2] for im in images}) > 1          # mixed source sizes inside the batch
    dm = [torch.from_numpy(m).to(DEV) for m in masks]
    b = sampleprep.prepare_batch_full(images, dm, params, H, W, DEV)
    check_batch(b, images, masks, params, H, W, f"batch{bi}")
    # the same batch from bit-packed, host and mixed (float32 tensor, device image) sources
    bits = sampleprep.prepare_batch_full(images, [BitMasks.from_dense(m, DEV) for m in masks], params, H, W, DEV)
    same_batches(b, bits)
    same_batches(b, sampleprep.prepare_batch_full(images, masks, params, H, W, DEV))
    mixed_m = [dm[i] if i % 4 == 0 else dm[i].float() if i % 4 == 1 else BitMasks.from_dense(dm[i], DEV) if i % 4 == 2 else masks[i] for i in range(8)]
    mixed_i = [torch.from_numpy(im).to(DEV) if i % 2 else im for i, im in enumerate(images)]
    same_batches(b, sampleprep.prepare_batch_full(mixed_i, mixed_m, params, H, W, DEV))


def test_population_covers_what_it_claims():
    seen, counts, sizes = set(), set(), set()
    for bi in range(8):
        images, masks, params, H, W = population_batch(bi)
        for im, m, p in zip(images, masks, params):
            seen.add(p.switches()); counts.add(len(m)); sizes.add((im.shape[:2], (H, W)))
    assert len(seen) == 64 and counts == {0, 1, 37, 300}
    assert {((256, 320), (512, 512)), ((520, 696), (512, 512)), ((1024, 1024), (512, 512)), ((360, 360), (256, 256))} <= sizes


def test_batch_without_instances_and_narrow_output():
    rs = np.random.RandomState(5)
    images = [make_sample(rs, 40, 56, 0)[0], make_sample(rs, 64, 48, 0)[0]]
    masks = [np.zeros((0, 40, 56), np.uint8), torch.zeros(0, 64, 48, dtype=torch.uint8, device=DEV)]
    params = [make_params(rs, 40, 56, 0b111111), sampleprep.identity_params()]
    b = sampleprep.prepare_batch_full(images, masks, params, 64, 64, DEV)
    check_batch(b, images, [np.zeros((0, 40, 56), np.uint8), np.zeros((0, 64, 48), np.uint8)], params, 64, 64, "empty")
    assert all(tuple(m.shape) == (0, 64, 64) for m in b.instance_masks) and all(g.shape == (0, 5) for g in b.gt_bboxes)
    assert all(float(g.abs().sum()) == 0 for g in b.gt)
    # a width that is a multiple of 8 but not of 16 takes the dword-store kernel
    img, m = make_sample(rs, 90, 70, 9)
    params = [make_params(rs, 90, 70, 0b101000), make_params(rs, 90, 70, 0b010111)]
    b = sampleprep.prepare_batch_full([img, img], [m, torch.from_numpy(m).to(DEV)], params, 96, 72, DEV)
    check_batch(b, [img, img], [m, m], params, 96, 72, "w72")
    with pytest.raises(ValueError):
        sampleprep.prepare_batch([img], [m], [params[0]], 100, 72, DEV)
    with pytest.raises(ValueError):
        sampleprep.prepare_batch([img], [m[:, :80]], [params[0]], 96, 72, DEV)


def test_train_step_on_the_device_tuple_equals_the_host_tuple(state_dict0):
    from kg_instance_segmentation_amd import KGnet
    from kg_instance_segmentation_amd.loss import DetectionLossAll
    from kg_instance_segmentation_amd.seg_loss import SEG_loss
    rs = np.random.RandomState(11)
    H = W = 256
    images, masks, params = [], [], []
    for i in range(2):
        img, m = make_sample(rs, 360, 360, 37)
        images.append(img); masks.append(m); params.append(make_params(rs, 360, 360, (0b100110, 0b011001)[i]))
    dev_tuple = sampleprep.prepare_batch(images, [BitMasks.from_dense(m, DEV) for m in masks], params, H, W, DEV)
    ss = [ref.prepare_sample(im, m, p, H, W) for im, m, p in zip(images, masks, params)]
    host_tuple = (torch.from_numpy(np.stack([s["img"] for s in ss])),) + tuple(torch.from_numpy(np.stack([s["gt"][l] for s in ss])) for l in range(4)) + \
        ([s["gt_masks"] for s in ss], [s["gt_bboxes"] for s in ss])                     # what collater returns (collater.py:20-25)
    model = KGnet.resnet50(pretrained=False)
    model.load_state_dict(state_dict0)
    model = model.to(DEV).train()
    ldec, lseg = DetectionLossAll(5), SEG_loss(H, W)
    res = []
    for img, g0, g1, g2, g3, gt_masks, gt_boxes in (dev_tuple, host_tuple):
        model.zero_grad(set_to_none=True)
        d0, d1, d2, d3, pred = model(img.to(DEV), gt_boxes)
        det = sum(ldec(p, t.to(DEV)) for p, t in zip((d0, d1, d2, d3), (g0, g1, g2, g3)))
        seg = lseg(pred, gt_masks, gt_boxes)
        (det if seg is None else det + seg).backward()
        torch.cuda.synchronize()
        res.append((float(det.detach()), None if seg is None else float(seg.detach())))
    print(f"[sampleprep train step] device tuple {res[0]}, host tuple {res[1]}")
    assert res[0][1] is not None, "no predicted patch matched a ground-truth box: the seg loss was not exercised"
    assert res[0] == res[1]
