"""Box populations for the per-box segmentation branch and the kernel route each of them is planned to take (TEST INFRASTRUCTURE, not product).

SegBranch (kg_instance_segmentation_amd/seg.py) chooses the kernel of every ragged convolution from the DATA: how well the boxes of a launch fill
their tiles, how many workgroups the launch has, how many pyramid levels accept a box.  This module
  * defines named, seeded box populations on a c0 map of 256 x 512 (levels 256 x 512 ... 16 x 32) that between them reach every route,
  * walks the launches of SegBranch.run_forward / _run_backward over seg.crop_rects, asks routes.py (the planner SegBranch.rconv / conv_bwd /
    ops.conv_halo ask) for the route of each and restates launch_halo's channel split (csrc/conv_halo.hip) as host arithmetic (`plan_routes`)
    -- tests/test_seg_routes_cpu.py asserts the coverage table from it and tests/test_gpu_seg_routes.py asserts that the launches observed on the GPU are exactly the planned ones,
  * builds the seeded feature maps, the float64 / float32 oracle runs and the per-region metrics of the gradient tests.
Route tags are "<entry point>[/<what distinguishes the route>]"; the same tags are produced from the arguments of the observed calls
(`tag_of_call`)."""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from kg_instance_segmentation_amd import routes

from . import net as onet

H0, W0 = 256, 512
SIZES = [(H0 >> l, W0 >> l) for l in range(5)]
FEAT_CH = [64, 64, 256, 512, 1024]                                        # c0..c4 channels (KGnet.py:125-227)
SKIP = [(64, 64, 128), (256, 64, 128), (512, 256, 512), (1024, 512, 1024)]     # skip_combine[l]: (in, out, cat)
FEAT_RMS = [0.045, 0.11, 0.16, 0.16, 0.28]                                # per-level rms of the calibrated fixture (tests/golden/net_cal.*.npz, a/b.eval.feat*)
# planes of (seg branch forward, seg branch backward) per policy (engine.PRECISIONS, columns 4 and 5)
POLICY_PLANES = {"fp32": (2, 1), "fp32b2": (2, 2), "half": (1, 1), "bf16": (1, 1)}
HALO_SPLIT_WGS = 128                                                      # launch_halo: chunk split of launches with at most this many workgroups


def _b(rows):
    a = np.asarray(rows, np.float32).reshape(-1, 4)
    return np.concatenate([a, np.linspace(1.0, 0.5, len(a), dtype=np.float32)[:, None]], 1).astype(np.float32)


def _grid_boxes(rng, n, lo, hi, h0=H0, w0=W0):
    """n boxes with sides uniform in [lo, hi), top-left corners uniform inside the image"""
    hh, ww = rng.uniform(lo, hi, n), rng.uniform(lo, hi, n)
    y1, x1 = rng.uniform(0, h0 - hh), rng.uniform(0, w0 - ww)
    return np.stack([y1, x1, y1 + hh, x1 + ww], 1)


def populations():
    """{name: list (per image) of [n, 5] float32 arrays (y1, x1, y2, x2, score) or None} -- all seeded, all inputs the reference accepts."""
    pops = {}
    # halo route at every level; the deep levels have few workgroups (channel split), level 2 has more than 128 (no split)
    pops["big"] = [_b([[0, 0, 256, 512], [8, 16, 250, 500], [20, 40, 200, 300], [100, 200, 255, 511]])]
    # gather route everywhere, top level < 4, most boxes end at level 0 / 1 / 2
    rng = np.random.default_rng(21)
    t = _grid_boxes(rng, 40, 2.6, 9.0)
    pops["tiny"] = [_b(t[:22]), _b(t[22:])]
    # every depth 0..5 in one launch, 2 x 2 crops inside a halo launch, clipping at all four image edges
    sides = [3, 6, 12, 24, 48, 96, 192]
    lad = [[10 + 3 * i, 14 + 60 * i, 10 + 3 * i + s, 14 + 60 * i + s] for i, s in enumerate(sides)]
    lad += [[120.0, 30.0, 121.4, 230.0],          # 1.4 x 200 px sliver: rejected at level 0
            [0.0, 0.0, 2.5, 2.5],                 # 2.5 px box at the origin: a 2 x 2 crop
            [236.0, 470.0, 300.0, 560.0],         # reaches past the bottom-right corner
            [-20.0, -30.0, 30.0, 40.0],           # starts at negative coordinates
            [200.0, 20.0, 203.0, 23.0],           # a second 3 x 3 crop
            [32.0, 300.0, 52.0, 320.0]]           # 20 px: 2 x 2 at level 3, rejected at level 4 (depth 4)
    pops["ladder"] = [_b(lad)]
    # unsplit ragged halo launches (> 128 workgroups), an image without boxes, many boxes per reduction bin
    rng = np.random.default_rng(22)
    c = _grid_boxes(rng, 160, 24.0, 72.0, 160, 320)
    c[:, [0, 2]] += 40; c[:, [1, 3]] += 90        # crowded into the middle of the image: every bin there holds dozens of boxes
    pops["crowd"] = [_b(c), None, _b([[30, 40, 90, 140], [100, 300, 180, 420], [5.5, 6.5, 20.5, 30.5], [200, 100, 250, 160]])]
    # pairwise disjoint (>= 16 px gaps at c0, so the crop rectangles are disjoint at every level), two pairs of identical crop size
    pops["disjoint"] = [_b([[16, 32, 26, 44],           # small A (10 x 12)
                            [32, 64, 128, 224],         # large A (96 x 160)
                            [160, 32, 200, 100],
                            [150, 250, 240, 330],
                            [20, 300, 50, 420],
                            [80, 352, 90, 364]]),       # small B = small A + (64, 320)
                        _b([[32, 320, 128, 480],        # large B = large A + (0, 256)
                            [150, 20, 170, 60],
                            [200, 200, 206, 207],
                            [16, 16, 120, 100],
                            [160, 400, 230, 500]])]
    # the accept / reject edge of crop_rects: coordinates on .5 after scaling (rint half-to-even), heights exactly 2 / just under 2
    pops["halfeven"] = [_b([[10.5, 20.5, 12.5, 60.5],       # 10.5 -> 10, 12.5 -> 12: height exactly 2 at level 0
                            [11.5, 70.5, 12.5, 110.5],      # 11.5 -> 12, 12.5 -> 12: rejected
                            [10.5, 120.5, 11.5, 160.5],     # 10.5 -> 10, 11.5 -> 12: 1 px high, accepted by the rounding
                            [30.0, 20.0, 32.0, 60.0],       # exactly 2
                            [30.0, 70.0, 31.49, 110.0],     # just under 2 after rounding: rejected
                            [40.0, 21.0, 50.0, 47.0],       # x on .5 at level 1 (10.5 -> 10, 23.5 -> 24)
                            [8.0, 200.0, 72.0, 296.0],      # y on .5 at level 4 (0.5 -> 0, 4.5 -> 4); x1 on 12.5 -> 12 at level 4
                            [24.0, 328.0, 56.0, 392.0],     # level 4: 1.5 -> 2, 3.5 -> 4: height exactly 2 there
                            [24.0, 408.0, 55.0, 472.0],     # level 4: 1.5 -> 2, 3.4375 -> 3: rejected there, depth 4
                            [100.0, 36.0, 108.0, 44.0],     # level 2: 25 .. 27, 9 .. 11: exactly 2 x 2; level 3: 12.5 -> 12, 13.5 -> 14: 2 x 2 again
                            [102.0, 70.0, 110.0, 78.0],     # level 2: 25.5 -> 26, 27.5 -> 28; 17.5 -> 18, 19.5 -> 20
                            [130.0, 100.0, 250.0, 400.0]])]
    return pops


NAMES = ("big", "tiny", "ladder", "crowd", "disjoint", "halfeven")


def seed_of(name):
    """seed of the feature maps of a population"""
    return 100 + NAMES.index(name)


def as_list(boxes):
    """the population with None replaced by an empty [0, 5] array (what the oracle iterates over)"""
    return [np.zeros((0, 5), np.float32) if b is None else np.asarray(b, np.float32) for b in boxes]


def features(boxes, seed, scale=1.0):
    """Seeded fp32 NCHW feature maps c0..c4 for the images of a population: ReLU of a normal draw, rms = FEAT_RMS * scale; non-zero
    values are kept >= 1e-4 so that "is positive" (the ReLU state the gradients are masked with) survives every 16-bit storage format."""
    n = len(boxes)
    g = torch.Generator().manual_seed(seed)
    out = []
    for l, (c, (h, w)) in enumerate(zip(FEAT_CH, SIZES)):
        f = F.relu(torch.randn(n, c, h, w, generator=g)) * (FEAT_RMS[l] * scale / math.sqrt(0.5))
        out.append(torch.where(f > 0, f.clamp_min(1e-4), f).contiguous())
    return out


# ---- the plan: what SegBranch.make_plan / run_forward / _run_backward will launch ----------------------------------------------------

def halo_ksplit(tiles, cout, cin_pad, vp):
    """launch_halo (csrc/conv_halo.hip): number of channel-chunk parts Z of a ragged 3x3 kg_conv2d_halo launch (1 = not split)"""
    wgs = tiles * ((cout + 63) // 64)
    limit = int(os.environ["KG_HALO_SPLIT"]) if os.environ.get("KG_HALO_SPLIT") else HALO_SPLIT_WGS      # (the library's own switch; 0 = never)
    if limit <= 0 or wgs > limit:
        return 1
    nch = cin_pad * vp // 64
    Z = min(-(-256 // wgs), nch // 2, 8)
    while Z > 1 and (Z - 1) * (-(-nch // Z)) >= nch:
        Z -= 1
    return max(Z, 1)


class Plan:
    pass


def plan(boxes, crop_rects=None):
    """Host restatement of SegBranch.make_plan: boxes sorted by depth (stable, descending), per-level crop sizes, rows and tile counts."""
    if crop_rects is None:
        from kg_instance_segmentation_amd.seg import crop_rects
    allb, img, idx = [], [], []
    for i, bb in enumerate(as_list(boxes)):
        allb.append(bb.reshape(-1, 5)); img += [i] * len(bb); idx += list(range(len(bb)))
    allb = np.concatenate(allb, 0) if allb else np.zeros((0, 5), np.float32)
    p = Plan()
    p.nimg = len(boxes)
    p.all_boxes, p.all_img = allb, np.asarray(img, np.int32)
    rects, depth = crop_rects(allb[:, :4], H0, W0, SIZES)
    p.all_depth, p.all_rects = depth, rects
    keep = depth > 0
    order = np.argsort(-depth[keep], kind="stable")
    sel = np.nonzero(keep)[0][order]
    p.sel = sel
    p.img, p.box_in_img, p.depth = p.all_img[sel], np.asarray(idx, np.int32)[sel], depth[sel]
    p.rects = [r[sel] for r in rects]
    p.nb = [int((p.depth > l).sum()) for l in range(5)]
    p.top = max([l for l in range(5) if p.nb[l] > 0], default=-1)
    p.hw = []
    for l in range(5):
        r = p.rects[l][:p.nb[l]]
        p.hw.append(((r[:, 2] - r[:, 0]).astype(np.int64), (r[:, 3] - r[:, 1]).astype(np.int64)))
    return p


def _rows(p, l, nbox):
    h, w = p.hw[l]
    return int((h[:nbox] * w[:nbox]).sum())


def _tiles(p, l, nbox, th, tw):
    h, w = p.hw[l]
    return int((((h[:nbox] + th - 1) // th) * ((w[:nbox] + tw - 1) // tw)).sum())


def plan_routes(boxes, policy, crop_rects=None):
    """[(pass, level, conv, tag, info)] for every launch of the conv family and its companions that SegBranch makes for this population
    under `policy`, pass = "fwd" / "bwd"; info = {"M", "tiles", "fill", "wgs", ...} where it applies."""
    P, Pg = POLICY_PLANES[policy]
    p = plan(boxes, crop_rects)
    out = []
    if p.top < 0:
        return p, out

    def conv3(pas, l, conv, nbox, cin_pad, cout, xP, wP, yP, flip, t8):
        """SegBranch.rconv (k = 3: rows output, bias / ReLU forward, mask in the flipped launches, tables of 16 x 32 and 16 x 16 tiles, of 8-pixel
        tiles where t8) + ops.conv_halo"""
        M, t32 = _rows(p, l, nbox), _tiles(p, l, nbox, 16, 32)
        info = {"M": M, "tiles32": t32, "fill32": M / (t32 * 512.0)}
        if routes.ragged_conv(3, M, t32, cin_pad, cin_pad, cout, xP > 1 or wP > 1 or yP > 1, True, True) == "halo":
            entry = routes.halo_entry(3, cin_pad, cout, xP, wP, yP, 1, True, False, flip, flip, False, False, True, t8, True)
            if entry == "kg_conv3x3_ws":
                tag = "kg_conv3x3_ws/tiles8"
            elif entry == "kg_conv3x3_c64":
                tag = "kg_conv3x3_c64/tiles16" + ("+flip" if flip else "")
            else:
                Z = halo_ksplit(t32, cout, cin_pad, routes.vplanes(xP, wP))
                info.update(wgs=t32 * ((cout + 63) // 64), ksplit=Z)
                tag = "kg_conv2d_halo/tiles32" + ("+flip" if flip else "") + ("+split" if Z > 1 else "")
        else:
            tag = f"kg_conv2d_igemm/mode{3 if flip else 2} 3x3"
        out.append((pas, l, conv, tag, info))

    def conv1(pas, l, conv, M, cin_pad, rows_w, xP, wP, yP, flip):
        """SegBranch.rconv (k = 1) + ops.can_1x1"""
        ok = routes.ragged_conv(1, M, 0, cin_pad, cin_pad, rows_w, xP > 1 or wP > 1 or yP > 1, True, True) == "1x1"
        out.append((pas, l, conv, "kg_conv1x1" if ok else f"kg_conv2d_igemm/mode{3 if flip else 2} 1x1", {"M": M}))

    def wgrad(l, conv, nbox, k):
        """SegBranch.conv_bwd: the weight gradient"""
        M = _rows(p, l, nbox)
        if k == 3:
            t16 = _tiles(p, l, nbox, 16, 16)
            info = {"M": M, "tiles16": t16, "fill16": M / (t16 * 256.0)}
            tag = "kg_conv2d_wgrad_halo/tiles16" if routes.ragged_wgrad_halo(3, M, t16) else "kg_conv2d_wgrad/mode2 3x3"
        else:
            info, tag = {"M": M}, "kg_conv2d_wgrad/mode2 1x1"
        out.append(("bwd", l, conv, tag, info))

    def aux(pas, l, name):
        out.append((pas, l, name, name, {}))

    # ---- run_forward
    aux("fwd", -1, "kg_seg_build_rows_levels")
    aux("fwd", p.top, "kg_rows_gather_f32")
    for l in range(p.top - 1, -1, -1):
        cin, cout, ccat = SKIP[l]
        nc = p.nb[l + 1]
        if nc:
            aux("fwd", l, "kg_bilinear_fwd")
            conv3("fwd", l, f"skip_combine.{l}.up.0", nc, cin, cout, P, P, P, False, l == 0)
            conv1("fwd", l, f"skip_combine.{l}.cat_conv.0", _rows(p, l, nc), ccat, cout, P, P, P, False)
        aux("fwd", l, "kg_rows_gather_f32")
    conv3("fwd", 0, "seg_head.0", p.nb[0], 64, 64, P, P, P, False, True)
    aux("fwd", 0, "kg_seg_conv3_c1")
    # ---- _run_backward (packed transposed weights: x planes Pg, w planes min(Pg, pdw) = Pg)
    wgrad(0, "seg_head.2", p.nb[0], 3)
    conv3("bwd", 0, "seg_head.2", p.nb[0], 8, 64, Pg, Pg, Pg, True, False)            # cin_pad = round_up(1, 8): never a halo launch
    wgrad(0, "seg_head.0", p.nb[0], 3)
    conv3("bwd", 0, "seg_head.0", p.nb[0], 64, 64, Pg, Pg, Pg, True, False)
    for l in range(p.top):
        cin, cout, ccat = SKIP[l]
        nc = p.nb[l + 1]
        if nc:
            wgrad(l, f"skip_combine.{l}.cat_conv.0", nc, 1)
            conv1("bwd", l, f"skip_combine.{l}.cat_conv.0", _rows(p, l, nc), cout, ccat, Pg, Pg, Pg, True)
            wgrad(l, f"skip_combine.{l}.up.0", nc, 3)
            conv3("bwd", l, f"skip_combine.{l}.up.0", nc, cout, cin, Pg, Pg, Pg, True, False)
            aux("bwd", l, "kg_bilinear_bwd")
        aux("bwd", l, "kg_crop_grad_reduce")
    aux("bwd", p.top, "kg_crop_grad_reduce")
    return p, out


def route_set(routes, pas=None):
    return {r[3] for r in routes if pas is None or r[0] == pas}


# every route named in the coverage table: tag -> the pass it has to be planned (and observed) in
REQUIRED_FWD = ("kg_conv2d_igemm/mode2 3x3", "kg_conv2d_igemm/mode2 1x1", "kg_conv3x3_ws/tiles8", "kg_conv3x3_c64/tiles16",
                "kg_conv2d_halo/tiles32", "kg_conv2d_halo/tiles32+split", "kg_conv1x1", "kg_rows_gather_f32", "kg_bilinear_fwd", "kg_seg_conv3_c1",
                "kg_seg_build_rows_levels")
REQUIRED_BWD = ("kg_conv2d_wgrad_halo/tiles16", "kg_conv2d_wgrad/mode2 3x3", "kg_conv2d_wgrad/mode2 1x1", "kg_conv2d_igemm/mode3 3x3",
                "kg_conv2d_igemm/mode3 1x1", "kg_conv2d_halo/tiles32+flip", "kg_conv2d_halo/tiles32+flip+split", "kg_conv3x3_c64/tiles16+flip",
                "kg_conv1x1", "kg_bilinear_bwd", "kg_crop_grad_reduce")
# the family of kernel names (up to the template arguments) an entry point may report through kg_last_kernel
KERNEL_FAMILY = {"kg_conv3x3_ws": ("conv3_ws_kernel",), "kg_conv3x3_c64": ("conv3_c64_kernel",), "kg_conv2d_halo": ("conv_halo_kernel",),
                 "kg_conv1x1": ("conv1x1_kernel", "conv1x1_stream_kernel"),
                 "kg_conv2d_igemm": ("conv_igemm_kernel", "conv_gather_kernel", "conv_small_kernel", "conv_small_mfma_kernel", "conv_tiny_kernel"),
                 "kg_conv2d_wgrad_halo": ("conv_wgrad_halo_kernel", "wgrad_halo_kernel"),
                 "kg_conv2d_wgrad": ("conv_wgrad_kernel", "conv_wgrad_ring_kernel")}
TRACKED = set(KERNEL_FAMILY) | {"kg_rows_gather_f32", "kg_rows_gather", "kg_rows_gather_planes", "kg_bilinear_fwd", "kg_bilinear_bwd",
                                "kg_crop_grad_reduce", "kg_seg_conv3_c1", "kg_seg_build_rows_levels"}


def _null(p):
    return p is None or getattr(p, "value", p) in (None, 0)


def tag_of_call(name, args):
    """Route tag of one observed _lib.call (same vocabulary as plan_routes); None for calls outside the seg branch's conv family.
    Argument positions: include/kgnet_hip.h / _lib._SIGS."""
    if name not in TRACKED:
        return None
    if name == "kg_conv3x3_ws":
        return name + ("/tiles8" if not _null(args[11]) and args[12] > 0 else "/dense")
    if name == "kg_conv3x3_c64":
        return name + ("/tiles16" if not _null(args[17]) and args[18] > 0 else "/dense") + ("+flip" if args[15] else "")
    if name == "kg_conv2d_halo":
        if _null(args[22]) or args[23] <= 0:
            return name + "/dense"
        pl = args[25]
        aP, wP = (pl.contents.a_planes, pl.contents.w_planes) if pl is not None else (1, 1)
        Z = halo_ksplit(args[23], args[12], args[10], routes.vplanes(aP, wP)) if (args[17] == 3 and not _null(args[3]) and _null(args[4])) else 1
        return name + "/tiles32" + ("+flip" if args[18] else "") + ("+split" if Z > 1 else "")
    if name == "kg_conv2d_igemm":
        return name + f"/mode{args[25]} {args[20]}x{args[21]}" + ("" if not _null(args[7]) else " dense")
    if name == "kg_conv2d_wgrad_halo":
        return name + ("/tiles16" if not _null(args[15]) and args[16] > 0 else "/dense")
    if name == "kg_conv2d_wgrad":
        return name + f"/mode{args[20]} {args[15]}x{args[16]}"
    return name


# ---- the oracle runs --------------------------------------------------------------------------------------------------------------

SEG_PREFIXES = ("skip_combine.", "seg_head.")


class RecNet(onet.Net):
    """oracle.net.Net that keeps, per box, the ReLU state of every hidden tensor of the branch (the outputs of the ReLU'd convolutions, in the
    order forward_seg evaluates them: up / cat_conv from the top level down, then seg_head.0)"""

    def __init__(self, sd):
        super().__init__(sd, training=True)
        self.hidden = []          # [box in emission order][(conv name, bool [C, h, w])]
        self._cur = []

    def conv(self, x, name, stride=1, pad=0, relu=False):
        y = super().conv(x, name, stride, pad, relu)
        if relu and name.startswith(SEG_PREFIXES):
            self._cur.append((name, (y.detach() > 0)[0]))
            if name == "seg_head.0":
                self.hidden.append(self._cur); self._cur = []
        return y


def loss_weights(boxes, seed):
    """Seeded weights w of the loss sum((patch * w).sum()), one per kept box in emission order (image by image, input order), uniform in
    [0.5, 1.5).  POSITIVE on purpose: with weights of random sign (a normal draw) every parameter gradient is a sum of cancelling terms --
    for seg_head.2.weight on `disjoint` sum |t| / |sum t| = 880 -- and the per-tensor relative error then measures that condition number, not
    the kernels: rounding only the two operands of that one weight gradient to IEEE half and summing EXACTLY in float64 already gives a relative
    L2 error of 1.43e-3 (the GPU's default policy measured 1.39e-3), above the 2^-10 a convolution of 11-bit operands can add to a
    well-conditioned sum."""
    p = plan(boxes)
    g = torch.Generator().manual_seed(seed)
    ws = [[] for _ in range(p.nimg)]
    for b in range(len(p.all_boxes)):
        if p.all_depth[b] > 0:
            r = p.all_rects[0][b]
            ws[int(p.all_img[b])].append(0.5 + torch.rand(int(r[2] - r[0]), int(r[3] - r[1]), generator=g))
    return ws


class _PerImage:
    """The feature maps of one level as forward_seg indexes them (f.shape, f[i:i+1, :, y1:y2, x1:x2]) over one leaf tensor per image, so that
    the backward pass of a crop touches one image's map, not the whole batch's."""

    def __init__(self, imgs):
        self.imgs = imgs
        self.shape = (len(imgs),) + tuple(imgs[0].shape[1:])

    def __getitem__(self, idx):
        si, sc_, sy, sx = idx
        assert si.stop == si.start + 1 and sc_ == slice(None)
        return self.imgs[si.start][:, :, sy, sx]


class OracleRun:
    """oracle.net.Net.forward_seg on the given fp32 feature maps evaluated in `dtype` (the state dict is cast as oracle/gradref.py casts it).
    After the forward pass: logits / patch shapes / detections per image and the ReLU states of the hidden tensors per box; backward(wts)
    back-propagates the loss sum((patch * w).sum()) and leaves the feature gradients (None above the top level) and parameter gradients."""

    def __init__(self, sd, feats, boxes, dtype=torch.float64, grad=True):
        self.dtype = dtype
        self.sd = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items() if k.startswith(SEG_PREFIXES)}
        if grad:
            for v in self.sd.values():
                v.requires_grad_(True)
        net = RecNet(self.sd)
        self.fo = [[f[i:i + 1].detach().clone().to(dtype).requires_grad_(grad) for i in range(f.shape[0])] for f in feats]
        with torch.set_grad_enabled(grad):      # (the maps are ReLU outputs: their gradient carries that mask)
            self.patches, self.dets = net.forward_seg([_PerImage([F.relu(f) for f in ff]) for ff in self.fo], as_list(boxes))
        self.logits = [[z.detach() for z in zz] for zz in net.seg_logits]
        self.shapes = [[tuple(z.shape) for z in zz] for zz in net.seg_logits]
        self.hidden = net.hidden
        self.gfeat = self.gparam = None

    def backward(self, wts):
        terms = [(pt * w.to(self.dtype)).sum() for pp, ww in zip(self.patches, wts) for pt, w in zip(pp, ww)]
        if terms:
            sum(terms).backward()
        self.gfeat = []
        for ff in self.fo:          # a level no box reaches has no gradient at all; an image without boxes has a zero gradient
            self.gfeat.append(None if all(f.grad is None for f in ff) else torch.cat([f.grad if f.grad is not None else torch.zeros_like(f) for f in ff], 0))
        self.gparam = {n: v.grad for n, v in self.sd.items()}
        self.patches = None
        return self


def flipped_units(hidden, ref_hidden):
    """[(box in emission order, level, "hid" | "pre", y, x)] -- the pixels of the hidden tensors of every box at which at least one channel differs in
    its ReLU state between two forward passes (the rule of gradref.flipped_units, per pixel instead of per channel: the gradient that passes
    through such a unit is present in one run and absent in the other -- a difference of the size of that contribution, not of rounding)."""
    out = []
    for k, (ha, hb) in enumerate(zip(hidden, ref_hidden)):
        assert [n for n, _ in ha] == [n for n, _ in hb], (k, [n for n, _ in ha], [n for n, _ in hb])
        for (name, a), (_, b) in zip(ha, hb):
            d = (a != b).any(0)
            if bool(d.any()):
                l = 0 if name == "seg_head.0" else int(name.split(".")[1])
                for y, x in torch.nonzero(d).tolist():
                    out.append((k, l, "hid" if name == "seg_head.0" else "pre", y, x))
    return sorted(set(out))


def _bilinear_taps(n_in, n_out):
    """F.interpolate(mode="bilinear", align_corners=False): the two input indices every output index reads"""
    src = np.maximum((np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    return i0, np.minimum(i0 + 1, n_in - 1)


def _window_1d(sizes, l, q, kind):
    """inclusive interval of level-0 logit positions whose loss gradient reaches the hidden unit at position q of level l (one axis).
    From a level-l output of cat_conv / up (`pre`): bilinear upsampling to level l - 1, the 3x3 up conv, the 1x1 cat_conv, ... down to level 0,
    then seg_head.0 and seg_head.2 (3x3 each); from seg_head.0's output (`hid`): seg_head.2 alone."""
    a = b = q
    while l > 0:
        i0, i1 = _bilinear_taps(int(sizes[l]), int(sizes[l - 1]))
        hit = np.nonzero(((i0 >= a) & (i0 <= b)) | ((i1 >= a) & (i1 <= b)))[0]
        if len(hit) == 0:
            return None
        a, b = int(hit.min()) - 1, int(hit.max()) + 1
        l -= 1
    r = 1 if kind == "hid" else 2
    return max(a - r, 0), min(b + r, int(sizes[0]) - 1)


def mask_weights(wts, boxes, units):
    """Sets the loss weights to zero wherever the loss gradient could reach one of `units` (flipped_units): such a unit then receives exactly zero
    gradient in every implementation, whatever its ReLU state.  Returns (new weights, share of the loss pixels set to zero)."""
    p = plan(boxes)
    kept = [b for b in range(len(p.all_boxes)) if p.all_depth[b] > 0]          # emission order
    flat = [w.clone() for ww in wts for w in ww]
    for k, l, kind, y, x in units:
        b = kept[k]
        hs = [int(p.all_rects[j][b][2] - p.all_rects[j][b][0]) for j in range(int(p.all_depth[b]))]
        ws = [int(p.all_rects[j][b][3] - p.all_rects[j][b][1]) for j in range(int(p.all_depth[b]))]
        wy, wx = _window_1d(hs, l, y, kind), _window_1d(ws, l, x, kind)
        if wy is None or wx is None:
            continue
        flat[k][wy[0]:wy[1] + 1, wx[0]:wx[1] + 1] = 0
    total = sum(w.numel() for w in flat)
    nz = sum(int((w == 0).sum()) for w in flat)
    out, i = [], 0
    for ww in wts:
        out.append(flat[i:i + len(ww)]); i += len(ww)
    return out, nz / max(total, 1)


# ---- metrics ------------------------------------------------------------------------------------------------------------------------

def rel_l2(got, ref):
    a, b = got.detach().double().cpu().flatten(), ref.detach().double().cpu().flatten()
    nb, d = float(b.norm()), float((a - b).norm())
    return d / nb if nb > 0 else (0.0 if d == 0 else float("inf"))


def max_rel(got, ref):
    """max |d| / max |ref|"""
    a, b = got.detach().double().cpu(), ref.detach().double().cpu()
    m, d = float(b.abs().max()), float((a - b).abs().max())
    return d / m if m > 0 else (0.0 if d == 0 else float("inf"))


def regions(boxes):
    """[(emission index of the box, image, level, (y1, x1, y2, x2))] for every kept box and every level below its depth"""
    p = plan(boxes)
    out, k = [], 0
    for b in range(len(p.all_boxes)):
        if p.all_depth[b] == 0:
            continue
        for l in range(int(p.all_depth[b])):
            out.append((k, int(p.all_img[b]), l, tuple(int(v) for v in p.all_rects[l][b])))
        k += 1
    return out


def region_metrics(gfeat, ref, boxes):
    """{(box, level): (relative L2, max |d| / max |ref|)} of the feature gradients inside every box's crop rectangle"""
    out = {}
    for k, i, l, (y1, x1, y2, x2) in regions(boxes):
        a, b = gfeat[l][i, :, y1:y2, x1:x2], ref[l][i, :, y1:y2, x1:x2]
        out[(k, l)] = (rel_l2(a, b), max_rel(a, b))
    return out


def outside_mask(boxes, l):
    """bool [N, H_l, W_l]: pixels of level l that no kept box's crop rectangle covers"""
    m = torch.ones(len(boxes), *SIZES[l], dtype=torch.bool)
    for k, i, ll, (y1, x1, y2, x2) in regions(boxes):
        if ll == l:
            m[i, y1:y2, x1:x2] = False
    return m


def n_conv_feature(l, combine):
    """backward convolutions on the longest path from the loss to the level-l feature gradient, the producing one included (SegBranch._run_backward:
    seg_head.2 dgrad, seg_head.0 dgrad, then per level cat_conv dgrad [-> the feature columns of a combine box] and up dgrad [-> next level])"""
    return (3 if combine else 2) + 2 * l


def n_conv_param(name):
    """... to a parameter gradient: the weight gradient itself plus the input gradients that produced its dY operand"""
    if name.startswith("seg_head.2"):
        return 1
    if name.startswith("seg_head.0"):
        return 2
    l = int(name.split(".")[1])
    return (3 if ".cat_conv." in name else 4) + 2 * l
