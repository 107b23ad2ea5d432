"""Which kernel does every ragged launch of the seg branch take, per box population?  (no GPU needed)

SegBranch routes its ragged convolutions by the DATA (tile fill, workgroup count, depth of every box).  oracle/segcases.py defines box
populations and plans the route of every launch from the host planner's answers (routes.py) and launch_halo's restated split (`plan_routes`); here the COVERAGE TABLE is asserted: every route of
SegBranch.rconv / conv_bwd / ops.conv_halo / launch_halo is planned by at least one population, so that tests/test_gpu_seg_routes.py -- which
asserts that the launches observed on the GPU equal the planned ones, and compares every box with the float64 oracle -- exercises all of them.
A change of a threshold, of a population or of the routing that makes a route unreachable fails HERE, naming the route.

Also here, because they need no GPU:
  * seg.crop_rects against oracle.net.Net.crop_coords on every population (clipped, rejected, half-to-even boxes included);
  * the proof that the per-region metrics of the gradient test see what they have to see: three mutations of the float64 oracle's own feature
    gradients (a crop shifted by one pixel, a zeroed last row, two boxes of equal crop size exchanged) each drive both metrics of the
    mutated box above 1e-2 -- the cap no per-region bound of the GPU test may exceed -- for the smallest and the largest box of `disjoint`;
  * the float32 oracle's ReLU flips against float64 (oracle/segcases.py flipped_units / mask_weights) stay under the cap of 1 loss pixel in 10
    on every population -- the same cap the GPU runs are held to."""
import numpy as np
import pytest
import torch

from oracle import segcases as sc

POPS = sc.populations()
FWD_POLICIES, BWD_POLICIES = ("fp32", "half", "bf16"), ("fp32b2", "fp32")
CAP = 1e-2


@pytest.fixture(scope="module")
def cal_sd():
    from oracle import weightgen
    return weightgen.gen_state_dict(0, variant="cal")


def test_population_names_and_shapes():
    assert tuple(POPS) == sc.NAMES
    for name, boxes in POPS.items():
        for bb in boxes:
            assert bb is None or (bb.dtype == np.float32 and bb.ndim == 2 and bb.shape[1] == 5), name
    assert 3 <= len(POPS["big"][0]) <= 4 and any(tuple(b[:4]) == (0, 0, sc.H0, sc.W0) for b in POPS["big"][0])
    t = np.concatenate(POPS["tiny"])
    sides = np.concatenate([t[:, 2] - t[:, 0], t[:, 3] - t[:, 1]])
    assert len(t) >= 40 and sides.min() >= 2.6 and sides.max() <= 9.0
    assert len(POPS["crowd"]) == 3 and len(POPS["crowd"][0]) >= 150 and POPS["crowd"][1] is None and 1 <= len(POPS["crowd"][2]) <= 8
    assert len(POPS["disjoint"]) == 2 and 8 <= sum(len(b) for b in POPS["disjoint"]) <= 12


@pytest.mark.parametrize("name", sc.NAMES)
def test_crop_rects_match_oracle_on_population(name):
    from kg_instance_segmentation_amd.seg import crop_rects
    from oracle.net import Net
    boxes = np.concatenate(sc.as_list(POPS[name]))
    rects, depth = crop_rects(boxes[:, :4], sc.H0, sc.W0, sc.SIZES)
    for b in range(len(boxes)):
        d = 0
        for l, (h, w) in enumerate(sc.SIZES):
            cc = Net.crop_coords(boxes[b, :4], sc.H0, sc.W0, h, w)
            if cc is None:
                break
            assert tuple(rects[l][b]) == cc, (name, b, l)
            d += 1
        assert d == depth[b], (name, b)


def test_halfeven_population_sits_on_the_accept_reject_edge():
    p = sc.plan(POPS["halfeven"])
    d = p.all_depth.tolist()
    assert d[0] >= 1 and d[1] == 0 and d[2] >= 1 and d[3] >= 1 and d[4] == 0            # exactly 2 / just under 2 at level 0
    assert int(p.all_rects[0][0][2] - p.all_rects[0][0][0]) == 2 and int(p.all_rects[0][2][2] - p.all_rects[0][2][0]) == 2
    assert d[7] == 5 and int(p.all_rects[4][7][2] - p.all_rects[4][7][0]) == 2 and d[8] == 4                    # ... at level 4
    assert d[9] == 4 and all(tuple(p.all_rects[l][9][2:] - p.all_rects[l][9][:2]) == (2, 2) for l in (2, 3))       # ... at levels 2 and 3 (12.5 -> 12, 13.5 -> 14)
    assert tuple(p.all_rects[1][5][[1, 3]]) == (10, 24)                                                        # 10.5 -> 10, 23.5 -> 24


def test_coverage_table():
    """every route is planned by at least one population (the table of DESIGN.md section 5, "Seg branch routes")"""
    fwd, bwd = {}, {}
    for name, boxes in POPS.items():
        for pol in FWD_POLICIES:
            for pas, l, conv, tag, info in sc.plan_routes(boxes, pol)[1]:
                if pas == "fwd":
                    fwd.setdefault(tag, set()).add((name, pol, l, conv))
        for pol in BWD_POLICIES:
            for pas, l, conv, tag, info in sc.plan_routes(boxes, pol)[1]:
                if pas == "bwd":
                    bwd.setdefault(tag, set()).add((name, pol, l, conv))
    for tag in sc.REQUIRED_FWD:
        assert tag in fwd, f"no population plans the forward route {tag}"
    for tag in sc.REQUIRED_BWD:
        assert tag in bwd, f"no population plans the backward route {tag}"
    for tag, users in sorted(fwd.items()) + sorted(bwd.items()):
        print(tag, sorted({u[0] for u in users}))


def test_populations_are_what_they_are_for():
    plans = {n: sc.plan(b) for n, b in POPS.items()}
    routes = {(n, pol): sc.plan_routes(b, pol)[1] for n, b in POPS.items() for pol in ("fp32", "half", "fp32b2")}
    # big: LDS-halo kernels for the forward 3x3 convs and the weight gradients of levels 0..3, with and without the channel split
    for pol in ("fp32", "half"):
        r = routes[("big", pol)]
        assert all(tag.startswith(("kg_conv2d_halo", "kg_conv3x3_")) for pas, l, conv, tag, _ in r if pas == "fwd" and conv.endswith((".up.0", "seg_head.0")))
        assert all(tag == "kg_conv2d_wgrad_halo/tiles16" for pas, l, conv, tag, _ in r if pas == "bwd" and tag.startswith("kg_conv2d_wgrad") and "1x1" not in tag)
        assert {"kg_conv2d_halo/tiles32", "kg_conv2d_halo/tiles32+split"} <= sc.route_set(r, "fwd")
    # tiny: gather kernels everywhere, the top level below 4, boxes ending at levels 0, 1 and 2
    assert plans["tiny"].top < 4 and set(plans["tiny"].depth.tolist()) >= {1, 2, 3}
    for pol in ("fp32", "half", "fp32b2"):
        assert not any("halo" in tag or "tiles" in tag for _, _, _, tag, _ in routes[("tiny", pol)])
    # ladder: every depth 0..5, a 2 x 2 crop inside the level-0 halo launch, forward and weight gradient on different routes at one level
    assert set(plans["ladder"].all_depth.tolist()) == {0, 1, 2, 3, 4, 5}
    h0, w0 = plans["ladder"].hw[0]
    assert ((h0 == 2) & (w0 == 2)).any()
    r = routes[("ladder", "fp32")]
    assert [tag for pas, l, conv, tag, _ in r if pas == "fwd" and conv == "seg_head.0"] == ["kg_conv3x3_ws/tiles8"]
    split = [l for l in range(4) if any(pas == "fwd" and ll == l and tag == "kg_conv2d_igemm/mode2 3x3" for pas, ll, _, tag, _ in r)
             and any(pas == "bwd" and ll == l and tag == "kg_conv2d_wgrad_halo/tiles16" and conv.endswith(".up.0") for pas, ll, conv, tag, _ in r)]
    assert split, "no level of `ladder` runs its forward conv on the gather kernel and its weight gradient on the halo kernel"
    b = np.concatenate(sc.as_list(POPS["ladder"]))
    assert (b[:, :2] < 0).any() and (b[:, 2] > sc.H0).any() and (b[:, 3] > sc.W0).any()          # clipping on all sides
    # crowd: an unsplit ragged kg_conv2d_halo launch (tiles x cout blocks > 128), an image without boxes
    assert any(tag == "kg_conv2d_halo/tiles32" and info["wgs"] > sc.HALO_SPLIT_WGS for _, _, _, tag, info in routes[("crowd", "fp32")])
    assert not (plans["crowd"].img == 1).any()
    # disjoint: crop rectangles pairwise disjoint at every level; two pairs of identical crop size, one small and one large
    reg = sc.regions(POPS["disjoint"])
    for a in range(len(reg)):
        for c in range(a + 1, len(reg)):
            (ka, ia, la, ra), (kc, ic, lc, rc) = reg[a], reg[c]
            if ka != kc and ia == ic and la == lc:
                assert ra[2] <= rc[0] or rc[2] <= ra[0] or ra[3] <= rc[1] or rc[3] <= ra[1], (reg[a], reg[c])
    small, large = equal_size_pairs()
    assert small and large


def crop_sizes(boxes):
    """{box (emission order): ((h, w) per level below its depth)}"""
    out = {}
    for k, i, l, (y1, x1, y2, x2) in sc.regions(boxes):
        out.setdefault(k, []).append((y2 - y1, x2 - x1))
    return {k: tuple(v) for k, v in out.items()}


def equal_size_pairs():
    """(smallest, largest) pair of boxes of `disjoint` with identical crop sizes at every level"""
    cs = crop_sizes(POPS["disjoint"])
    pairs = sorted(((cs[a][0][0] * cs[a][0][1], a, b) for a in cs for b in cs if a < b and cs[a] == cs[b]))
    assert len(pairs) >= 2, pairs
    return pairs[0][1:], pairs[-1][1:]


def test_backward_bound_derivation():
    """n_conv of the issue's derivation, counted from SegBranch._run_backward: seg_head.2 weight 1; level-l feature gradient 2 + 2 l inside a
    box that ends there, 3 + 2 l inside one that goes on; the deepest is 10, so no derived bound exceeds 10 * 2^-10 = 9.8e-3 < the cap"""
    assert sc.n_conv_param("seg_head.2.weight") == 1 and sc.n_conv_param("seg_head.0.bias") == 2
    assert sc.n_conv_param("skip_combine.0.cat_conv.0.weight") == 3 and sc.n_conv_param("skip_combine.3.up.0.weight") == 10
    assert [sc.n_conv_feature(l, False) for l in range(5)] == [2, 4, 6, 8, 10] and [sc.n_conv_feature(l, True) for l in range(4)] == [3, 5, 7, 9]
    assert 10 * 2.0 ** -10 < CAP


def test_halo_split_rule():
    """launch_halo's chunk split restated (csrc/conv_halo.hip): at most 128 workgroups, >= 2 chunks per part, <= 8 parts"""
    assert sc.halo_ksplit(16, 512, 1024, 3) == 2 and sc.halo_ksplit(16, 512, 1024, 1) == 2       # 128 workgroups
    assert sc.halo_ksplit(17, 512, 1024, 1) == 1                                                 # 136 workgroups
    assert sc.halo_ksplit(31, 64, 256, 3) == 6 and sc.halo_ksplit(10, 64, 256, 1) == 2 and sc.halo_ksplit(4, 64, 64, 1) == 1


@pytest.fixture(scope="module")
def disjoint_f64(cal_sd):
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    boxes = POPS["disjoint"]
    run = sc.OracleRun(cal_sd, sc.features(boxes, sc.seed_of("disjoint")), boxes, torch.float64)
    run.backward(sc.loss_weights(boxes, 7))
    return run


def _mutants(gfeat, kind, k, other=None):
    """the float64 feature gradients with box k's region mutated at EVERY level below its depth"""
    out = [g.clone() if g is not None else None for g in gfeat]
    reg = {(kk, l): (i, r) for kk, i, l, r in sc.regions(POPS["disjoint"])}
    for (kk, l), (i, (y1, x1, y2, x2)) in reg.items():
        if kk != k:
            continue
        src = gfeat[l][i, :, y1:y2, x1:x2]
        if kind == "shift":             # the crop taken one pixel further right
            out[l][i, :, y1:y2, x1:x2] = torch.roll(src, 1, 2)
        elif kind == "last_row":
            out[l][i, :, y2 - 1, x1:x2] = 0
        else:                           # the regions of two boxes of equal crop size exchanged
            j, (v1, u1, v2, u2) = reg[(other, l)]
            out[l][i, :, y1:y2, x1:x2] = gfeat[l][j, :, v1:v2, u1:u2]
            out[l][j, :, v1:v2, u1:u2] = src
    return out


@pytest.mark.parametrize("kind", ["shift", "last_row", "swap"])
def test_region_metrics_see_a_one_pixel_error(disjoint_f64, kind):
    """each mutation drives BOTH per-region metrics of the mutated box above the cap at every level, for the smallest and the largest box"""
    ref = disjoint_f64.gfeat
    small, large = equal_size_pairs()
    clean = sc.region_metrics(ref, ref, POPS["disjoint"])
    assert all(v == (0.0, 0.0) for v in clean.values())
    for k, other in (small, large):
        m = sc.region_metrics(_mutants(ref, kind, k, other), ref, POPS["disjoint"])
        mine = {kl: v for kl, v in m.items() if kl[0] == k}
        print(kind, k, {kl[1]: (round(v[0], 3), round(v[1], 3)) for kl, v in mine.items()})
        assert mine and all(v[0] > CAP and v[1] > CAP for v in mine.values()), (kind, k, mine)
        untouched = {kl: v for kl, v in m.items() if kl[0] not in (k, other if kind == "swap" else k)}
        assert all(v == (0.0, 0.0) for v in untouched.values())


@pytest.mark.parametrize("name", sc.NAMES)
def test_float32_oracle_flips_stay_under_the_cap(cal_sd, name):
    """the float32 oracle's ReLU flips against float64, and the share of the loss pixels their windows take: at most 1 in 10"""
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    boxes = POPS[name]
    feats = sc.features(boxes, sc.seed_of(name))
    r64 = sc.OracleRun(cal_sd, feats, boxes, torch.float64, grad=False)
    r32 = sc.OracleRun(cal_sd, feats, boxes, torch.float32, grad=False)
    units = sc.flipped_units(r32.hidden, r64.hidden)
    wts, share = sc.mask_weights(sc.loss_weights(boxes, 7), boxes, units)
    print(name, len(units), "flipped pixels, share of the loss pixels set to zero", share)
    assert share <= 0.1, (name, len(units), share)
    rms = [float(z.double().pow(2).mean().sqrt()) for zz in r64.logits for z in zz]
    assert 0.01 <= min(rms) and max(rms) <= 0.68, (min(rms), max(rms))       # the range EVAL_TOL's fp32 bound is proven on (golden `b`: 0.018 .. 0.68)


def test_flip_window_covers_every_loss_pixel_that_reaches_the_unit(cal_sd):
    """mask_weights' windows are exact enough: with the loss weights zeroed inside the window of a hidden unit, that unit's pre-activation receives
    a gradient of exactly zero in the float64 oracle (checked on one deep box of `halfeven`, one unit per hidden tensor)."""
    from oracle import net as onet
    boxes = [POPS["halfeven"][0][[6]]]          # depth 5
    feats = sc.features(boxes, 5)
    sd = {k: v.double() for k, v in cal_sd.items() if k.startswith(sc.SEG_PREFIXES)}
    kept = []

    class Keep(onet.Net):
        def conv(self, x, name, stride=1, pad=0, relu=False):
            y = super().conv(x, name, stride, pad, relu)
            if relu:
                y.retain_grad(); kept.append((name, y))
            return y
    fo = [f.double().requires_grad_(True) for f in feats]
    patches, _ = Keep(sd, training=True).forward_seg(fo, boxes)
    units = []
    for name, y in kept:
        l = 0 if name == "seg_head.0" else int(name.split(".")[1])
        units.append((0, l, "hid" if name == "seg_head.0" else "pre", y.shape[2] // 2, y.shape[3] // 3))
    w, share = sc.mask_weights(sc.loss_weights(boxes, 3), boxes, units)
    assert 0 < share < 1
    (patches[0][0] * w[0][0].double()).sum().backward()
    for (name, y), (_, l, kind, yy, xx) in zip(kept, units):
        assert float(y.grad[0, :, yy, xx].abs().max()) == 0.0, name
        assert float(y.grad.abs().max()) > 0.0, name
