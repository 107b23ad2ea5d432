"""Which kernel does every DENSE convolution launch take, and does a small parity case stand behind every class?  (no GPU needed)

oracle/densecases.py asks the host planner (routes.py) what ops.conv_auto / conv_halo / conv_wgrad will call, restates the library's launchers (launch_halo,
kg_launch_conv_gather, kg_launch_conv_tiny, kg_conv1x1, kg_conv2d_wgrad, kg_conv2d_wgrad_halo, kg_launch_conv_small, kg_conv2d_halo_heads2) as host
arithmetic and lists one parity case per launch class.  tests/test_gpu_dense_routes.py runs the cases and asserts that the library launches what the
plan says.  Here the TABLE is asserted:
  * every case plans the kernel, split state and python-level kind it is meant to hit;
  * every dense class of the newest committed profiles/r*_bench_launches.txt has a case whose key covers it, every ragged class is in SEG_FAMILY
    with a route of tests/test_gpu_seg_routes.py; every kernel name a dense launcher can note has a case; deleting a case fails with the class;
  * both sides of every fill threshold plan different keys;
  * the bound of every case SEES one lost unit of work: the float64 reference with one (tap, 8-channel group) slice removed -- for weight
    gradients one 64-pixel chunk -- violates the bound on at least one element, and the float32 evaluation of the reference never does;
  * the channel split of the planner is segcases.halo_ksplit's."""
import glob
import os

import pytest
import torch

from oracle import densecases as dc, segcases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = {c.name: dc.plan(c) for c in dc.CASES}


def newest_census():
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_bench_launches.txt")))
    assert files, "no committed launch census"
    with open(files[-1]) as f:
        return os.path.basename(files[-1]), dc.parse_census(f.read())


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.name)
def test_case_plans_what_it_is_meant_to_hit(case):
    kind, key, _ = PLANS[case.name]
    assert (kind, key.kernel, key.split) == (case.kind, case.kernel, case.split), (case, kind, key)
    assert key.fmt == case.fmt and key.kernel in dc.KERNEL_NAMES


def uncovered_census_classes(cases):
    keys = [dc.plan(c)[1] for c in cases]
    name, census = newest_census()
    return [(k, line.strip()) for k, seg, line in census if k is not None and not any(dc.covers(ck, k) for ck in keys)]


def test_every_dense_census_class_has_a_case():
    name, census = newest_census()
    assert len(census) >= 100 and sum(k is not None for k, _, _ in census) >= 80, (name, len(census))
    missing = uncovered_census_classes(dc.CASES)
    assert not missing, f"{name}: launch classes without a parity case:\n" + "\n".join(f"{k}\n    {l}" for k, l in missing)


def test_every_ragged_census_class_belongs_to_the_seg_tests():
    name, census = newest_census()
    ragged = {seg for k, seg, _ in census if k is None}
    assert ragged, name
    for cls in sorted(ragged):
        assert cls in dc.SEG_FAMILY, f"{name}: ragged class {cls} is neither dense nor in SEG_FAMILY"
        assert dc.SEG_FAMILY[cls] in sc.REQUIRED_FWD + sc.REQUIRED_BWD, cls
    for route in dc.SEG_FAMILY.values():
        assert route in sc.REQUIRED_FWD + sc.REQUIRED_BWD, route


def test_every_kernel_name_has_a_case():
    planned = {key.kernel for _, key, _ in PLANS.values()}
    for kern in dc.KERNEL_NAMES:
        assert kern in planned, f"no case plans kernel {kern}"
    assert not set(dc.KERNEL_NAMES) & set(dc.UNREACHABLE)
    for kern in planned:
        assert kern in dc.KERNEL_NAMES, kern


def test_every_noted_name_of_the_sources_is_listed():
    """the hand-written list against the kg_note_kernel calls of csrc/*.hip: a literal name that is neither in KERNEL_NAMES nor in UNREACHABLE
    (nor a seg-branch / measurement-only note) is a launcher the table does not know"""
    import re
    src = os.path.join(ROOT, "kg_instance_segmentation_amd", "csrc")
    lit = set()
    for f in ("conv_halo.hip", "conv_gather.hip", "conv_tiny.hip", "conv_small.hip", "conv1x1.hip", "conv_wgrad.hip", "conv7_narrow.hip", "conv3_c64.hip", "conv3_ws.hip"):
        with open(os.path.join(src, f)) as fh:
            text = fh.read()
        for m in re.finditer(r"kg_note_kernel\(([^;]*)\);", text):
            lit |= set(re.findall(r'"([^"%]+)"', m.group(1)))
        if f == "conv_wgrad.hip":
            lit |= set(re.findall(r'"(conv_wgrad_ring_kernel<\d, \d>)"', text))
    known = set(dc.KERNEL_NAMES) | set(dc.UNREACHABLE)
    for name in sorted(lit):
        if "/unsplit" in name:
            continue          # (heads2 beyond the scratch cap: a note about a dropped split, not a kernel)
        assert name in known, f"csrc notes kernel {name!r}: add a case or an UNREACHABLE entry with its reason"


def lost_classes(cases):
    have = {dc.class_id(c) for c in cases}
    return [r for r in dc.REQUIRED if r not in have]


def test_every_required_class_has_exactly_one_hand_written_case():
    """densecases.REQUIRED is the written-out list of launch classes the hand-written table has to cover (one line per class: key + trait)"""
    ids = [dc.class_id(c, PLANS[c.name][1]) for c in dc.HAND]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    lost = lost_classes(dc.HAND)
    assert not lost, "launch classes that lost their cover:\n" + "\n".join(lost)
    extra = sorted(set(ids) - set(dc.REQUIRED))
    assert not extra, "cases whose class is not listed in REQUIRED:\n" + "\n".join(extra)


def uncovered_recorded_keys(cases):
    keys = [dc.plan(c)[1] for c in cases if not c.env]
    return [k for k in dc.CENSUS_64 if not any(dc.covers(ck, k) for ck in keys)]


def test_every_recorded_train_step_class_has_a_generated_case():
    """densecases.CENSUS_64 (the full keys of the 2 x 64 x 64 train step that no hand-written case reproduces): the shape search finds a case for
    every key, its plan IS the key, and no key is redundant (covered by a hand-written case or by another generated one)"""
    assert all(c is not None for c in dc.GENERATED), [str(k) for k, c in zip(dc.CENSUS_64, dc.GENERATED) if c is None]
    for k, c in zip(dc.CENSUS_64, dc.GENERATED):
        assert PLANS[c.name][1] == k, (k, PLANS[c.name][1])
    assert not uncovered_recorded_keys(dc.CASES)
    hand = [PLANS[c.name][1] for c in dc.HAND if not c.env]
    assert not [k for k in dc.CENSUS_64 if any(dc.covers(h, k) for h in hand)]


def test_deleting_any_one_case_fails_with_the_name_of_its_class():
    for victim in dc.HAND:
        lost = lost_classes([c for c in dc.HAND if c is not victim])
        assert lost == [dc.class_id(victim, PLANS[victim.name][1])], (victim, lost)
    for victim in dc.GENERATED:
        lost = uncovered_recorded_keys([c for c in dc.CASES if c is not victim])
        assert lost == [PLANS[victim.name][1]], (victim, lost)
    # and for the classes the workload launches: without the cases of a kernel the bench census test names the uncovered lines
    for kern in ("conv_halo7_w4_kernel<false, 2> + " + dc.H7, "conv1x1_stream_kernel<2, 1>", "wgrad_halo_kernel<7, 2, 1, true>"):
        lost = uncovered_census_classes([c for c in dc.CASES if PLANS[c.name][1].kernel != kern])
        assert lost and all(k.kernel == kern for k, _ in lost), (kern, lost)


@pytest.mark.parametrize("a,b", dc.THRESHOLD_PAIRS)
def test_threshold_pairs_plan_different_keys(a, b):
    ka, kb = PLANS[a][1], PLANS[b][1]
    assert ka != kb and (ka.kernel, ka.split) != (kb.kernel, kb.split), (a, b, ka, kb)
    assert ka.entry == kb.entry


def test_channel_split_is_halo_ksplit():
    """launch_halo's Z through the planner == segcases.halo_ksplit on shared inputs; the dense cases sit on both sides of its limits"""
    seen = set()
    for tiles in (1, 2, 7, 12, 16, 32, 43, 64, 65, 128, 129, 198):
        for cout in (40, 64, 128, 200, 256):
            for cin_pad, vp in ((64, 1), (128, 1), (256, 1), (1024, 1), (64, 3), (128, 3), (512, 3)):
                z = sc.halo_ksplit(tiles, cout, cin_pad, vp)
                with dc.environment({"KG_HALO3_NB2": "0"}):
                    kern, split = dc.launch_halo(3, tiles, cout, cin_pad, vp, False, True, False, None)
                assert kern == dc.H3 and split == (z > 1), (tiles, cout, cin_pad, vp, z, kern, split)
                assert dc.launch_halo(3, tiles, cout, cin_pad, vp, False, False, False, None)[1] is False       # an fp32 export is never split
                seen.add(z)
    assert {1, 2, 4, 8} <= seen, seen
    with dc.environment({"KG_HALO_SPLIT": "0"}):
        assert dc.launch_halo(3, 12, 64, 256, 1, False, True, False, None) == (dc.H3, False)
    assert dc.launch_halo(3, 12, 64, 256, 1, False, True, False, None) == (dc.H3, True)


_REFS = {}


def ref_of(case):
    if case.name not in _REFS:
        _REFS.clear()          # (one at a time: the threshold-sized cases hold a few hundred MB)
        torch.set_num_threads(min(torch.get_num_threads(), 16))
        _REFS[case.name] = dc.Reference(case)
    return _REFS[case.name]


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.name)
def test_bound_sees_one_lost_unit_of_work(case):
    """the float64 reference itself and its float32 evaluation are inside the bound; the reference minus one (tap, 8-channel group) slice / one
    64-pixel chunk is outside on at least one element"""
    r = ref_of(case)
    for which, d in enumerate(r.outs):
        assert float(d["bound"].min()) > 0 and d["allow"] <= 1e-3 * max(d["rms"], 1e-30), (case, which, d["allow"], d["rms"])
        nbad, worst = r.violations(d["f32"], which)
        assert nbad == 0, (case, which, worst)
        nbad, worst = r.violations(r.mutant(which), which)
        print(f"[{case.name} out {which}] rms {d['rms']:.3g} allowance {d['allow']:.3g} (float32 yardstick {d['yard']:.3g}) u_out {d['u']:.3g}; "
              f"mutant: {nbad} of {d['ref'].numel()} elements outside, worst |d| / bound {worst:.3g}")
        assert nbad >= 1, (case, which, worst)
