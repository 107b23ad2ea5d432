"""Do the parity cases of the step tail run every index path, and do their bounds bite?  (no GPU needed)

oracle/tailcases.py restates the launch geometry of the kernels that run after the last conv of a train step (the two losses, sigmoid_, grad_pack /
grad_pack3, grad_scale, scale_tensors, the split weight-gradient reductions and their deferred flush, bias_grad, the batched weight pack, the fused
Adam), lists the cases and builds float64 references, bounds and mutants; tests/test_gpu_tail.py runs the cases on the device.  Here the TABLE and the
BOUNDS are asserted before any kernel runs:
  * every index path the restated geometry can return for a tensor below 64 M elements is claimed by a case (claims are computed), or is listed as
    left out with the size it would need;
  * the float32 CPU evaluation of every case sits within every bound;
  * every mutant does not: one 16-byte chunk unwritten or taken from its neighbour (pack, scale, Adam, sigmoid), one pixel dropped from a loss sum,
    the second grid-stride trip skipped in the capped loss case, one split dropped / one group summing its neighbour's range / the groups added in
    reverse order in a reduction, one row dropped from a bias sum, the planted element missed by the grad_scale maximum, one job of a table run with
    its neighbour's size;
  * float32 and float64 agree on the binade of every grad_scale maximum;
  * the job -> block layouts of tailcases equal what ops.scale_tensors and PackQueue.flush build (h2d and the library call stubbed)."""
import collections

import numpy as np
import pytest
import torch

from oracle import tailcases as tc

WORST = collections.defaultdict(float)


def note(k, v):
    WORST[k] = max(WORST[k], v)
    return v


def ids(cases):
    return [c.name for c in cases]


# ---- every path has a case ------------------------------------------------------------------------------------------------------------------------

def test_every_index_path_is_claimed_by_a_case():
    tabs = [tc.table_claims([(n, (off,)) for n, off, _ in c.jobs]) for c in tc.SCALE_CASES]
    paths = set().union(*[t["paths"] for t in tabs])
    assert paths == {"vector", "scalar tail", "scalar unaligned", "idle chunks", "full last block", "several blocks", "last block unroll > 0", "empty job"}
    assert {t["njobs"] for t in tabs} >= {1, 2, 3, 37} and max(t["probes"] for t in tabs) >= 6
    atabs = [tc.table_claims([(n, offs) for n, offs, _ in c.jobs]) for c in tc.ADAM_CASES]
    assert set().union(*[t["paths"] for t in atabs]) >= paths - {"empty job"}
    for which in range(4):          # the scalar path forced by each of p, g, m, v alone
        assert any(sum(1 for o in offs if o % 4) == 1 and offs[which] % 4 for c in tc.ADAM_CASES for _, offs, _ in c.jobs)
    assert {(c.t, c.wd) for c in tc.ADAM_CASES} == {(1, 0.0), (3, 0.0), (1, 0.01), (3, 0.01)}
    assert {g for c in tc.ADAM_CASES for _, _, g in c.jobs} == set(tc.GMAGS)

    gs = [tc.gs_claims(c) for c in tc.GS_CASES]
    need = [("plant_first", True), ("plant_tail", True), ("plant_last_tensor", True), ("cap", True), ("empty tensor", True)]
    for k, v in need:
        assert any(d.get(k) == v for d in gs), (k, v)
    assert any(d["cap"] and d["plant_trip"] >= 4 for d in gs) and any(d["cap"] and d["plant_tail"] for d in gs) and any(d["cap"] and d["plant_first"] for d in gs)
    assert any(d["cap"] and d["plant_last_tensor"] for d in gs)
    assert any("unaligned p" in d["paths"] for d in gs) and any("unaligned q" in d["paths"] for d in gs)
    assert any(d["plant_loop"] == "scalar" and d["plant_trip"] >= 1 and not d["plant_tail"] for d in gs)
    assert {d["ntensors"] for d in gs} >= {1, 3, 24} and {d["blocks"] for d in gs} >= {1, 4, 512}
    assert {c.value for c in tc.GS_CASES} >= {"big", "negative", "1e-38", "3e38", "inf", "nan", "zero"}

    sg = [tc.sig_claims(c) for c in tc.SIG_CASES]
    assert any(d["wraps"] for d in sg) and any(d["blocks"] == 1 and d["ragged"] for d in sg) and any(d["specials"] for d in sg)
    assert tc.SIG_CAP * tc.SIG_THREADS + 1 in [c.n for c in tc.SIG_CASES]          # the smallest size with a second trip

    rd = [tc.red_claims(c) for c in tc.RED_CASES]
    for k, v in (("route", "ch64"), ("route", "ch16"), ("G", 2), ("G", 7), ("G", 16), ("G", 4), ("nt", 1008), ("nt", 800), ("nt", 32), ("taps", 49), ("taps", 25),
                 ("empty last group", True), ("S%G", True), ("part chunk", True), ("part chunk", False), ("unroll8", True), ("tail", True), ("bias_C%nw", True),
                 ("e strides", True), ("outputs", 1), ("outputs", 2), ("outputs", 3), ("outputs", 4)):
        assert any(d[k] == v for d in rd), (k, v)
    assert any(d["route"] == "ch16" and d["G"] == 1 and d["taps"] == 9 for d in rd) and any(d["route"] == "ch64" and d["taps"] == 1 for d in rd)
    assert {c.S for c in tc.RED_CASES} >= {1, 7, 8, 9, 16, 17, 56, 57}
    lay = tc.batch_layout(tc.defer_jobs())
    assert len(tc.defer_jobs()) >= 30 and sum(1 for ch, _, _ in lay if ch == 16) >= 2 and sum(1 for ch, _, _ in lay if ch == 64) >= 1
    jobs = tc.defer_jobs()
    assert any(nt == 1024 and any(tc.reduce_shape(sum(jobs[i][0].counts), jobs[i][0].cin, jobs[i][0].taps, jobs[i][0].S, jobs[i][0].bias_C)["nt"] == 256 for i, _ in l)
               for _, nt, l in lay), "a 1008-thread job next to a 256-thread job in one batch"

    dt = [tc.det_claims(c) for c in tc.DET_CASES]
    for k in ("single_block", "ragged", "image_boundary_in_block", "second_trip", "cap1024", "scratch_limited", "final_strides", "den_override", "grad_out", "zero_gt"):
        assert any(d[k] for d in dt), k
        assert any(not d[k] for d in dt), k
    assert any(d["second_trip"] and d["scratch_limited"] and d["total"] < 2000 for d in dt) and any(d["cap1024"] and d["second_trip"] for d in dt)
    assert all(d["bwd_trips"] == 1 for d in dt) and tc.DET_UNRUN          # the backward's second trip is left out, with its size

    sl = [tc.seg_claims(c) for c in tc.SEG_CASES]
    assert set().union(*[d["npix"] for d in sl]) == set(tc.SEG_NPIX) and set().union(*[d["npairs"] for d in sl]) == {1, 3}
    assert any(d["final_strides"] for d in sl) and any(d["npatches"] == 3 for d in sl) and all(d["unaligned prob_off"] for d in sl)

    bs = [tc.bias_claims(c) for c in tc.BIAS_CASES]
    for k, v in (("route", "vector"), ("route", "scalar"), ("nslabs", 2), ("unrolled", True), ("remainder", True), ("scratch_limited", True), ("idle_threads", True),
                 ("final_strides", True), ("one_block", True), ("P", 2), ("fmt", "half"), ("fmt", "bf16"), ("accumulate", True), ("misaligned", True)):
        assert any(d[k] == v for d in bs), (k, v)
    assert any(d["route"] == "scalar" and d["nslabs"] == 2 for d in bs) and any(d["route"] == "scalar" and d["scratch_limited"] for d in bs)
    assert any(d["route"] == "vector" and d["unrolled"] and not d["remainder"] for d in bs)

    gp = [tc.gp_claims(c) for c in tc.GP_CASES + tc.GP3_CASES]
    for kern in ("tr", "pack3"):
        for k in ("vector_reads", "tile_spans_images", "short_last_tile", "wraps", "padding"):
            assert any(d["kernel"] == kern and d[k] for d in gp), (kern, k)
        assert any(d["kernel"] == kern and d["wraps"] and d["vector_reads"] for d in gp) and any(d["kernel"] == kern and d["wraps"] and not d["vector_reads"] for d in gp)
    assert any(d["kernel"] == "tr" and d["one_quad_last_tile"] for d in gp)
    assert any(d["kernel"] == "pixel" for d in gp) and not any(d["kernel"] == "pixel" and d["wraps"] for d in gp) and tc.GP_UNRUN
    assert {(d["fmt"], d["P"]) for d in gp} == {("bf16", 1), ("bf16", 2), ("half", 1), ("half", 2)}
    assert {(d["prob"], d["scale"]) for d in gp if d["kernel"] != "pack3"} == {(True, True), (True, False), (False, True), (False, False)}
    assert {sum(c.pads) for c in tc.GP3_CASES} == {24, 64}

    pj = tc.pack_jobs()
    assert len(pj) >= 40 and {j[0] for j in pj} == {"fwd", "tr", "rows", "narrow"} and {(j[4], j[5]) for j in pj} >= {(1, 1), (2, 2), (3, 3), (2, 1)}
    assert {j[3] for j in pj} == {1, 3, 7} and any(j[0] == "fwd" and j[2] % 64 for j in pj) and any(j[0] == "tr" and j[1] % 64 for j in pj)
    assert any(j[6] for j in pj) and any(j[7] for j in pj) and {j[8] for j in pj if j[0] == "narrow"} == {8, 16}


def test_restated_geometry_at_the_sizes_the_issue_names():
    assert tc.job_layout([4097, 0, 1, 4096]) == ([0, 2, 2, 3], 4)
    assert [tc.job_search([0, 2, 2, 3], b)[0] for b in range(4)] == [0, 0, 2, 3]
    assert tc.gs_blocks(1) == 1 and tc.gs_blocks(16385) == 2 and tc.gs_blocks(8_500_004) == 512 and tc.gs_blocks(8_388_608) == 512
    assert tc.gs_reader(8_400_003, True, 512, 8_400_002) == ("scalar", 0) and tc.gs_reader(8_400_003, True, 512, 4 * 512 * 1024) == ("vector", 1)
    r = lambda *a: tc.reduce_shape(*a)
    assert (r(2048, 24, 1, 8)["ch"], r(2048, 24, 1, 8)["G"]) == (64, 4) and r(2047, 24, 1, 8)["ch"] == 16
    assert [r(16, 24, 9, S)["nt"] for S in (15, 16, 17, 56, 57, 64)] == [256, 288, 288, 1008, 1008, 1008]
    assert r(16, 24, 25, 16)["nt"] == 800 and r(16, 24, 49, 40)["nt"] == 256 and r(16, 24, 9, 57)["ranges"][-1] == (54, 57)
    assert [r(16, 24, 1, S)["nt"] for S in (15, 16, 23, 24, 31, 32)] == [256, 32, 32, 48, 48, 64]          # 32 and 48: no whole wave (REFUSED with a bias)
    assert all(r(sum(d["counts"]), d["cin"], d["taps"], d["S"])["nw"] == 0 for d in tc.REFUSED)
    assert r(16, 24, 9, 57, 16)["gx"] == 16 + 2 and r(16, 24, 9, 57)["nw"] == 15
    g = tc.det_geometry
    assert g(1, 11, 13)["nb"] == 1 and g(2, 17, 19)["nb"] == 3 and g(1, 31, 33, 10) == {"total": 1023, "nb": 2, "trips": 2, "bwd_blocks": 4, "bwd_trips": 1}
    assert g(1, 129, 131)["nb"] == 67 and g(1, 513, 513)["nb"] == 1024 and g(1, 513, 513)["trips"] == 2 and g(1, 512, 512)["trips"] == 1
    b = tc.bias_geometry
    assert b(5000, 24, 48)["slabs"][0]["nrl"] == 85 and b(5000, 24, 48)["slabs"][0]["nb"] == 15 and b(5000, 24, 48, scratch_floats=72)["slabs"][0]["nb"] == 3
    assert [s["Cs"] for s in b(5, 2056, 2080)["slabs"]] == [2048, 8] and [s["Cs"] for s in b(5, 1027, 1040)["slabs"]] == [1024, 3]
    assert b(700, 24, 48, aligned=False)["route"] == "scalar" and b(700, 24, 47)["route"] == "scalar"
    assert tc.pack_grid("fwd", 70, 100) == (70, 2) and tc.pack_grid("tr", 70, 100) == (2, 100) and tc.pack_grid("narrow", 5, 70) == (1, 70)


# ---- job tables -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tc.SCALE_CASES, ids=ids(tc.SCALE_CASES))
def test_scale_tensors_reference_and_mutants(case):
    xs = tc.scale_operands(case)
    want, flag = tc.scale_reference(case, xs)
    assert flag == int(case.plant is not None and case.plant[2] != "edge")
    for x, w in zip(xs, want):
        fin = torch.isfinite(w)
        assert bool(((w[fin] == 0) | (w[fin].abs() >= tc.TINY)).all())          # results normal or zero: no flush-to-zero ambiguity
        for kind, lo, hi, vals in tc.chunk_mutants(w, x, case.seed):
            assert not tc.same_bits(w[lo:hi], vals), (case, kind, lo)
        if x.numel() % 4:          # the scalar tail skipped: the last, partial chunk keeps its input
            lo = x.numel() // 4 * 4
            if tc.same_bits(w[lo:], x[lo:]):          # (an inf stays an inf: then the FLAG is what shows the skipped tail, raised by nothing else)
                rest = [t if t is not w else t[:lo] for t in want]
                assert flag == 1 and all(bool((t.abs() <= 3.4e38).all()) for t in rest), (case, "tail")
    # a job run with its neighbour's size leaves elements unscaled (or runs past its end): the sizes of some neighbours differ
    ns = [n for n, _, _ in case.jobs]
    if len(ns) > 1:
        assert any(a != b for a, b in zip(ns, ns[1:]))
        j, k = max(((i, ns[o]) for i in range(len(ns)) for o in (i - 1, i + 1) if 0 <= o < len(ns)), key=lambda t: ns[t[0]] - t[1])
        assert ns[j] - k >= 4 and not tc.same_bits(want[j][k:], xs[j][k:])


@pytest.mark.parametrize("case", tc.ADAM_CASES, ids=ids(tc.ADAM_CASES))
def test_adam_float32_within_bound_and_mutants_outside(case):
    r = tc.AdamReference(case)
    for j, ((p, g, m, v), (n, offs, gmag)) in enumerate(zip(r.ops, case.jobs)):
        y = r.yardstick(j)
        for k, val in y.items():
            assert note("adam " + k, val) <= 1.0, (case, j, k, val)
        p32 = r.jobs[j]["p32"]
        fixed_point = gmag == 0.0 and case.t == 1 and case.wd == 0.0
        if fixed_point:          # g = 0 on zero moments: nothing may move, and no chunk mutant exists (every value is its own update)
            assert torch.equal(p32, p) and not bool(r.jobs[j]["m"][0].any()) and not bool(r.jobs[j]["v"][0].any())
            continue
        m32, v32 = r.jobs[j]["m"][1], r.jobs[j]["v"][1]
        before = {"update": p, "m": m, "v": v}
        after = {"update": p32, "m": m32, "v": v32}
        for name in ("update", "m", "v"):
            if name == "v" and gmag == 0.0 and case.wd == 0.0:
                continue          # v' = beta2 v: a stale chunk differs by 0.1 % only where v != 0 -- checked through m and the update
            muts = tc.chunk_mutants(after[name], before[name], case.seed + j)
            if n % 4:          # the scalar tail skipped: the last, partial chunk keeps what it held
                muts.append(("tail unwritten", n // 4 * 4, n, before[name][n // 4 * 4:].clone()))
            for kind, lo, hi, vals in muts:
                got = {k2: after[k2].clone() for k2 in after}
                got[name][lo:hi] = vals
                rr = r.job_ratio(j, got["update"], got["m"], got["v"], names=(name,))
                assert rr[name] > 1.0, (case, j, name, kind, rr)
    # a 0.2 % error of every update -- what the old tolerance hid -- is far outside
    j = next(i for i, (_, _, gm) in enumerate(case.jobs) if not (gm == 0.0 and case.t == 1 and case.wd == 0.0))
    p = r.ops[j][0]
    worse = (p.double() + 1.002 * (r.jobs[j]["p32"].double() - p.double())).float()
    assert r.job_ratio(j, worse, r.jobs[j]["m"][1], r.jobs[j]["v"][1])["update"] > 10.0


# ---- grad_scale -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tc.GS_CASES, ids=ids(tc.GS_CASES))
def test_grad_scale_binade_condition_and_missed_maximum(case):
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    o = tc.gs_operands(case)
    m32, m64 = tc.gs_max(o, torch.float32), tc.gs_max(o, torch.float64)
    S = tc.gs_scale(m32)
    if case.value in ("inf", "nan", "zero"):
        assert S == 1.0
        return
    assert np.frexp(m32)[1] == np.frexp(m64)[1], "float32 and float64 must agree on the binade of the maximum"
    assert S == tc.gs_scale(m64)
    if case.value == "1e-38":
        assert S == 2.0 ** 100 and 0 < m32 < tc.TINY
    elif case.value == "3e38":
        assert S == 2.0 ** -100
    else:
        assert 2.0 ** (tc.GS_TARGET - 1) <= m32 * S < 2.0 ** tc.GS_TARGET
    # the mutant: the planted element is missed
    assert tc.gs_scale(tc.gs_max(o, torch.float32, skip=case.plant)) != S


# ---- sigmoid ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tc.SIG_CASES, ids=ids(tc.SIG_CASES))
def test_sigmoid_float32_within_bound_and_mutants_outside(case):
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    r = tc.SigReference(case)
    assert note("sigmoid", r.ratio(r.f32)) <= 1.0
    muts = tc.chunk_mutants(r.f32, r.x, case.seed)
    assert muts and (len(muts) == 2 or case.n < 8)
    for kind, lo, hi, vals in muts:
        assert r.ratio(vals, lo, hi) > 1.0, (case, kind, lo)
    if case.n >= len(tc.SIG_SPECIALS):          # the special values: a stale logit is seen at each of them but x = 0.5's fixed point (none planted)
        k = case.n - len(tc.SIG_SPECIALS)
        for i in range(k, case.n):
            assert r.ratio(r.x[i:i + 1], i, i + 1) > 1.0, (case, float(r.x[i]))


# ---- split weight-gradient reductions ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tc.RED_CASES, ids=ids(tc.RED_CASES))
def test_reduction_float32_within_bound_and_mutants_outside(case):
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    r = tc.RedReference(case)
    for acc in (0, 1):
        for name, (r64, r32, b) in r.expect(acc).items():
            assert note("wgrad_reduce " + name, tc.ratio(r32.double() - r64, b)) <= 1.0, (case, acc, name)
    w64, w32, wb = r.expect(0)["w"]
    muts = r.mutants()
    assert any(k.startswith("split") for k in muts)
    for kind, val in muts.items():
        if kind == "reverse order":          # only the bit comparison with the in-order float32 evaluation sees a changed ORDER
            assert not torch.equal(val, w32), (case, kind)
        else:
            assert tc.ratio(val.double() - w64, wb) > 1.0, (case, kind)
    if r.shape["G"] >= 3 and case.S >= 3 * r.shape["Sg"]:
        assert "reverse order" in muts and "range overlap" in muts
    if case.bias_C:
        b64, b32, bb = r.expect(0)["b"]
        assert tc.ratio((b64 - r.bpart[case.S - 1].double()) - b64, bb) > 1.0


def test_deferred_batches_restated():
    jobs = tc.defer_jobs()
    lay = tc.batch_layout(jobs)
    seen = sorted(i for _, _, l in lay for i, _ in l)
    assert seen == list(range(len(jobs))) and all(len(l) <= tc.REDUCE_BATCH for _, _, l in lay)
    for ch, nt, l in lay:
        assert nt % 64 == 0 and nt <= 1024 and l[0][1] == 0
        for (i, b0), (i2, b1) in zip(l, l[1:]):
            c = jobs[i][0]
            assert b1 - b0 == tc.red_claims(c)["blocks"]


# ---- detection loss -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tc.DET_CASES, ids=ids(tc.DET_CASES))
def test_detection_loss_float32_within_bound_and_mutants_outside(case):
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    r = tc.DetReference(case)
    print(f"[log term] {case.name}: MARGIN x worst CPU float32 log / log1p error = {r.log_ulps:.2f} ulps")
    assert 0 < r.log_ulps <= 8.0
    assert note("det_loss out8", r.out8_ratio(r.yardstick8())) <= 1.0
    cl = tc.det_claims(case)
    for kind, out8 in r.mutants8().items():
        # compared on the four loss words (the denominators do not change when a pixel with an overridden / zero mask is dropped)
        d = tc.ratio((out8 - r.out8)[:4], r.b8[:4])
        assert d > 1.0, (case, kind, d)
    assert ("second trip skipped" in r.mutants8()) == cl["second_trip"]
    if case.get("gt") == "zero":
        assert float(r.s[2]) == 0.0 and float(r.s[4]) == 0.0 and float(r.out8[5]) == 1.0 / tc.EPS_DEN and float(r.out8[2]) == 0.0
    if case.get("gt") == "binary":
        assert r.exact_m2 and float(r.b8[7]) == 0.0
    if cl["total"] > 100_000:
        return          # (the gradient maps of the capped case: checked on the device only; the float32 evaluation of 14 M elements adds nothing here)
    ref, f32 = r.grads(torch.float64), r.grads(torch.float32)
    bnd = r.grad_bounds(ref)
    for k in ref:
        assert note("det_loss " + k, tc.ratio(f32[k].double() - ref[k], bnd[k])) <= 1.0, (case, k)
        # zero references (sign 0, p == t, mask 0) and live ones
        assert bool((ref[k] == 0).any()) and (bool((ref[k] != 0).any()) or (case.get("gt") == "zero" and k != "g_kp")), (case, k)
        # mutant: one 16-byte chunk holds its neighbour's values
        flat, fb = ref[k].reshape(-1), bnd[k].reshape(-1)
        hit = 0
        for lo in range(0, min(flat.numel() - 8, 4000), 4):
            if not torch.equal(flat[lo:lo + 4], flat[lo + 4:lo + 8]):
                assert tc.ratio(flat[lo + 4:lo + 8] - flat[lo:lo + 4], fb[lo:lo + 4]) > 1.0
                hit += 1
        assert hit or case.get("gt") == "zero"
    assert float(ref["g_kp"].abs().max()) >= 1e6 * float(ref["g_kp"].abs()[ref["g_kp"] != 0].min())          # the dynamic range the product bound is for


# ---- seg loss -------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tc.SEG_CASES, ids=ids(tc.SEG_CASES))
def test_seg_loss_float32_within_bound_and_mutants_outside(case):
    r = tc.SegReference(case)
    assert note("seg_loss loss", tc.ratio((r.loss32.double() - r.loss).reshape(1), r.bloss.reshape(1))) <= 1.0
    assert note("seg_loss gprob", tc.ratio(r.g32.double() - r.g, r.bg)) <= 1.0
    assert not bool(r.written.all()) and bool((r.bg[~r.written] == 0).all())          # the gaps between the patches keep their fill
    big = int(r.terms.abs().argmax())
    assert tc.ratio((r.terms[big]).reshape(1), r.bloss.reshape(1)) > 1.0          # the clamped pixel (p = 0 with t = 1: a term of 100 w) dropped
    small = r.terms.abs().sort().values
    assert float(small[-1]) > 50 * float(small[len(small) // 2])
    for off, npix, p0, np_ in r.o["patches"]:          # a gprob chunk that stays at the fill (0, as seg_loss.py allocates it) or holds its neighbour's values
        if npix >= 8:
            lo = off + 4
            assert tc.ratio(r.g[lo:lo + 4], r.bg[lo:lo + 4]) > 1.0
            assert tc.ratio(r.g[lo + 4:lo + 8] - r.g[lo:lo + 4], r.bg[lo:lo + 4]) > 1.0


# ---- bias_grad --------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tc.BIAS_CASES, ids=ids(tc.BIAS_CASES))
def test_bias_grad_float32_within_bound_and_dropped_row_outside(case):
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    r = tc.BiasReference(case)
    assert note("bias_grad", tc.ratio(r.f32.double() - r.ref, r.bound)) <= 1.0
    for row in tc.bias_rows(case):
        assert tc.ratio(r.dropped(row) - r.ref, r.bound) > 1.0, (case, row)


# ---- grad_pack --------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tc.GP_CASES, ids=ids(tc.GP_CASES))
def test_grad_pack_float32_within_bound_and_mutants_outside(case):
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    grad, prob = tc.gp_operands(case)
    r = tc.GradPackReference(case, grad, prob if case.prob else None)
    assert note(f"grad_pack {case.fmt} P{case.P}", r.ratio(r.f32)) <= 1.0
    R = r.ref.shape[0]
    rows = sorted({0, R - 1, min(R - 1, 256), R // 2})
    for row in rows:          # one 16-byte chunk (8 channels; here the first min(C, 8)) left at the fill / taken from the next pixel / the tile's first pixel again
        w = min(case.C, 8)
        fill = torch.full((1, w), tc.FILL, dtype=torch.float64)
        assert tc.ratio(fill - r.ref[row:row + 1, :w], r.bound[row:row + 1, :w]) > 1.0, (case, row)
        other = row + 1 if row + 1 < R else row - 1
        assert tc.ratio(r.ref[other:other + 1, :w] - r.ref[row:row + 1, :w], r.bound[row:row + 1, :w]) > 1.0, (case, row)
    cl = tc.gp_claims(case)
    if cl["wraps"]:          # `i0` not advanced: the second trip writes the first tile's pixels again, its own stay at the fill
        first = tc.GP_TR_CAP * tc.GP_THREADS
        assert first < R and tc.ratio(torch.full_like(r.ref[first:first + 1], tc.FILL) - r.ref[first:first + 1], r.bound[first:first + 1]) > 1.0


# ---- layouts against the product's host code --------------------------------------------------------------------------------------------------------------

def test_job_tables_equal_what_the_product_builds(monkeypatch):
    from kg_instance_segmentation_amd import ops
    calls = []
    monkeypatch.setattr(ops, "h2d", lambda arr, dev: torch.from_numpy(np.ascontiguousarray(arr).copy()))
    monkeypatch.setattr(ops._lib, "call", lambda name, *a, **kw: calls.append((name, a, kw)))
    monkeypatch.setattr(ops, "stream_ptr", lambda: None)
    monkeypatch.setattr(ops, "ptr", lambda t: t)
    # ops.scale_tensors
    case = next(c for c in tc.SCALE_CASES if len(c.jobs) == 37)
    ts = [torch.zeros(n) for n, _, _ in case.jobs]
    one = torch.ones(1)
    ops.scale_tensors(ts, one)
    name, a, _ = calls.pop()
    live = [n for n, _, _ in case.jobs if n > 0]          # (the wrapper drops empty tensors; the C ABI accepts them, as the table computes)
    blk0, total = tc.job_layout(live)
    dt = np.dtype([("p", "<u8"), ("n", "<i8"), ("scale", "<u8"), ("blk0", "<i4"), ("pad", "<i4")])
    tab = a[0].numpy().view(dt)
    assert name == "kg_scale_tensors" and a[1] == len(live) and a[2] == total
    assert tab["n"].tolist() == live and tab["blk0"].tolist() == blk0
    # PackQueue.flush
    jobs = tc.pack_jobs()
    q = ops.PackQueue(0)

    class PW:
        pass
    for kind, cout, cin, k, xP, wP, row0, c0, extra in jobs:
        w = torch.zeros(cout, cin, k, k)
        pw = PW()
        pw.buf, pw.K, pw.cin_pad, pw.xP, pw.wP = torch.zeros(1), 64, 64, xP, wP
        q.add(w, pw, row0, c0, kind in ("tr", "narrow"), None)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: __import__("contextlib").nullcontext())
    q.flush()
    name, a, _ = calls.pop()
    lay, total = tc.pack_layout(jobs)
    pdt = np.dtype([("w", "<u8"), ("dst", "<u8"), ("rowmap", "<u8")] + [(n, "<i4") for n in
                   ("Cout", "Cin", "taps", "K", "cin_pad", "row0", "c0", "transposed", "gx", "blk0", "xP", "wP", "tap_stride", "tap_pitch")])
    tab = a[0].numpy().view(pdt)
    assert name == "kg_pack_weight_batch" and a[1] == len(jobs) and a[2] == total
    assert list(zip(tab["blk0"].tolist(), tab["gx"].tolist())) == lay


def test_worst_float32_ratio_per_kernel():
    """(report) worst |float32 CPU evaluation - float64| / bound per kernel and output over the cases run in this process"""
    for k, v in sorted(WORST.items()):
        print(f"[float32 yardstick / bound] {k}: {v:.3f}")
    assert all(v <= 1.0 for v in WORST.values())
