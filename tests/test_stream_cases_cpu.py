"""Do the parity cases of the streaming kernels (csrc/norm_pool.hip) run every index path, and do their bounds bite?  (no GPU needed)

oracle/streamcases.py restates the launch geometry of every entry point of norm_pool.hip on the host, lists the cases and builds their float64
references, bounds and mutants; tests/test_gpu_stream.py runs the cases on the device.  Here the TABLE and the BOUNDS are asserted, before any
kernel runs:
  * every index path the cases are there for -- the 32-bit-division branch of kg_divmod, a second partly filled trip of every grid-stride loop
    that a < 64 M-element tensor can reach, > 64 partials per channel, rows_per_block no multiple of 32 / 64, the one-row tail of the frozen
    kernel's two-row loop, a scratch-limited reduce_geometry, the 512-block cap, host-built partials, the generic bilinear kernel at non-2x
    ratios / when down-sampling / at IH = 1 / at IW = 1, the 2x kernel with and without a strip tail, the mask of bilinear_bwd, the carry of
    rows_absmax_kernel with a C8 that does not divide the stride in a second sweep -- is claimed by at least one case, the claim COMPUTED from
    the restated geometry (streamcases.REQUIRED, streamcases.claims);
  * the float32 CPU evaluation of every case, rounded to the output's planes, sits within the case's own bound on every element, and the
    float32 evaluation of every reduced quantity within its bound;
  * every mutant of every case fails its bound: one 16-byte chunk taken from the neighbouring row, one chunk left at the fill value, one row
    (one block partial) dropped from a reduction, the planted maximum of a rescale case removed.  A mutant touches one chunk, so it is checked
    on that chunk; the float32 evaluation is checked on every element."""
import collections

import pytest
import torch

from oracle import streamcases as sc

WORST = collections.defaultdict(float)
REFS = {}


def reference(c):
    return sc.Reference(c)


def test_every_listed_index_path_is_claimed_by_a_case():
    assert not sc.required_missing(), sc.required_missing()
    # deleting the cases of a path is seen: without the large rescale shapes the second sweep is gone
    small = [c for c in sc.CASES if not (c.entry == "rescale" and c.M > 10000)]
    assert ("rescale", "plant_sweep", 1) in sc.required_missing(small)
    assert ("bn_frozen", "two_row_tail", True) in sc.required_missing([c for c in sc.CASES if c.entry != "bn_frozen"])
    # the wraps cases sit just above the cap: the smallest shape at which the second trip exists
    assert sc.WRAP_M * 8 > sc.EW_CAP * sc.EW_THREADS >= (sc.WRAP_M - 13) * 8
    assert not any(sc.claims(c).get("div64") for c in sc.CASES)          # (the 64-bit branch stays unrun: streamcases.UNRUN)


def test_restated_geometry_at_the_sizes_the_issue_names():
    g = lambda M, C: sc.reduce_geometry(M, C, 2 * C * 512)
    assert g(1, 8) == (1, 1) and g(33, 8) == (1, 33) and g(257, 8) == (2, 129) and g(8225, 8) == (33, 250) and g(16641, 8) == (66, 253)
    assert g(131100, 8) == (511, 257)          # (n is capped at 512; 257 rows per block then need 511 blocks)
    assert sc.reduce_geometry(8225, 72, 2 * 72 * 3) == (3, 2742) and sc.reduce_geometry(10, 8, 15) is None
    assert sc.frozen_tail(8225, 33, 250) and not sc.frozen_tail(1, 1, 1) and not sc.frozen_tail(64, 1, 64)
    assert sc.bilinear_route(9, 5, 18, 10) == "2x" and sc.bilinear_route(1, 6, 2, 12) == "generic" and sc.bilinear_route(6, 1, 12, 2) == "generic"
    a = sc.absmax_geometry(131100, 8)
    assert (a["blocks"], a["stride"], a["dr"], a["dc"], a["sweeps"]) == (256, 262144, 32768, 0, 2)
    a = sc.absmax_geometry(5000, 3)
    assert (a["blocks"], a["stride"], a["dr"], a["dc"], a["sweeps"]) == (4, 4096, 1365, 1, 1)


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_float32_evaluation_within_bound_and_every_mutant_outside(case):
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    r = reference(case)
    e = case.entry
    for name, out in r.rows.items():
        y = out.ratio(out.f32)
        WORST[e + " " + name] = max(WORST[e + " " + name], y)
        assert y <= 1.0, (case, name, y)
        muts = r.row_mutants(name)
        kinds = {m[0] for m in muts}
        assert "fill" in kinds and ("neighbour" in kinds or out.ref.shape[0] == 1 or not bool(out.ref.any())), (case, name, kinds)
        for m in muts:
            assert r.row_mutant_ratio(name, m) > 1.0, (case, name, m[:3])
    if r.vecs:
        y = r.vec_ratio({k: v.f32 for k, v in r.vecs.items()})
        WORST[e + " sums"] = max(WORST[e + " sums"], y)
        assert y <= 1.0, (case, {k: v.ratio(v.f32) for k, v in r.vecs.items()})
        assert r.vec_ratio({k: v.ref for k, v in r.vecs.items()}) == 0.0
        drops = r.drop_mutants()
        assert drops
        for row, vals in drops.items():
            assert r.vec_ratio(vals) > 1.0, (case, "dropping row", row, "stays within the bound")
    if e == "rescale":
        if case.value in ("big", "pow2"):
            assert r.scalars["r"] < 1.0 and r.r_without_plant != r.scalars["r"], (case, r.scalars, r.r_without_plant)
        else:
            assert r.scalars["r"] == 1.0
        if case.plant == "lofavour":
            assert r.r_of_plane0 == r.scalars["r"] / 2
    if e in ("rescale", "rows_scale", "scale_multi"):
        # exact operations: the expected buffer differs from the input buffer in every in-slice chunk unless the factor is 1
        s = r.scalars["r"] if e == "rescale" else r.s
        pairs = zip(r.buffers, [sc.layout(v, case.fmt, it[2], it[3])[0] for v, it in zip(r.o.gs, case.items)]) if e == "scale_multi" else \
            [(r.buffer, sc.layout(r.o.g, case.fmt, case.P)[0])]
        for want, before in pairs:
            same = torch.equal(want.view(torch.int16), before.view(torch.int16))
            assert same == (s == 1.0), (case, s)


def test_worst_float32_ratio_per_kernel():
    """(report) worst |float32 CPU evaluation - float64| / bound per kernel and output over the cases run in this process"""
    for k, v in sorted(WORST.items()):
        print(f"[float32 yardstick / bound] {k}: {v:.3f}")
    assert all(v <= 1.0 for v in WORST.values())


def test_conditioning_case_is_measured_not_bounded():
    """the 30-sigma case: torch's float32 batch_norm against float64 and the float32 one-pass evaluation against float64 are both finite numbers
    the GPU test prints and compares with; the one-pass formula loses ~900 x more than the two-pass one, which is what the case is for"""
    c = sc.CONDITIONING
    o = sc.Operands(c)
    x64 = o.x.double()
    mu, var = x64.mean(0), x64.var(0, unbiased=False)
    assert float((mu.abs() / var.sqrt()).min()) > 25
    nb, rpb = sc.reduce_geometry(c.M, c.C, sc.default_scratch(c.C, False))
    m1, i1 = sc.onepass_f32(o.x, nb, rpb)
    is64 = 1.0 / (var + sc.EPS32).sqrt()
    e_one = float(((i1 - is64).abs() / is64).max())
    x32 = o.x.t().reshape(1, c.C, c.M, 1)
    rm, rv = torch.zeros(c.C), torch.ones(c.C)
    y32 = torch.nn.functional.batch_norm(x32, rm, rv, None, None, True, 1.0, sc.EPS32)
    y64 = (x64 - mu) * is64
    e_torch = float((y32[0, :, :, 0].t().double() - y64).abs().max())
    print(f"[conditioning] one-pass float32 (kernel decomposition) relative invstd error {e_one:.3g}; torch float32 batch_norm worst |y - float64| {e_torch:.3g}")
    assert 0 < e_one < 1e-2 and e_torch < 1e-3
