"""Dense convolutions against FLOAT64, one small case per launch class -- with the launched kernel observed.

Everything Engine launches through ops.conv_auto / conv_wgrad / conv1x1 / conv_halo_heads2 / conv7_narrow is dispatched twice, by ops.py and again
inside the library (launch_halo, kg_launch_conv_gather, kg_launch_conv_tiny, kg_conv1x1, kg_conv2d_wgrad, kg_conv2d_wgrad_halo, ...), where fill
thresholds pick kernel variants and a channel / K split that the kernel name does not show.  oracle/densecases.py restates both levels on the host
and lists the cases; tests/test_dense_routes_cpu.py asserts the table (every class of the bench census and every kernel name has a case, the bound
of every case sees one lost (tap, 8-channel group) slice).  Here, on the GPU:

CASES (test_case).  Each case goes through ops; `_lib.call` is wrapped, the one dense entry point the case reaches is turned into a class key from
its ARGUMENTS (densecases.key_of_call: planes, epilogue operands, the statistics side channel's state, the split as the launcher derives it) and the
kernel is read from kg_last_kernel.  Asserted: python-level kind == plan, kernel name == plan, key == plan -- a variant whose guard is false falls
through to another kernel and FAILS here by name.  Then every output element is compared with float64 within
    u_out * |ref| + dropped plane products + max(4 x worst |float32 CPU evaluation - float64|, 2e-6 x rms)        (densecases.Reference)
and every element outside the written channel slice equals the fill value.  Armed cases also compare the statistics partials the launch commits
(sum v, sum v^2; backward: sum g, sum g * xhat) with float64 sums (densecases.stats_reference).
Cases that need a library switch (KG_HALO3_NB2=2, KG_HALO7_W4=2, KG_GATHER_N64=1) run in one child process per switch, one at a time, with a
timeout; nothing more is started on the GPU by this file after a child that died on a signal, hung or reported a GPU fault.  Inside the child the same kernel-name assertion applies.

CENSUS (test_train_step_census).  One train step (forward, losses, backward) of the random-init network at 2 x 64 x 64 with seeded boxes per policy
("fp32", "fp32b2", "half", "bf16") under the same spy.  Asserted for every observed dense launch: the library launched the kernel the planner derives
from the call's arguments, and the launch's FULL key (entry point, kernel, kernel size, stride, mode, planes, products, format, split, epilogue) is
covered by a case (densecases.covers: equal fields; a case with more of the element-wise epilogue steps bias / residual / mask / ReLU covers a
launch with fewer of them, because those steps are one shared function, each behind its own null test; fp32 export, oscale, statistics and the
fused bias gradient have to match).  The classes the hand-written cases do not reproduce are recorded in densecases.CENSUS_64 and get one GENERATED
case each (densecases.search_case: the cheapest shape of a small grid whose plan is exactly the key); a launch that is neither fails with its key.

MEASURED on MI355X, 2026-10-18, on this file as committed (228 cases, 219 tests).  Worst |d| / bound over the cases of a kernel family: GPU, in
brackets the float32 CPU evaluation (the yardstick) against the same bound:
  families whose worst case has a single-plane rows output (the bound is dominated by u_out = half an ulp of the stored format, which correct
      rounding reaches): conv_halo_kernel 0.996 (0.247), conv_halo3_w4 0.996 (0.217), conv_halo7_w4 0.995 (0.232), conv3_c64 0.995 (0.079),
      conv_gather 0.996 (0.235), conv_tiny 0.995 (0.221), conv_small_mfma 0.995 (0.216), conv1x1_stream / conv1x1 0.995 (0.063),
      conv_igemm 0.976 (0.005), conv7_narrow 0.993 (0.069)
  two-plane rows outputs only: conv3_ws 0.199 (0.232)
  fp32 outputs: conv_wgrad_kernel 0.101 (0.244), conv_wgrad_ring 0.142 (0.245), wgrad_halo 0.189 (0.248); second-layer heads on one bf16 plane 0.661 (0.125)
  statistics sums, worst |d| / bound: first sum 0.034, second sum 0.021
  EXCEPTION, with its cause: with the library's float32 evaluation as the only yardstick `heads2 one plane` (K = 3136, one bf16 plane, fp32 export)
      measured 3.3e-6 = 1.26 x its bound (4 x 6.4e-7).  Cause, found on the CPU: 8-bit x 8-bit products are exact in fp32 and the CPU sums in wide
      blocks, so that yardstick is 5 ulp; the same sum through ONE fp32 accumulator in 98 steps of 32 channels gives 1.9e-6 with round-to-nearest and
      7.4e-6 with truncation.  For that family alone -- single-plane operands into an fp32 output -- densecases.chain_error (the sequential chain,
      round-to-nearest) is a second float32 evaluation; every other case uses the library evaluation alone.  MARGIN = 4 and FLOOR = 2e-6 are unchanged.
  wall time of this file 30 s: 219 tests, the four census train steps and the three switch children (4 .. 5 s each) included; the largest case
      (heads2 no split) 2.1 s, most of it the float64 reference on the CPU.
"""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from kg_instance_segmentation_amd import _lib, ops  # noqa: E402
from kg_instance_segmentation_amd.ops import PT  # noqa: E402
from oracle import densecases as dc  # noqa: E402

DEV = "cuda"
FILL = 9.0
SWITCHES = ("KG_HALO3_NB2", "KG_HALO7_W4", "KG_HALO7_NB2", "KG_GATHER_N64", "KG_HALO_SPLIT", "KG_GATHER_SPLIT", "KG_HEADS2_KPART")
_SET = {k: os.environ[k] for k in SWITCHES if k in os.environ}
ACTIVE = [c for c in dc.CASES if (c.env or {}) == _SET]          # the cases of THIS process's environment (a child: the cases of its switch)
SWITCH_ENVS = sorted({tuple(sorted(c.env.items())) for c in dc.CASES if c.env})


class Spy:
    """records every _lib.call of a dense entry point made while active: (entry point, key from the arguments, kernel name); follows the statistics
    side channel (armed by kg_conv_stats_begin / kg_conv_bstats_begin until kg_conv_stats_end) as the library does"""

    def __init__(self):
        self.calls, self.armed = [], None

    def __enter__(self):
        self.orig = _lib.call

        def call(name, *args, fmt=0):
            self.orig(name, *args, fmt=fmt)
            if name == "kg_conv_stats_begin":
                self.armed = "fwd"
            elif name == "kg_conv_bstats_begin":
                self.armed = "bwd"
            elif name == "kg_conv_stats_end":
                self.armed = None
            elif name in dc.DENSE_ENTRIES:
                key = dc.key_of_call(name, args, fmt, self.armed)
                self.calls.append((name, key, _lib.last_kernel(fmt)))
        _lib.call = call
        return self

    def __exit__(self, *exc):
        _lib.call = self.orig


# ---- device operands ---------------------------------------------------------------------------------------------------------------------

def rows(t):
    n, c, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(n * h * w, c).contiguous()


def nchw(r, n, h, w):
    return r.view(n, h, w, -1).permute(0, 3, 1, 2)


def to_pt(rows_f32, P, fmt, cpad=None, sliced=False, fill=0.0):
    """fp32 [rows, C] host tensor -> PT of P planes on the device (columns zero-padded to cpad); sliced: a column slice of a wider buffer whose
    other columns hold `fill`"""
    r, C = rows_f32.shape
    cpad = cpad or C
    ctot, c0 = (dc.round_up(cpad, 8) + 16, 8) if sliced else (dc.round_up(cpad, 8), 0)          # (plane strides are multiples of 8 elements)
    buf = torch.full((r, P * ctot), fill, dtype=torch.float32)
    for p, pl in enumerate(dc.split_planes(rows_f32, fmt, P)):
        buf[:, p * ctot + c0:p * ctot + c0 + cpad] = 0.0
        buf[:, p * ctot + c0:p * ctot + c0 + C] = pl
    buf = buf.to(dc.DT[fmt]).to(DEV)
    return PT(buf[:, c0:c0 + cpad], P, ctot), buf


def from_pt(pt):
    out = pt.plane(pt.P - 1).double()
    for p in range(pt.P - 2, -1, -1):
        out = out + pt.plane(p).double()
    return out.cpu()


def outside_is_fill(buf, P, cpad, sliced):
    if not sliced:
        return True
    ctot = dc.round_up(cpad, 8) + 16
    m = torch.ones(P * ctot, dtype=torch.bool)
    for p in range(P):
        m[p * ctot + 8:p * ctot + 8 + cpad] = False
    return bool((buf[:, m.to(buf.device)].float() == FILL).all())


def single(pt):
    return pt if pt.P > 1 else pt.t


def run_case(c, o):
    """launches the case through ops; returns (python-level kind, [outputs as float64 NCHW / OIHW host tensors], statistics [C, 2] or None, spy, untouched)"""
    P, fmt, dt = c.P, c.fmt, dc.DT[c.fmt]
    fi = 1 if fmt == "half" else 0
    stats, untouched = None, True
    dev = lambda t: None if t is None else t.to(DEV)
    with Spy() as spy:
        if c.op in ("fwd", "dgrad"):
            tr = c.op == "dgrad"
            src, kin, oc, (oh, ow) = (o.dy, c.cout, c.cin, (c.H, c.W)) if tr else (o.x, c.cin, c.cout, (c.OH, c.OW))
            kpad = dc.round_up(kin, 8)
            xp, _ = to_pt(rows(src), P, fmt, cpad=kpad, sliced=c.slices)
            pw = ops.PackedWeight(oc, c.k * c.k, kpad, DEV, xP=P, wP=P, dtype=dt)
            pw.pack(o.w.to(DEV), transposed=tr)
            M = c.N * oh * ow
            geom = (M, c.OH, c.OW, c.H, c.W, c.k, c.k, c.stride, c.pad) if tr else (M, c.H, c.W, c.OH, c.OW, c.k, c.k, c.stride, c.pad)
            mask = to_pt(rows(o.mask), 1, fmt)[0].t if c.mask else None
            yf = torch.full((c.N, oc, oh, ow), FILL, dtype=torch.float32, device=DEV) if c.f32 else None
            y = ybuf = None
            res = None
            if not c.f32:
                init = rows(o.res) if (c.res and tr) else torch.full((M, oc), FILL)      # (input gradients accumulate in place, as Engine does)
                y, ybuf = to_pt(init, P, fmt, sliced=c.slices, fill=FILL)
                res = y if (c.res and tr) else (to_pt(rows(o.res), P, fmt)[0] if c.res else None)
            part = None
            if c.armed == "fwd":
                part = ops.conv_stats_begin(torch.device(DEV), fi)
            elif c.armed == "bwd":
                part = ops.conv_bstats_begin(to_pt(rows(o.bnx), P, fmt)[0], dev(o.bn_mean), dev(o.bn_invstd), M, oc, c.N)
            nb = 0
            try:
                kind = ops.conv_auto(single(xp), pw, oc, geom, c.N, y=None if y is None else single(y), y_f32=yf, bias=dev(o.bias),
                                     res=None if res is None else single(res), mask=mask, relu=c.relu, transposed=tr, oscale=dev(o.oscale), tiny=c.tiny)
            finally:
                if c.armed:
                    nb = ops.conv_stats_end(fi)
            torch.cuda.synchronize()
            if c.armed:
                assert nb > 0, (c, "the armed launch wrote no statistics partials")
                stats = part[:nb * oc * 2].view(nb, oc, 2).double().sum(0).cpu()
            out = yf.double().cpu() if c.f32 else nchw(from_pt(y), c.N, oh, ow)
            if y is not None:
                untouched = outside_is_fill(ybuf, P, oc, c.slices)
            return kind, [out], stats, spy, untouched
        if c.op == "wgrad":
            xp, _ = to_pt(rows(o.x), P, fmt, cpad=dc.round_up(c.cin, 8))
            gp, _ = to_pt(rows(o.dy), P, fmt, cpad=dc.round_up(c.cout, 8))
            gw = torch.full((c.cout, c.cin, c.k, c.k), float("nan"), dtype=torch.float32, device=DEV)
            db = torch.full((c.cout,), float("nan"), dtype=torch.float32, device=DEV) if c.bias_out else None
            kind = ops.conv_wgrad(single(xp), single(gp), c.cin, c.cout, (c.N * c.OH * c.OW, c.H, c.W, c.OH, c.OW, c.k, c.k, c.stride, c.pad), [(gw, 0, c.cout)],
                                  N=c.N, bias_out=db)
            torch.cuda.synchronize()
            return kind, [gw.double().cpu()] + ([db.double().cpu()] if c.bias_out else []), None, spy, True
        if c.op == "heads2":
            C = c.cin
            layout, vmap = ops.heads2_layout()
            pw = ops.PackedWeight(64, 49, C, DEV, groups=3, xP=P, wP=P, dtype=dt)
            bias64 = torch.zeros(64, device=DEV)
            outs = []
            for h, co in enumerate((5, 10, 40)):
                rm = torch.tensor(layout[h], dtype=torch.int32, device=DEV)
                pw.pack_rows(o.ws[h].to(DEV), rm, group=h)
                bias64[rm.long()] = o.bs[h].to(DEV)
                outs.append(torch.full((c.N, co, c.H, c.W), float("nan"), dtype=torch.float32, device=DEV))
            xp, _ = to_pt(rows(o.x), P, fmt)
            ops.conv_halo_heads2(single(xp), pw, bias64, torch.tensor(vmap, dtype=torch.int32, device=DEV), outs[0], outs[1], outs[2], c.N, c.H, c.W, C,
                                 kp_sigmoid=False)
            torch.cuda.synchronize()
            return "heads2", [t.double().cpu() for t in outs], None, spy, True
        if c.op == "narrow":
            C, co, slot = c.cin, c.cout, c.slot
            c_lo = 0 if slot == 8 else 8
            g = torch.Generator().manual_seed(c.seed + 2)
            junk = torch.randn(c.N * c.H * c.W, 64, generator=g) * 100.0          # the other heads' channels of the packed dY rows: the kernel must not see them
            junk[:, c_lo:c_lo + slot] = 0.0
            junk[:, c_lo:c_lo + co] = rows(o.dy)
            gy = to_pt(junk, 1, fmt)[0]
            mask = to_pt(rows(o.mask), 1, fmt)[0]
            pw = ops.PackedWeight(C, 7 * slot // 8, 64, DEV, dtype=dt)
            pw.pack_narrow(o.w.to(DEV), slot)
            y, ybuf = to_pt(torch.full((c.N * c.H * c.W, C), FILL), 1, fmt, sliced=True, fill=FILL)
            ops.conv7_narrow(gy.t, pw, C, c.N, c.H, c.W, y.t, mask=mask.t, chan_lo=c_lo, chan_slot=slot)
            torch.cuda.synchronize()
            return "narrow", [nchw(from_pt(y), c.N, c.H, c.W)], None, spy, outside_is_fill(ybuf, 1, C, True)
    raise ValueError(c.op)


WORST = {}


@pytest.mark.parametrize("case", ACTIVE, ids=lambda c: c.name)
def test_case(case):
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    want_kind, want_key, _ = dc.plan(case)
    o = dc.Operands(case)
    kind, outs, stats, spy, untouched = run_case(case, o)
    assert len(spy.calls) == 1, (case, spy.calls)
    entry, key, kern = spy.calls[0]
    assert kind == want_kind, (case, kind, want_kind)
    assert kern == want_key.kernel == case.kernel, f"{case}: launched {kern}, planned {want_key.kernel}, meant to hit {case.kernel}"
    assert key == want_key, (case, key, want_key)
    r = dc.Reference(case, o)
    assert len(outs) == len(r.outs)
    fam = kern.split("<")[0]
    for which, got in enumerate(outs):
        d = r.outs[which]
        nbad, worst = r.violations(got, which)
        _, yard = r.violations(d["f32"], which)
        print(f"[{case.name} out {which}] {kern} split={key.split}: worst |d| / bound GPU {worst:.3f}, float32 yardstick {yard:.3f}; allowance {d['allow']:.3g} "
              f"u_out {d['u']:.3g} rms {d['rms']:.3g}")
        w = WORST.setdefault(fam, [0.0, 0.0])
        w[0], w[1] = max(w[0], worst), max(w[1], yard)
        assert bool(torch.isfinite(got).all()) and nbad == 0, (case, which, nbad, worst)
    assert untouched, (case, "columns outside the written channel slice changed")
    if stats is not None:
        val, bnd = dc.stats_reference(r)
        ratio = (stats - val).abs() / bnd
        print(f"[{case.name} statistics] worst |d| / bound sum {float(ratio[:, 0].max()):.3f}, second sum {float(ratio[:, 1].max()):.3f}")
        assert float(ratio.max()) <= 1.0, (case, ratio.max(0))


def test_worst_ratio_per_kernel_family():
    """(report) worst |d| / bound per kernel family over the cases of this process: GPU, float32 yardstick"""
    for fam, (g, y) in sorted(WORST.items()):
        print(f"[family {fam}] GPU {g:.3f}  float32 yardstick {y:.3f}")
    assert all(g <= 1.0 for g, _ in WORST.values())


_DIED = []


@pytest.mark.parametrize("env", SWITCH_ENVS, ids=lambda e: ",".join(f"{k}={v}" for k, v in e))
def test_switch_cases_in_a_child_process(env):
    """the cases that need a library switch: a fresh `python -m pytest -k test_case` child with the switch set (the library reads it once per process);
    the child's test_case asserts the kernel name, so a forced variant whose guard is false fails there instead of passing on the old kernel"""
    if _SET:
        return            # (this IS a child)
    assert not _DIED, f"not started: the child of {_DIED[0]} died, hung or faulted"
    n = sum(1 for c in dc.CASES if tuple(sorted((c.env or {}).items())) == env)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-s", "-m", "gpu", "-k", "test_case"], capture_output=True,
                           text=True, env=dict(os.environ, **dict(env)), cwd=root, timeout=300)
    except subprocess.TimeoutExpired:
        _DIED.append(env)          # a hung child: nothing more is started on the GPU by this file
        raise
    print(r.stdout[-3000:])
    out = r.stdout + r.stderr
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or "illegal memory access" in out or "HSA_STATUS_ERROR" in out or "Memory access fault" in out:
        _DIED.append(env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert f"{n} passed" in r.stdout.splitlines()[-1], r.stdout[-500:]


# ---- census of one train step ---------------------------------------------------------------------------------------------------------------

POLICIES = ("fp32", "fp32b2", "half", "bf16")
CASE_KEYS = [dc.plan(c)[1] for c in dc.CASES if not c.env]


def train_step_calls(policy, size=64, n_img=2, n_boxes=4, seed=5):
    from kg_instance_segmentation_amd import KGnet
    from kg_instance_segmentation_amd.loss import DetectionLossAll
    from kg_instance_segmentation_amd.seg_loss import SEG_loss
    from oracle import synth
    torch.manual_seed(seed)
    x, gt_boxes, gt_masks, gt_lv = synth.train_batch(n_img, size, size, seed, n_boxes=n_boxes)
    m = KGnet.resnet50(pretrained=False, precision=policy).to(DEV).train()
    m.zero_grad()
    ldec, lseg = DetectionLossAll(kp_radius=5), SEG_loss(height=size, width=size)
    with Spy() as spy:
        d0, d1, d2, d3, pred = m(x.to(DEV), gt_boxes)
        loss = sum(ldec(p, t.to(DEV)) for p, t in zip((d0, d1, d2, d3), gt_lv)) + lseg(pred, gt_masks, gt_boxes)
        loss.backward()
        torch.cuda.synchronize()
    return spy.calls


@pytest.mark.parametrize("policy", POLICIES)
def test_train_step_census(policy):
    """every dense launch of one train step: the library launched the kernel the planner derives from the call's arguments, and its class has a case"""
    if _SET:
        return            # (children run the switch cases only)
    assert not _DIED, f"not started: the child of {_DIED[0]} died, hung or faulted"
    calls = train_step_calls(policy)
    dense = [(e, k, kern) for e, k, kern in calls if k is not None]
    assert len(dense) >= 100, (policy, len(dense), len(calls))
    wrong = sorted({(e, k.kernel, kern) for e, k, kern in dense if k.kernel != kern})
    assert not wrong, f"{policy}: the planner and the library disagree (entry, planned, launched): {wrong}"
    classes = sorted(set(k for _, k, _ in dense), key=str)
    missing = [k for k in classes if not any(dc.covers(ck, k) for ck in CASE_KEYS)]
    print(f"[census {policy}] {len(dense)} dense launches of {len(calls)}, {len(classes)} classes, {len(missing)} without a case")
    assert not missing, f"{policy}: launch classes without a parity case (add the key to densecases.CENSUS_64):\n" + "\n".join(str(k) for k in missing)
