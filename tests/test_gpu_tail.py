"""The step tail against FLOAT64, element by element, on every index path a < 64 M-element tensor can reach.

What runs after the last conv of a train step -- kg_detection_loss_fwd / _bwd, kg_seg_loss, kg_sigmoid_inplace, kg_grad_pack / kg_grad_pack3, kg_grad_scale,
kg_scale_tensors, kg_wgrad_reduce / _multi / _bias with the deferred batch flush, kg_bias_grad, kg_pack_weight_batch and kg_adam_step -- is about 150 of the
676 launches of a step.  oracle/tailcases.py restates the launch geometry of each on the host, lists the cases with the index paths each one runs
(computed) and builds float64 references, bounds and mutants; tests/test_tail_cases_cpu.py proves on the CPU that every path has a case, that the
float32 CPU evaluation sits within every bound and that every mutant does not.  Here every case runs through ops / _lib.call:
  * kg_scale_tensors: bit-equal to one IEEE multiply per element (NaN for NaN); a guard before and after every tensor untouched; the flag as computed;
  * kg_adam_step (through _lib.call and through optim.Adam with two groups, a late parameter and an unaligned gradient view): m, v and the update
    p_new - p_old by the rows bound per job (+ 2^-24 |p_new|); g = 0 on zero moments leaves p bit-equal; g and the guards untouched;
  * kg_grad_scale: out[0] bit-equal to the reference power of two, out[1] == 1 / out[0], both scratch words zero, a second call gives the same;
  * kg_sigmoid_inplace: the rows bound + 2^-126, the special values each a group of its own;
  * the reductions: every element within the sum rule against float64 AND bit-equal to the float32 evaluation in the restated summation order;
    the deferred flush bit-equal to the immediate launches, job by job, outputs holding their fill until the flush, pending counts as documented;
    kg_wgrad_reduce_bias refuses 1 tap / 16 <= S < 32 with bias partials (no whole wave: reduce_shape used to divide by zero there);
  * the losses: all eight words of out8 (sum rule, product, exact), the three gradient maps per element (product bound, zero where the reference
    is zero), the scratch guard; kg_seg_loss forward and backward calls separately, elements outside every patch keep the fill;
  * kg_bias_grad: the sum rule per channel, columns of the wider buffer hold a large fill, scratch guard;
  * kg_grad_pack: the rows bound per element (half: + 2^-25), padding columns bit-zero, every other column still the fill; kg_grad_pack3 bit-equal to
    three kg_grad_pack launches, capped sizes included;
  * kg_pack_weight_batch: byte-equal to the single-tensor entry points on sentinel-filled buffers, immediate and held launches, both formats.
Left out, with the size they would need: det_loss_bwd_kernel's second trip (> 4096 x 256 pixels: about 700 MB of maps); grad_pack_kernel's (cpad > 64)
second trip (> 8192 x 256 pixels x 72 channels: 151 M output elements).

The job table optim.Adam builds is compared with tailcases.job_layout HERE (the optimizer refuses CPU parameters); those of ops.scale_tensors and
PackQueue.flush in tests/test_tail_cases_cpu.py.

MEASURED on MI355X, 2026-10-19, on this file as committed (192 tests, all passing; no kernel's arithmetic had to change -- the one library
change is the argument check of kg_wgrad_reduce_bias described above).  Worst |d| / bound over the cases of a kernel, GPU, in brackets the float32
CPU evaluation against the same bound:
  exact: kg_scale_tensors, kg_grad_scale (max 1e-38 -> 2^100 and 3e38 -> 2^-100 included), every reduction against its in-order float32 evaluation,
      the deferred flush against the immediate launches (44 jobs per library), kg_grad_pack3 against three kg_grad_pack, kg_pack_weight_batch (46 jobs)
  rows: adam m 0.231 (0.231), v 0.237 (0.237), update 0.912 (0.912: 2^-24 |p_new| IS the last rounding of p); sigmoid 0.069 (0.069);
      grad_pack bf16 P1 0.996 (0.996), bf16 P2 0.466 (0.466), half P1 0.995 (0.995), half P2 0.187 (0.187) (one plane: the bound is half an ulp of
      the stored format and correct rounding reaches it); grad_pack3 block 0 bf16 P1 0.969 (0.969), half P2 0.166 (0.166)
  sum: wgrad_reduce weights 0.970 (0.970: S = 1 with accumulate, where the bound is the one rounding of prior + sum), bias column 0.034 (0.034);
      bias_grad 0.038 (0.049); det_loss out8 0.650 (0.650); seg_loss loss 0.013 (0.094)
  product: det_loss g_kp 0.661 (0.661) with k = 7, g_sh 0.244 (0.244) with k = 7, g_md 0.175 (0.175) with k = 8; seg_loss gprob 0.391 (0.391)
  logf / log1pf term of the BCE sums: MARGIN x the CPU's worst float32 log / log1p error = 2.13 .. 2.49 ulps over the detection cases (per case, printed)
  wall time of this file 8 s; slowest: the optimizer test 1.6 s, det_loss 513 x 513 0.8 s, wgrad_reduce 256 x 449 x 49 0.6 s, every other case below 0.4 s.
"""
import ctypes
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from kg_instance_segmentation_amd import _lib, ops, optim  # noqa: E402
from kg_instance_segmentation_amd._lib import c_float, ptr, stream_ptr  # noqa: E402
from kg_instance_segmentation_amd.ops import PT, PackedWeight  # noqa: E402
from oracle import densecases as dc, tailcases as tc  # noqa: E402

DEV = "cuda"
GUARD_VAL = -777.0
WORST = {}
T0 = [None]


def note(k, gpu, yard=None):
    if T0[0] is None:
        T0[0] = time.time()
    a, b = WORST.get(k, (0.0, 0.0))
    WORST[k] = (max(a, gpu), max(b, yard if yard is not None else 0.0))
    return gpu


def ids(cases):
    return [c.name for c in cases]


def threads16():
    torch.set_num_threads(min(torch.get_num_threads(), 16))


class Guarded:
    """a flat fp32 device tensor `off` floats off 16-byte alignment, with 8 guard floats before and after"""
    PRE = POST = 8

    def __init__(self, x, off=0, dtype=torch.float32):
        n = x.numel()
        self.buf = torch.full((self.PRE + off + n + self.POST,), GUARD_VAL, dtype=dtype, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.lo, self.n = self.PRE + off, n
        self.view = self.buf[self.lo:self.lo + n]
        self.view.copy_(x.reshape(-1))

    def guards_ok(self):
        b = self.buf.cpu()
        return bool((b[:self.lo] == GUARD_VAL).all()) and bool((b[self.lo + self.n:] == GUARD_VAL).all())

    def host(self):
        return self.view.cpu()

    @property
    def ptr(self):
        """the device address of the view (an empty view reports a null data_ptr)"""
        return self.buf.data_ptr() + self.lo * self.buf.element_size()


def scalar(v):
    return None if v is None else torch.tensor([v], dtype=torch.float32, device=DEV)


# ---- kg_scale_tensors -------------------------------------------------------------------------------------------------------------------------------
SCALE_DT = np.dtype([("p", "<u8"), ("n", "<i8"), ("scale", "<u8"), ("blk0", "<i4"), ("pad", "<i4")])
ADAM_DT = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i8"), ("blk0", "<i4"), ("pad", "<i4")])


@pytest.mark.parametrize("case", tc.SCALE_CASES, ids=ids(tc.SCALE_CASES))
def test_scale_tensors(case):
    xs = tc.scale_operands(case)
    want, flag = tc.scale_reference(case, xs)
    bufs = [Guarded(x, off) for x, (n, off, si) in zip(xs, case.jobs)]
    scal = torch.tensor(tc.SCALES, dtype=torch.float32, device=DEV)
    blk0, total = tc.job_layout([n for n, _, _ in case.jobs])
    arr = np.zeros(len(case.jobs), SCALE_DT)
    for i, (b, (n, off, si)) in enumerate(zip(bufs, case.jobs)):
        arr[i] = (b.ptr, n, scal[si:si + 1].data_ptr(), blk0[i], 0)
        assert b.ptr % 16 == 4 * (off % 4) and (n == 0 or b.ptr == b.view.data_ptr())
    tab = ops.h2d(arr.view(np.uint8).reshape(-1), torch.device(DEV))
    fl = torch.zeros(1, dtype=torch.int32, device=DEV) if case.flag == "given" else None
    _lib.call("kg_scale_tensors", ptr(tab), len(case.jobs), total, ptr(fl), stream_ptr())
    torch.cuda.synchronize()
    for j, (b, w) in enumerate(zip(bufs, want)):
        assert tc.same_bits(b.host(), w), (case, j)
        assert b.guards_ok(), (case, j)
    if fl is not None:
        assert int(fl) == flag, (case, int(fl), flag)
    assert torch.equal(scal.cpu(), torch.tensor(tc.SCALES, dtype=torch.float32))
    note("scale_tensors (bit-equal)", 0.0)


def test_scale_tensors_through_ops_wrapper():
    """ops.scale_tensors on the 37-job table: the wrapper drops the empty tensor and lays the rest out as tailcases.job_layout does"""
    case = next(c for c in tc.SCALE_CASES if len(c.jobs) == 37)
    xs = tc.scale_operands(case)
    bufs = [Guarded(x, off) for x, (n, off, si) in zip(xs, case.jobs)]
    s = scalar(3.0)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.scale_tensors([b.view for b in bufs], s, flag=flag)
    torch.cuda.synchronize()
    for b, x in zip(bufs, xs):
        assert tc.same_bits(b.host(), x * torch.tensor(3.0)) and b.guards_ok()
    assert int(flag) == 0


# ---- kg_adam_step -----------------------------------------------------------------------------------------------------------------------------------

def check_adam_job(r, j, p_new, m_new, v_new, label, fixed_point):
    rr = r.job_ratio(j, p_new, m_new, v_new)
    y = r.yardstick(j)
    for k in rr:
        assert note("adam " + k, rr[k], y[k]) <= 1.0, (label, j, k, rr)
    if fixed_point:
        assert torch.equal(p_new, r.ops[j][0]) and not bool(m_new.any()) and not bool(v_new.any()), (label, j)


@pytest.mark.parametrize("case", tc.ADAM_CASES, ids=ids(tc.ADAM_CASES))
def test_adam_step(case):
    r = tc.AdamReference(case)
    bufs = [[Guarded(t, off) for t, off in zip(job_ops, offs)] for job_ops, (n, offs, gm) in zip(r.ops, case.jobs)]
    blk0, total = tc.job_layout([n for n, _, _ in case.jobs])
    arr = np.zeros(len(case.jobs), ADAM_DT)
    for i, (b, (n, offs, gm)) in enumerate(zip(bufs, case.jobs)):
        arr[i] = tuple(x.ptr for x in b) + (n, blk0[i], 0)
    tab = ops.h2d(arr.view(np.uint8).reshape(-1), torch.device(DEV))
    s = r.s
    _lib.call("kg_adam_step", ptr(tab), len(case.jobs), total, c_float(s["beta1"]), c_float(s["beta2"]), c_float(s["eps"]), c_float(s["step"]),
              c_float(s["bc2s"]), c_float(s["wd"]), stream_ptr())
    torch.cuda.synchronize()
    for j, (b, (n, offs, gm)) in enumerate(zip(bufs, case.jobs)):
        check_adam_job(r, j, b[0].host(), b[2].host(), b[3].host(), case.name, gm == 0.0 and case.t == 1 and case.wd == 0.0)
        assert torch.equal(b[1].host(), r.ops[j][1]), (case, j, "the gradient is read only")
        assert all(x.guards_ok() for x in b), (case, j)


def test_adam_optimizer_groups_late_parameter_unaligned_gradient(monkeypatch):
    """optim.Adam: two parameter groups with different lr, a parameter that joins at step 2 (its own bias correction: a second launch for its group),
    a gradient that is an unaligned view; every launch's job table equals tailcases.job_layout; every step against float64 from the state before it"""
    g = torch.Generator().manual_seed(5)
    shapes = [(4097,), (33, 7), (4096,), (1000,)]
    params = [torch.nn.Parameter((0.01 * torch.randn(s, generator=g)).to(DEV)) for s in shapes]
    opt = optim.Adam([{"params": [params[0], params[1], params[3]], "lr": 1e-4}, {"params": [params[2]], "lr": 3e-4}], weight_decay=0.01)
    launches = []
    real_call = _lib.call

    def spy(name, *a, **kw):
        if name == "kg_adam_step":
            launches.append((a[1], a[2], float(a[6].value)))
        return real_call(name, *a, **kw)
    monkeypatch.setattr(_lib, "call", spy)
    grads_store = torch.zeros(4 + 231, device=DEV)
    for step in (1, 2):
        grads = [torch.randn(s, generator=g) * (0.5 + i) for i, s in enumerate(shapes)]
        live = [0, 1, 2] if step == 1 else [0, 1, 2, 3]
        for i in range(4):
            params[i].grad = None
        for i in live:
            if i == 1:
                grads_store[1:232].copy_(grads[1].reshape(-1))
                params[1].grad = grads_store[1:232].view(33, 7)
                assert params[1].grad.data_ptr() % 16 == 4 and params[1].grad.is_contiguous()
            else:
                params[i].grad = grads[i].to(DEV)
        before = {}
        for i in live:
            st = opt.state.get(params[i], {})
            before[i] = (params[i].detach().cpu().reshape(-1).clone(), grads[i].reshape(-1),
                         st["exp_avg"].cpu().reshape(-1).clone() if st else torch.zeros(params[i].numel()),
                         st["exp_avg_sq"].cpu().reshape(-1).clone() if st else torch.zeros(params[i].numel()))
        launches.clear()
        opt.step()
        torch.cuda.synchronize()
        # launches: group 0 at t = step (and, at step 2, the late parameter at t = 1), group 1
        want = [([4097, 231], 1e-4, step)] + ([([1000], 1e-4, 1)] if step == 2 else []) + [([4096], 3e-4, step)]
        assert len(launches) == len(want), launches
        for (nj, blk, step_size), (ns, lr, t) in zip(launches, want):
            assert nj == len(ns) and blk == tc.job_layout(ns)[1]
            assert step_size == tc.adam_scalars(lr, 0.9, 0.999, 1e-8, 0.01, t)["step"]
        for i in live:
            lr = 3e-4 if i == 2 else 1e-4
            t = 1 if (i == 3) else step
            r = tc.AdamReference(None, ops_=[before[i]], scalars=tc.adam_scalars(lr, 0.9, 0.999, 1e-8, 0.01, t))
            st = opt.state[params[i]]
            check_adam_job(r, 0, params[i].detach().cpu().reshape(-1), st["exp_avg"].cpu().reshape(-1), st["exp_avg_sq"].cpu().reshape(-1), f"optimizer step {step}", False)
            assert float(st["step"]) == t


# ---- kg_grad_scale ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tc.GS_CASES, ids=ids(tc.GS_CASES))
def test_grad_scale(case):
    threads16()
    o = tc.gs_operands(case)
    S = tc.gs_scale(tc.gs_max(o, torch.float32))
    pb = [Guarded(p, poff) for (p, q), (n, poff, hasq, qoff) in zip(o, case.tensors)]
    qb = [Guarded(q, qoff) if q is not None else None for (p, q), (n, poff, hasq, qoff) in zip(o, case.tensors)]
    nt = len(o)
    ptrs = (ctypes.c_void_p * nt)(*[b.ptr for b in pb])
    prbs = (ctypes.c_void_p * nt)(*[b.ptr if b is not None else None for b in qb])
    cnts = (ctypes.c_long * nt)(*[n for n, *_ in case.tensors])
    scr = Guarded(torch.zeros(2), 0, dtype=torch.int32)
    scr.buf.fill_(-777)
    scr.view.zero_()
    for rep in range(2):
        out = torch.full((2,), float("nan"), dtype=torch.float32, device=DEV)
        _lib.call("kg_grad_scale", ptrs, prbs, cnts, nt, tc.GS_TARGET, ptr(scr.view), ptr(out), stream_ptr())
        torch.cuda.synchronize()
        got = out.cpu()
        assert float(got[0]) == S, (case, rep, float(got[0]), S)
        assert float(got[1]) == 1.0 / float(got[0]), (case, rep)
        b = scr.buf.cpu()
        assert b[scr.lo:scr.lo + 2].tolist() == [0, 0] and bool((b[:scr.lo] == -777).all()) and bool((b[scr.lo + 2:] == -777).all()), (case, rep)
    for b, (p, q) in zip(pb, o):
        assert tc.same_bits(b.host(), p) and b.guards_ok()
    note("grad_scale (bit-equal)", 0.0)


# ---- kg_sigmoid_inplace -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tc.SIG_CASES, ids=ids(tc.SIG_CASES))
def test_sigmoid(case):
    threads16()
    r = tc.SigReference(case)
    b = Guarded(r.x)
    ops.sigmoid_(b.view)
    torch.cuda.synchronize()
    got = b.host()
    assert note("sigmoid", r.ratio(got), r.ratio(r.f32)) <= 1.0, case
    assert b.guards_ok()


# ---- split weight-gradient reductions ---------------------------------------------------------------------------------------------------------------
PARTS = {}


def red_ref(c):
    if c.name not in PARTS:
        r = tc.RedReference(c)
        PARTS[c.name] = (r, r.part.to(DEV), r.bpart.to(DEV) if c.bias_C else None)
    return PARTS[c.name]


def red_outputs(c, r, acc):
    """fresh output tensors: the fill (accumulate 0) or the prior values (accumulate 1)"""
    k = int(round(c.taps ** 0.5))
    outs, row = [], 0
    for n in c.counts:
        t = torch.full((n, c.cin, k, k), tc.FILL, dtype=torch.float32, device=DEV)
        if acc:
            t.copy_(r.prior[row:row + n].reshape(n, c.cin, k, k))
        outs.append(t)
        row += n
    db = None
    if c.bias_C:
        db = torch.full((c.bias_C,), tc.FILL, dtype=torch.float32, device=DEV)
        if acc:
            db.copy_(r.bprior)
    return outs, db


def red_launch(c, part, bpart, outs, db, acc, fmt=0):
    k = int(round(c.taps ** 0.5))
    cout = sum(c.counts)
    stride = ctypes.c_long(cout * c.taps * c.cin)
    gp = (ctypes.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
    cn = (ctypes.c_int * len(outs))(*c.counts)
    if c.bias_C:
        _lib.call("kg_wgrad_reduce_bias", ptr(part), gp, cn, len(outs), c.cin, k, k, c.S, stride, acc, ptr(bpart), ptr(db), c.bias_C, stream_ptr(), fmt=fmt)
    elif len(outs) == 1:
        _lib.call("kg_wgrad_reduce", ptr(part), ptr(outs[0]), cout, c.cin, k, k, c.S, stride, acc, stream_ptr(), fmt=fmt)
    else:
        _lib.call("kg_wgrad_reduce_multi", ptr(part), gp, cn, len(outs), c.cin, k, k, c.S, stride, acc, stream_ptr(), fmt=fmt)
    return gp, cn          # (kept alive by the caller until the launch is enqueued)


def red_got(c, outs):
    return torch.cat([o.reshape(o.shape[0], c.cin, c.taps) for o in outs], 0).cpu()


@pytest.mark.parametrize("case", tc.RED_CASES, ids=ids(tc.RED_CASES))
def test_wgrad_reduce(case):
    threads16()
    r, part, bpart = red_ref(case)
    for acc in (0, 1):
        outs, db = red_outputs(case, r, acc)
        red_launch(case, part, bpart, outs, db, acc)
        torch.cuda.synchronize()
        exp = r.expect(acc)
        got = {"w": red_got(case, outs)}
        if case.bias_C:
            got["b"] = db.cpu()
        for name, (r64, r32, b) in exp.items():
            assert note("wgrad_reduce " + name, tc.ratio(got[name].double() - r64, b), tc.ratio(r32.double() - r64, b)) <= 1.0, (case, acc, name)
            assert torch.equal(got[name], r32), (case, acc, name, "not the restated summation order")


@pytest.mark.parametrize("fmt", [0, 1], ids=["bf16 library", "half library"])
def test_wgrad_reduce_deferred_flush_is_bit_equal_to_the_immediate_launches(fmt):
    threads16()
    jobs = tc.defer_jobs()
    immediate = []
    for c, acc in jobs:
        r, part, bpart = red_ref(c)
        outs, db = red_outputs(c, r, acc)
        red_launch(c, part, bpart, outs, db, acc, fmt=fmt)
        immediate.append((outs, db))
    torch.cuda.synchronize()
    lib = _lib.load(fmt)
    deferred, keep = [], []
    try:
        _lib.call("kg_wgrad_reduce_defer", 1, fmt=fmt)
        for c, acc in jobs:
            r, part, bpart = red_ref(c)
            outs, db = red_outputs(c, r, acc)
            keep.append(red_launch(c, part, bpart, outs, db, acc, fmt=fmt))
            deferred.append((outs, db))
        assert lib.kg_wgrad_reduce_pending() == len(jobs)
        torch.cuda.synchronize()
        for (c, acc), (outs, db) in zip(jobs, deferred):          # nothing has run: fill or prior values still there
            r = red_ref(c)[0]
            want, wdb = red_outputs(c, r, acc)
            assert all(torch.equal(a, b) for a, b in zip(outs, want)) and (db is None or torch.equal(db, wdb)), (c, acc)
        _lib.call("kg_wgrad_reduce_flush", stream_ptr(), fmt=fmt)
        assert lib.kg_wgrad_reduce_pending() == 0
        torch.cuda.synchronize()
    finally:
        _lib.call("kg_wgrad_reduce_defer", 0, fmt=fmt)
    assert lib.kg_wgrad_reduce_pending() == 0
    for (c, acc), (o1, d1), (o2, d2) in zip(jobs, immediate, deferred):
        assert all(torch.equal(a, b) for a, b in zip(o1, o2)), (c, acc, "deferred weights differ from the immediate launch")
        assert d1 is None or torch.equal(d1, d2), (c, acc, "deferred bias differs from the immediate launch")
        assert not bool((o2[0] == tc.FILL).all())


@pytest.mark.parametrize("fmt", [0, 1], ids=["bf16 library", "half library"])
def test_wgrad_reduce_bias_refuses_blocks_without_a_whole_wave(fmt):
    """1 tap, CH = 16, 16 <= S < 32 gives 32- or 48-thread blocks: reduce_shape divided by nt / 64 == 0 when bias partials came along (the C ABI
    could reach it, ops.conv_wgrad cannot).  Now an argument error, nothing launched; the same shape without bias partials still reduces."""
    lib = _lib.load(fmt)
    for d in tc.REFUSED:
        cout = sum(d["counts"])
        part = torch.ones(d["S"], cout, 1, d["cin"], device=DEV)
        out = torch.full((cout, d["cin"], 1, 1), tc.FILL, device=DEV)
        bpart, db = torch.ones(d["S"], d["bias_C"], device=DEV), torch.full((d["bias_C"],), tc.FILL, device=DEV)
        gp, cn = (ctypes.c_void_p * 1)(out.data_ptr()), (ctypes.c_int * 1)(cout)
        rc = lib.kg_wgrad_reduce_bias(ptr(part), gp, cn, 1, d["cin"], 1, 1, d["S"], ctypes.c_long(cout * d["cin"]), 0, ptr(bpart), ptr(db), d["bias_C"], stream_ptr())
        torch.cuda.synchronize()
        assert rc == 1 and b"whole wave" in lib.kg_last_error(), (d, rc, lib.kg_last_error())
        assert bool((out == tc.FILL).all()) and bool((db == tc.FILL).all())
        rc = lib.kg_wgrad_reduce_bias(ptr(part), gp, cn, 1, d["cin"], 1, 1, d["S"], ctypes.c_long(cout * d["cin"]), 0, None, None, 0, stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0 and bool((out == float(d["S"])).all())


# ---- detection loss ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tc.DET_CASES, ids=ids(tc.DET_CASES))
def test_detection_loss(case):
    threads16()
    r = tc.DetReference(case)
    o = r.o
    dev = {k: o[k].to(DEV) for k in ("kp", "sh", "md", "gt")}
    den = o["den"].to(DEV) if o["den"] is not None else None
    nscr = case.get("scratch", tc.DET_SCRATCH)
    scr = Guarded(torch.zeros(nscr))
    out8 = torch.full((8,), float("nan"), dtype=torch.float32, device=DEV)
    _lib.call("kg_detection_loss_fwd", ptr(dev["kp"]), ptr(dev["sh"]), ptr(dev["md"]), ptr(dev["gt"]), case.N, case.H, case.W, c_float(tc.KP_RADIUS), ptr(den),
              ptr(scr.view), nscr, ptr(out8), stream_ptr())
    torch.cuda.synchronize()
    got8 = out8.cpu()
    per = ((got8.double() - r.out8).abs() / r.b8.clamp_min(1e-300)).tolist()
    print(f"[out8] {case.name}: got {got8.tolist()} ratios {[round(x, 3) for x in per]} log term {r.log_ulps:.2f} ulps")
    assert note("det_loss out8", r.out8_ratio(got8), r.out8_ratio(r.yardstick8())) <= 1.0, (case, per)
    assert scr.guards_ok()
    if case.get("gt") == "zero":
        assert float(got8[2]) == 0.0 and float(got8[3]) == 0.0 and float(got8[7]) == 0.0
    go = scalar(o["go"])
    g_kp, g_sh, g_md = (torch.full_like(dev[k], tc.FILL) for k in ("kp", "sh", "md"))
    _lib.call("kg_detection_loss_bwd", ptr(dev["kp"]), ptr(dev["sh"]), ptr(dev["md"]), ptr(dev["gt"]), case.N, case.H, case.W, c_float(tc.KP_RADIUS), ptr(out8),
              ptr(go), ptr(g_kp), ptr(g_sh), ptr(g_md), stream_ptr())
    torch.cuda.synchronize()
    ref = r.grads(torch.float64)
    bnd = r.grad_bounds(ref)
    small = r.geom["total"] <= 100_000
    f32 = r.grads(torch.float32) if small else None
    for k, t in (("g_kp", g_kp), ("g_sh", g_sh), ("g_md", g_md)):
        y = tc.ratio(f32[k].double() - ref[k], bnd[k]) if small else None
        assert note("det_loss " + k, tc.ratio(t.cpu().double() - ref[k], bnd[k]), y) <= 1.0, (case, k)


# ---- seg loss ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tc.SEG_CASES, ids=ids(tc.SEG_CASES))
def test_seg_loss(case):
    r = tc.SegReference(case)
    o = r.o
    dev = torch.device(DEV)
    ptab = ops.h2d(np.ascontiguousarray(np.array(o["patches"], np.int32)), dev)
    pair_t = np.zeros(len(o["pairs"]), dtype=[("off", np.int32), ("w", np.float32)])
    pair_t["off"], pair_t["w"] = [p[0] for p in o["pairs"]], [p[1] for p in o["pairs"]]
    pairs_d = ops.h2d(pair_t.view(np.uint8), dev)
    prob, tgt = o["prob"].to(DEV), o["tgt"].to(DEV)
    part = Guarded(torch.zeros(case.npatches))
    out = torch.full((1,), float("nan"), device=DEV)
    _lib.call("kg_seg_loss", ptr(prob), ptr(tgt), ptr(ptab), ptr(pairs_d), case.npatches, ptr(part.view), ptr(out), None, None, stream_ptr())      # forward
    torch.cuda.synchronize()
    b1 = r.bloss.reshape(1)
    assert note("seg_loss loss", tc.ratio((out.cpu().double() - r.loss).reshape(1), b1), tc.ratio((r.loss32.double() - r.loss).reshape(1), b1)) <= 1.0, case
    assert part.guards_ok()
    gprob = torch.full_like(prob, tc.FILL)
    go = scalar(o["go"])
    _lib.call("kg_seg_loss", ptr(prob), ptr(tgt), ptr(ptab), ptr(pairs_d), case.npatches, None, None, ptr(go), ptr(gprob), stream_ptr())          # backward
    torch.cuda.synchronize()
    g = gprob.cpu()
    assert bool((g[~r.written] == tc.FILL).all()), (case, "an element outside every patch was written")
    w = r.written
    assert note("seg_loss gprob", tc.ratio(g[w].double() - r.g[w], r.bg[w]), tc.ratio(r.g32[w].double() - r.g[w], r.bg[w])) <= 1.0, case
    assert torch.equal(prob.cpu(), o["prob"])


# ---- kg_bias_grad -------------------------------------------------------------------------------------------------------------------------------------
BIG_FILL = 1000.0


@pytest.mark.parametrize("case", tc.BIAS_CASES, ids=ids(tc.BIAS_CASES))
def test_bias_grad(case):
    threads16()
    r = tc.BiasReference(case)
    ctot, c0 = tc.bias_layout(case)
    dt = dc.DT[case.fmt]
    buf = torch.full((case.M, case.P * ctot), BIG_FILL, dtype=dt)
    for p, plane in enumerate(dc.split_planes(r.dy, case.fmt, case.P)):
        buf[:, p * ctot + c0:p * ctot + c0 + case.C] = plane.to(dt)
    buf = buf.to(DEV)
    view = buf[:, c0:c0 + case.C]
    assert (view.data_ptr() % 16 == 0) == (not case.get("misalign"))
    db = r.prior.to(DEV) if case.accumulate else torch.full((case.C,), tc.FILL, device=DEV)
    fmt = 1 if case.fmt == "half" else 0
    if case.get("scratch"):
        scr = Guarded(torch.zeros(case.scratch))
        for p in range(case.P):
            _lib.call("kg_bias_grad", ops.ctypes_offset(view, p * ctot), ptr(db), ptr(scr.view), case.scratch, case.M, case.C, buf.stride(0),
                      1 if (case.accumulate or p > 0) else 0, stream_ptr(), fmt=fmt)
        torch.cuda.synchronize()
        assert scr.guards_ok()
    else:
        ops.bias_grad(PT(view, case.P, ctot) if case.P > 1 else view, case.C, db, accumulate=case.accumulate)
        torch.cuda.synchronize()
    assert note("bias_grad", tc.ratio(db.cpu().double() - r.ref, r.bound), tc.ratio(r.f32.double() - r.ref, r.bound)) <= 1.0, case


# ---- kg_grad_pack / kg_grad_pack3 ---------------------------------------------------------------------------------------------------------------------

class PackOut:
    """[R, P * ctot] output buffer of fill values; the written slice is columns [8, 8 + cpad) of every plane"""

    def __init__(self, R, cpad, fmt, P, fill=tc.FILL):
        self.ctot, self.cpad, self.P, self.fill = cpad + 16, cpad, P, fill
        self.buf = torch.full((R, P * self.ctot), fill, dtype=dc.DT[fmt], device=DEV)
        self.pt = PT(self.buf[:, 8:8 + cpad], P, self.ctot)

    def planes(self):
        return [self.pt.plane(p).cpu() for p in range(self.P)]

    def outside_is_fill(self):
        m = torch.ones(self.buf.shape[1], dtype=torch.bool)
        for p in range(self.P):
            m[p * self.ctot + 8:p * self.ctot + 8 + self.cpad] = False
        return bool((self.buf[:, m.to(DEV)].float() == self.fill).all())


@pytest.mark.parametrize("case", tc.GP_CASES, ids=ids(tc.GP_CASES))
def test_grad_pack(case):
    threads16()
    grad, prob = tc.gp_operands(case)
    prob = prob if case.prob else None
    r = tc.GradPackReference(case, grad, prob)
    out = PackOut(r.ref.shape[0], case.cpad, case.fmt, case.P)
    ops.grad_pack(grad.to(DEV), prob.to(DEV) if prob is not None else None, out.pt, case.N, case.C, case.H, case.W, case.cpad, scale=scalar(tc.GP_SCALE) if case.scale else None)
    torch.cuda.synchronize()
    planes = out.planes()
    got = planes[-1].double()
    for p in range(case.P - 2, -1, -1):
        got = got + planes[p].double()
    assert note(f"grad_pack {case.fmt} P{case.P}", r.ratio(got[:, :case.C]), r.ratio(r.f32)) <= 1.0, case
    for p, pl in enumerate(planes):
        assert not bool(pl[:, case.C:].view(torch.int16).any()), (case, p, "padding columns must be bit-zero")
    assert out.outside_is_fill(), case


@pytest.mark.parametrize("case", tc.GP3_CASES, ids=ids(tc.GP3_CASES))
def test_grad_pack3_is_bit_equal_to_three_grad_packs(case):
    threads16()
    gs = [tc.gp_operands(case, C, salt=k)[0].to(DEV) for k, C in enumerate(case.Cs)]
    prob = tc.gp_operands(case, case.Cs[0], salt=7)[1].to(DEV)
    R, cpad = case.N * case.H * case.W, sum(case.pads)
    one, three = PackOut(R, cpad, case.fmt, case.P, 3.0), PackOut(R, cpad, case.fmt, case.P, 3.0)
    s = scalar(tc.GP_SCALE)
    ops.grad_pack3(gs, prob, one.pt, case.N, case.Cs, case.H, case.W, case.pads, scale=s)
    off = 0
    for k in range(3):
        ops.grad_pack(gs[k], prob if k == 0 else None, three.pt.cols(off, off + case.pads[k]), case.N, case.Cs[k], case.H, case.W, case.pads[k], scale=s)
        off += case.pads[k]
    torch.cuda.synchronize()
    assert torch.equal(one.buf.view(torch.int16), three.buf.view(torch.int16)), case
    assert one.outside_is_fill()
    pl0 = one.pt.plane(0)
    assert bool((pl0[:, :case.Cs[0]].float() != 0).any()) and not bool(pl0[:, case.Cs[0]:case.pads[0]].view(torch.int16).any())
    if R < 100_000:          # and the first block against float64 (kp gradient times p (1 - p))
        cc = tc.Case("grad_pack", "block 0 of " + case.name, N=case.N, C=case.Cs[0], cpad=case.pads[0], H=case.H, W=case.W, fmt=case.fmt, P=case.P, prob=True, scale=True)
        r = tc.GradPackReference(cc, gs[0].cpu(), prob.cpu())
        planes = one.planes()
        got = planes[-1].double()
        for p in range(case.P - 2, -1, -1):
            got = got + planes[p].double()
        assert note(f"grad_pack3 {case.fmt} P{case.P}", r.ratio(got[:, :case.Cs[0]]), r.ratio(r.f32)) <= 1.0, case


# ---- kg_pack_weight_batch -------------------------------------------------------------------------------------------------------------------------------
SENTINEL = 3.0


def pack_targets(jobs, dtype):
    """a sentinel-filled PackedWeight per job (the three `rows` jobs of a head triple share one, as the fused second-layer heads do)"""
    pws, shared = [], None
    for kind, cout, cin, k, xP, wP, row0, c0, extra in jobs:
        taps = k * k
        if kind == "fwd":
            pw = PackedWeight(row0 + cout, taps, dc.round_up(c0 + cin, 64), DEV, xP, wP, dtype=dtype)
        elif kind == "tr":
            pw = PackedWeight(row0 + cin, taps, dc.round_up(c0 + cout, 64), DEV, xP, wP, dtype=dtype)
        elif kind == "rows":
            if extra == 0:
                shared = PackedWeight(64, taps, cin, DEV, xP, wP, groups=3, dtype=dtype)
                shared.buf.fill_(SENTINEL)
            pw = shared
        else:
            pw = PackedWeight(row0 + cin, 7 * extra // 8, 64, DEV, dtype=dtype)
        if kind != "rows":
            pw.buf.fill_(SENTINEL)
        pws.append(pw)
    return pws


def pack_all(jobs, pws, ws, rowmaps):
    for (kind, cout, cin, k, xP, wP, row0, c0, extra), pw, w in zip(jobs, pws, ws):
        if kind == "fwd":
            pw.pack(w, row0=row0, c0=c0)
        elif kind == "tr":
            pw.pack(w, row0=row0, c0=c0, transposed=True)
        elif kind == "rows":
            pw.pack_rows(w, rowmaps[extra], group=extra)
        else:
            pw.pack_narrow(w, extra, row0=row0)


@pytest.mark.parametrize("hold", [False, True], ids=["immediate flush", "held launch"])
@pytest.mark.parametrize("dtype", [ops.BF16, ops.F16], ids=["bf16", "half"])
def test_pack_weight_batch_is_byte_equal_to_the_single_tensor_packs(dtype, hold):
    jobs = tc.pack_jobs()
    g = torch.Generator().manual_seed(11)
    ws = [(torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).to(DEV) for kind, cout, cin, k, *_ in jobs]
    rows, _ = ops.heads2_layout()
    rowmaps = [torch.tensor(rw, dtype=torch.int32, device=DEV) for rw in rows]
    single, batched = pack_targets(jobs, dtype), pack_targets(jobs, dtype)
    ops.flush_packs()
    was = ops.PACKQ.defer
    try:
        ops.PACKQ.defer = False
        pack_all(jobs, single, ws, rowmaps)
        ops.PACKQ.defer = True
        pack_all(jobs, batched, ws, rowmaps)
        q = ops.PACKQ16 if dtype == ops.F16 else ops.PACKQ
        assert len(q.jobs) == len(jobs)
        torch.cuda.synchronize()
        assert all(bool((pw.buf == SENTINEL).all()) for pw in batched), "a deferred pack must not run before the flush"
        ops.flush_packs(hold=hold)
        if hold:
            assert q.pending is not None
            torch.cuda.synchronize()
            assert all(bool((pw.buf == SENTINEL).all()) for pw in batched), "a held batch must not run before launch_held_packs"
            ops.launch_held_packs()
        assert q.pending is None and not q.jobs
        torch.cuda.synchronize()
    finally:
        ops.PACKQ.defer = was
    for j, (a, b) in enumerate(zip(single, batched)):
        assert torch.equal(a.buf.view(torch.int16), b.buf.view(torch.int16)), (jobs[j], "batched pack differs from the single-tensor pack")
        assert bool((a.buf != SENTINEL).any()) and bool((a.buf == SENTINEL).any())
    # one forward and one transposed single-plane job against the planes of the weights at their restated positions
    fmt = "half" if dtype == ops.F16 else "bf16"
    for want_kind in ("fwd", "tr"):
        j = next(i for i, jb in enumerate(jobs) if jb[0] == want_kind and (jb[4], jb[5]) == (1, 1) and jb[3] == 3)
        kind, cout, cin, k, xP, wP, row0, c0, _ = jobs[j]
        pw, w = batched[j], ws[j].cpu()
        plane = (dc.split_planes(w, fmt, 1, dc.wscale_of(fmt))[0] * dc.wscale_of(fmt)).to(dtype).reshape(cout, cin, k * k)          # (stored times KG_WSCALE)
        buf = pw.buf.cpu()
        for tap in range(k * k):
            col = tap * pw.cin_pad + c0
            if kind == "fwd":
                assert torch.equal(buf[row0:row0 + cout, col:col + cin], plane[:, :, tap]), (jobs[j], tap)
            else:
                assert torch.equal(buf[row0:row0 + cin, col:col + cout], plane[:, :, tap].t()), (jobs[j], tap)


# ---- report -------------------------------------------------------------------------------------------------------------------------------------------

def test_worst_ratio_per_kernel():
    """(report) worst |d| / bound per kernel over the cases run in this process: GPU, in brackets the float32 CPU evaluation"""
    for k, (gpu, yard) in sorted(WORST.items()):
        print(f"[GPU / bound (float32 yardstick / bound)] {k}: {gpu:.3f} ({yard:.3f})")
    if T0[0] is not None:
        print(f"[wall] {time.time() - T0[0]:.1f} s since the first case of this file")
    assert all(gpu <= 1.0 for gpu, _ in WORST.values())
