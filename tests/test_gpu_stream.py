"""The streaming kernels of csrc/norm_pool.hip against FLOAT64, element by element, on every index path a < 64 M-element tensor can reach.

BatchNorm train / frozen (statistics, apply, backward), the max-pool, the dense bilinear resize with its exact-2x kernel, add_rows, rows_rescale /
rows_scale / rows_scale_multi and img_pack are about 300 of the 676 launches of a train step.  oracle/streamcases.py restates their launch geometry on
the host, lists the cases with the index paths each one runs (computed, not asserted by hand) and builds float64 references, bounds and mutants;
tests/test_stream_cases_cpu.py proves on the CPU that every listed path has a case, that the float32 CPU evaluation sits within every bound and that
one misplaced or unwritten 16-byte chunk, one dropped row of a reduction and a missed maximum do not.  Here every case runs through ops / _lib.call:
  * every element of every rows output is compared with float64 within
        U_OUT[(fmt, P)] * |ref| + max(4 x worst |float32 CPU evaluation - float64| over the case, 2e-6 x rms(ref))      (streamcases.RowsOut)
    bit for bit where the operation is exact (max-pool forward and its argmax bytes, rows_scale* by a power of two, img_pack's padding channels);
  * every reduced quantity (mean, invstd, scale, shift, running statistics, dgamma, dbeta, the three coef rows) within the sum rule of
    densecases.stats_reference propagated linearly (streamcases module docstring);
  * every column outside the written slice, every plane, still holds the fill value; the scratch of a reduction is followed by a guard that must
    stay untouched; rows_rescale leaves its two scratch words zero;
  * the max-pool backward runs with the stored argmax and by re-scanning: bit-equal to each other, ties compared (nine-value inputs), not masked;
  * kg_bn_bwd from host-built partials [nb][C][2] with parts_scale = 2^-3 equals the column-reduction route within the sum bound;
  * M = 0 returns KG_OK and writes nothing for the entry points that document it (kg_add_rows, kg_bilinear_fwd, kg_bilinear_bwd, kg_rows_rescale,
    kg_rows_scale); no other entry point is called with M = 0.
Left out, with the size they would need: the max-pool FORWARD's second grid-stride trip (a 134 M-element input), the exact-2x bilinear kernel's
(65 536 x 256 threads x 8 rows: about 1 G input elements), the 64-bit branch of kg_divmod (> 2^32 chunks).  reduce_geometry caps n at 512, which
at M = 131 100 gives rows_per_block = 257 and nb = 511 (the table computes it; the cap is what the case is for).

CONDITIONING (test_conditioning_30_sigma; measured, not a parity case).  Channels with |mean| = 30 sigma, M = 8225, C = 72, three bf16 planes: the
one-pass variance q / M - mean^2 cancels 900 : 1.  Yardstick: the float32 evaluation of the SAME formula -- sum x and sum x^2 in float32 in
colreduce_kernel's decomposition, combined in double (streamcases.onepass_f32).  Measured on the CPU: that evaluation has a relative invstd error
of 3.9e-5 against float64; torch's own float32 batch_norm (two-pass) is 1.3e-5 off in y = (x - mean) * invstd, i.e. the one-pass formula is not
what limits a 30-sigma channel by more than 3 x.  Asserted: kernel error <= 2^-24 |ref| + MARGIN x that evaluation's error.

MEASURED on MI355X, 2026-10-19, on this file as committed (1116 cases, 1120 tests, all passing; no kernel had to change).  Worst |d| / bound over
the cases of a kernel, GPU, in brackets the float32 CPU evaluation (rounded to the output's planes) against the same bound:
  rows outputs (the worst case has a single-plane output, where the bound is half an ulp of the stored format and correct rounding reaches it):
      bn_apply y 0.996 (0.996), bn_bwd dx 0.995 (0.995), bn_frozen dx 0.994 (0.994), bn_frozen scale-only dx 0.994 (0.994), add_rows y 0.998 (0.998),
      maxpool dx 0.997 (0.997), maxpool y and argmax bytes bit-equal, bilinear_fwd y 0.998 (0.998), bilinear_bwd dx
      0.996 (0.996), img_pack y 0.996 (0.996), padding channels bit-zero; rows_rescale / rows_scale / rows_scale_multi bit-equal, r and cum_out exact
  reduced quantities: bn_stats mean 0.131 (0.102), invstd 0.124 (0.139), scale 0.122 (0.157), shift 0.158 (0.150), running_mean 0.298 (0.298),
      running_var 0.222 (0.222); bn_finalize mean 0.028 (0.097), invstd 0.044 (0.120), scale 0.079 (0.137), shift 0.170 (0.170), running_mean
      0.315 (0.315), running_var 0.238 (0.238); bn_bwd dgamma 0.078 (0.053), dbeta 0.388 (0.388), coef 0.988 (0.988: the row a = gamma * invstd is ONE
      fp32 rounding on both sides, against 2^-24 |a|); bn_frozen dgamma 0.300 (0.300), dbeta 0.300 (0.300)
  conditioning (|mean| / sigma 29.4): relative invstd error kernel 3.98e-5, float32 one-pass evaluation 3.87e-5 (torch float32 batch_norm 1.3e-5 in y);
      mean error kernel 2.59e-6, evaluation 1.35e-6 (the kernel's mean is rounded to fp32: 2^-24 x 40 = 2.4e-6)
  wall time of this file 39 s; slowest case bn_bwd M524300 C64 wraps 4.9 s, the seven ~33 M-element cases 2.6 .. 4.9 s each (float64 reference),
      every other case below 1 s.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from kg_instance_segmentation_amd import _lib, ops  # noqa: E402
from kg_instance_segmentation_amd._lib import c_float, ptr, stream_ptr  # noqa: E402
from kg_instance_segmentation_amd.ops import PT  # noqa: E402
from oracle import densecases as dc, streamcases as sc  # noqa: E402

DEV = "cuda"
FILL = sc.FILL
GUARD = 64
WORST = {}


# ---- device operands ---------------------------------------------------------------------------------------------------------------------

class Buf:
    """a rows operand on the device: the whole buffer, the PT of its column slice, its layout"""

    def __init__(self, host_buf, C, P, c0, ctot):
        self.buf = host_buf.to(DEV)
        self.C, self.P, self.c0, self.ctot = C, P, c0, ctot
        self.pt = PT(self.buf[:, c0:c0 + C], P, ctot)

    @property
    def arg(self):
        return self.pt if self.P > 1 else self.pt.t

    def value(self):
        """sum of the planes, float64 on the host (lowest plane first)"""
        out = self.pt.plane(self.P - 1).double()
        for p in range(self.P - 2, -1, -1):
            out = out + self.pt.plane(p).double()
        return out.cpu()

    def outside_is_fill(self):
        m = torch.ones(self.buf.shape[1], dtype=torch.bool)
        for p in range(self.P):
            m[p * self.ctot + self.c0:p * self.ctot + self.c0 + self.C] = False
        if not bool(m.any()):
            return True
        return bool((self.buf[:, m.to(DEV)].float() == FILL).all())


def dev_in(v, fmt, P, sliced=True):
    buf, c0, ctot = sc.layout(v, fmt, P, sliced)
    return Buf(buf, v.shape[1], P, c0, ctot)


def dev_out(R, C, fmt, P):
    ctot = C + 16
    return Buf(torch.full((R, P * ctot), FILL, dtype=dc.DT[fmt]), C, P, 8, ctot)


def f32(t):
    return None if t is None else t.float().to(DEV)


def scalar(v):
    return None if v is None else torch.tensor([v], dtype=torch.float32, device=DEV)


def guarded(n):
    """n floats of scratch followed by a guard the kernels must not touch"""
    t = torch.full((n + GUARD,), -777.0, dtype=torch.float32, device=DEV)
    return t


def guard_ok(t, n):
    return bool((t[n:] == -777.0).all())


def fi(c):
    return 1 if c.fmt == "half" else 0


# ---- running a case ----------------------------------------------------------------------------------------------------------------------

def run(c, o, r):
    """launches the case; returns ({name: float64 rows output}, {name: fp32 vector output}, [Buf whose outside must be fill], extra checks passed)"""
    e, fmt = c.entry, c.fmt
    rows, vecs, outs, ok = {}, {}, [], True
    if e == "bn_apply":
        x, y = dev_in(o.x, fmt, c.pl("x")), dev_out(c.M, c.C, fmt, c.pl("y"))
        res = dev_in(o.res, fmt, c.pl("res")) if o.res is not None else None
        ops.bn_apply(x.arg, c.C, f32(o.scale), f32(o.shift), y.arg, res=res.arg if res else None, relu=c.relu)
        rows["y"], outs = y.value(), [y]
    elif e == "bn_frozen_scale":
        dy, dx = dev_in(o.dy, fmt, c.pl("dy")), dev_out(c.M, c.C, fmt, c.pl("y"))
        ops.bn_bwd_frozen(None, dy.arg, c.C, f32(o.scale), None, None, None, None, dx.arg)
        rows["dx"], outs = dx.value(), [dx]
    elif e == "add_rows":
        a, y = dev_in(o.a, fmt, c.pl("x")), dev_out(c.M, c.C, fmt, c.pl("y"))
        b = dev_in(o.b, fmt, c.pl("b")) if o.b is not None else None
        m = dev_in(o.mask, fmt, 1, sliced=False) if o.mask is not None else None          # (ldm = C: not the ld of a, b or y)
        ops.add_rows(a.arg, b.arg if b else None, y.arg, c.C, mask=m.pt.t if m else None, scale=(scalar(o.s1), scalar(o.s2)) if o.s1 is not None else None)
        rows["y"], outs = y.value(), [y]
    elif e in ("bn_bwd", "bn_frozen"):
        x, dy, dx = dev_in(o.x, fmt, c.pl("x")), dev_in(o.dy, fmt, c.pl("dy")), dev_out(c.M, c.C, fmt, c.pl("y"))
        n = c.get("scratch") or sc.default_scratch(c.C, True)
        scr = guarded(n)
        dg, db = (f32(o.dgamma0), f32(o.dbeta0)) if c.accumulate else (torch.full((c.C,), FILL, device=DEV), torch.full((c.C,), FILL, device=DEV))
        planes = ops.pl(a=x.arg, b=dy.arg, y=dx.arg)
        ga, mu, istd, sca, rme, rva = (f32(t) for t in (o.gamma, o.mean, o.invstd, o.scale, o.rmean, o.rvar))          # (alive until the synchronize)
        if e == "bn_bwd":
            part, nbp, rs = None, 0, None
            if c.get("parts"):
                part, nbp, rs = sc.host_partials(o, c, c.parts, 2.0 ** -3).to(DEV), c.parts, scalar(2.0 ** -3)
            _lib.call("kg_bn_bwd", ptr(x.pt.t), ops.ld(x.pt), ptr(dy.pt.t), ops.ld(dy.pt), ptr(ga), ptr(mu), ptr(istd), ptr(dg), ptr(db),
                      1 if c.accumulate else 0, ptr(dx.pt.t), ops.ld(dx.pt), c.M, c.C, ptr(scr), n, ptr(part), nbp, ptr(rs), planes, stream_ptr(), fmt=fi(c))
            torch.cuda.synchronize()
            vecs["coef"] = scr[:3 * c.C].view(3, c.C).cpu()
        else:
            _lib.call("kg_bn_bwd_frozen", ptr(x.pt.t), ops.ld(x.pt), ptr(dy.pt.t), ops.ld(dy.pt), ptr(sca), ptr(rme), ptr(rva),
                      c_float(1e-5), ptr(dg), ptr(db), 1 if c.accumulate else 0, ptr(dx.pt.t), ops.ld(dx.pt), c.M, c.C, ptr(scr), n, planes, stream_ptr(), fmt=fi(c))
        torch.cuda.synchronize()
        vecs["dgamma"], vecs["dbeta"] = dg.cpu(), db.cpu()
        rows["dx"], outs, ok = dx.value(), [dx], guard_ok(scr, n)
    elif e == "bn_stats":
        x = dev_in(o.x, fmt, c.pl("x"))
        n = c.get("scratch") or sc.default_scratch(c.C, False)
        scr = guarded(n)
        st = torch.full((4, c.C), FILL, dtype=torch.float32, device=DEV)
        rm, rv = (f32(o.rmean), f32(o.rvar)) if c.running else (None, None)
        ga, be = f32(o.gamma), f32(o.beta)
        _lib.call("kg_bn_stats_train", ptr(x.pt.t), ops.ld(x.pt), c.M, c.C, ptr(ga), ptr(be), ptr(rm), ptr(rv), c_float(0.1), c_float(1e-5),
                  ptr(st[0]), ptr(st[1]), ptr(st[2]), ptr(st[3]), ptr(scr), n, ops.pl(a=x.arg), stream_ptr(), fmt=fi(c))
        torch.cuda.synchronize()
        vecs = dict(zip(("mean", "invstd", "scale", "shift"), st.cpu()))
        if c.running:
            vecs["running_mean"], vecs["running_var"] = rm.cpu(), rv.cpu()
        outs, ok = [x], guard_ok(scr, n)
    elif e == "bn_finalize":
        rm, rv = (f32(o.rmean), f32(o.rvar)) if c.running else (None, None)
        st = ops.bn_finalize_train(o.part.to(DEV), c.nb, c.M, c.C, f32(o.gamma), f32(o.beta), rm, rv)
        vecs = dict(zip(("mean", "invstd", "scale", "shift"), [t.cpu() for t in st]))
        if c.running:
            vecs["running_mean"], vecs["running_var"] = rm.cpu(), rv.cpu()
    elif e == "maxpool":
        N, H, W, C = c.N, c.H, c.W, c.C
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        x, y = dev_in(sc.rows_of(o.x), fmt, c.pl("x")), dev_out(N * OH * OW, C, fmt, c.pl("x"))
        arg = torch.full((N * OH * OW, C), 77, dtype=torch.uint8, device=DEV)
        ops.maxpool_fwd(x.arg, y.arg, N, H, W, C, argmax=arg)
        dy = dev_in(sc.rows_of(o.dy), fmt, c.pl("dy"))
        dx1, dx2 = dev_out(N * H * W, C, fmt, c.pl("y")), dev_out(N * H * W, C, fmt, c.pl("y"))
        ops.maxpool_bwd(x.arg, dy.arg, dx1.arg, N, H, W, C, argmax=arg)
        ops.maxpool_bwd(x.arg, dy.arg, dx2.arg, N, H, W, C)
        torch.cuda.synchronize()
        rows["y"], rows["dx"], outs = y.value(), dx1.value(), [y, dx1, dx2]
        ok = torch.equal(dx1.buf.view(torch.int16), dx2.buf.view(torch.int16)) and torch.equal(arg.cpu(), r.arg)
    elif e == "bilinear_fwd":
        x, y = dev_in(sc.rows_of(o.x), fmt, c.pl("x")), dev_out(c.N * c.OH * c.OW, c.C, fmt, c.pl("y"))
        ops.bilinear_fwd(x.arg, y.arg, c.N, c.IH, c.IW, c.OH, c.OW, c.C)
        rows["y"], outs = y.value(), [y]
    elif e == "bilinear_bwd":
        dy, dx = dev_in(sc.rows_of(o.dy), fmt, c.pl("dy")), dev_out(c.N * c.IH * c.IW, c.C, fmt, c.pl("y"))
        m = dev_in(sc.rows_of(o.mask), fmt, 1, sliced=False) if o.mask is not None else None          # (ldmask = C)
        ops.bilinear_bwd(dy.arg, dx.arg, c.N, c.IH, c.IW, c.OH, c.OW, c.C, mask=m.pt.t if m else None)
        rows["dx"], outs = dx.value(), [dx]
    elif e == "img_pack":
        y = dev_out(c.N * c.H * c.W, 8, fmt, c.P)
        img = o.img.contiguous().to(DEV)
        _lib.call("kg_img_pack", ptr(img), ptr(y.pt.t), ops.ld(y.pt), c.N, c.C, c.H, c.W, ops.pl(y=y.arg), stream_ptr(), fmt=fi(c))
        rows["y"], outs = y.value(), [y]
        ok = bool((y.buf[:, [p * y.ctot + 8 + k for p in range(c.P) for k in range(c.C, 8)]].view(torch.int16) == 0).all()) if c.C < 8 else True
    else:
        raise ValueError(e)
    torch.cuda.synchronize()
    return rows, vecs, outs, ok


FAULT_WORDS = ("illegal memory access", "HSA_STATUS_ERROR", "Memory access fault", "unspecified launch failure", "hipErrorLaunchFailure")


def on_gpu(fn, *a):
    """runs the device part of a test; after a GPU fault nothing more is started on the device: the session ends there"""
    try:
        return fn(*a)
    except (RuntimeError, _lib.KGLibraryError) as exc:
        if any(w in str(exc) for w in FAULT_WORDS):
            pytest.exit(f"GPU fault, nothing more is run: {exc}", returncode=3)
        raise


def note(kernel, gpu, yard):
    w = WORST.setdefault(kernel, [0.0, 0.0])
    w[0], w[1] = max(w[0], gpu), max(w[1], yard)


PARITY = [c for c in sc.CASES if c.entry not in ("rescale", "rows_scale", "scale_multi")]
EXACT = [c for c in sc.CASES if c.entry in ("rescale", "rows_scale", "scale_multi")]


@pytest.mark.parametrize("case", PARITY, ids=lambda c: c.name)
def test_case(case):
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    o = sc.Operands(case)
    r = sc.Reference(case, o)
    rows, vecs, outs, ok = on_gpu(run, case, o, r)
    assert set(rows) == set(r.rows) and set(vecs) == set(r.vecs), (case, sorted(rows), sorted(vecs))
    msg = []
    for name, got in rows.items():
        out = r.rows[name]
        g, y = out.ratio(got), out.ratio(out.f32)
        note(f"{case.entry} {name}", g, y)
        msg.append(f"{name} GPU {g:.3f} (float32 {y:.3f}) allow {out.allow:.3g} u {out.u:.3g}")
    for name, got in vecs.items():
        v = r.vecs[name]
        g, y = v.ratio(got), v.ratio(v.f32)
        note(f"{case.entry} {name}", g, y)
        msg.append(f"{name} GPU {g:.3f} (float32 {y:.3f})")
    print(f"[{case.name}] worst |d| / bound: " + "; ".join(msg))
    for name, got in rows.items():
        assert r.rows[name].ratio(got) <= 1.0, (case, name, r.rows[name].ratio(got))
    for name, got in vecs.items():
        assert r.vecs[name].ratio(got) <= 1.0, (case, name, r.vecs[name].ratio(got))
    for b in outs:
        assert b.outside_is_fill(), (case, "columns outside the written slice changed")
    assert ok, (case, "guard words / argmax bytes / padding channels / the two backward routes differ")


def bits_equal(a, b):
    return torch.equal(a.view(torch.int16).cpu(), b.view(torch.int16))


@pytest.mark.parametrize("case", EXACT, ids=lambda c: c.name)
def test_exact_case(case):
    """the rescale family: the whole buffer, every plane and every column, bit for bit; r, cum_out and the scratch words"""
    o = sc.Operands(case)
    on_gpu(run_exact, case, o, sc.Reference(case, o))


def run_exact(case, o, r):
    c, fmt = case, case.fmt
    if c.entry == "rescale":
        g = dev_in(o.g, fmt, c.P)
        scr = torch.zeros(2 + GUARD, dtype=torch.int32, device=DEV)
        cum_in = torch.tensor(r.cum_in, dtype=torch.float32, device=DEV)
        out = torch.full((3 + GUARD,), FILL, dtype=torch.float32, device=DEV)
        _lib.call("kg_rows_rescale", ptr(g.pt.t), ops.ld(g.pt), ctypes.c_long(c.M), c.C, sc.T_LOG2, ptr(cum_in), ptr(out[0:2]), ptr(out[2:3]), ptr(scr),
                  ops.pl(a=g.arg), stream_ptr(), fmt=fi(c))
        torch.cuda.synchronize()
        got = {"cum": float(out[0]), "inv": float(out[1]), "r": float(out[2])}
        assert got == r.scalars, (case, got, r.scalars)
        assert bool((scr == 0).all()) and bool((out[3:] == FILL).all()), (case, "scratch not left zero / words behind the outputs written")
        assert bits_equal(g.buf, r.buffer), (case, "tensor differs from every plane times r")
    elif c.entry == "rows_scale":
        g = dev_in(o.g, fmt, c.P)
        ops.rows_scale(g.arg, c.C, scalar(o.s1), scalar(o.s2))
        torch.cuda.synchronize()
        assert bits_equal(g.buf, r.buffer), case
    else:
        gs = [dev_in(v, fmt, P, sliced) for v, (M, C, P, sliced) in zip(o.gs, c.items)]
        ops.rows_scale_multi([(g.arg, g.C) for g in gs], scalar(o.s1), scalar(o.s2))
        torch.cuda.synchronize()
        for k, (g, want) in enumerate(zip(gs, r.buffers)):
            assert bits_equal(g.buf, want), (case, "tensor", k)


def test_rescale_chain():
    """cum_out of one boundary is cum_in of the next: scale and 1 / scale multiply up exactly"""
    a = sc.BY_NAME["rescale M777 C64 max at mid half P2"]
    b = sc.BY_NAME["rescale M5000 C24 max at chunk0 half P2"]
    cum = torch.tensor([1.0, 1.0], dtype=torch.float32, device=DEV)
    want = 1.0
    for c in (a, b, a):
        o = sc.Operands(c)
        g = dev_in(o.g, c.fmt, c.P)
        rr, cum = ops.rows_rescale(g.arg, c.C, cum, sc.T_LOG2)
        ref = sc.Reference(c, o)
        want *= ref.scalars["r"]
        torch.cuda.synchronize()
        assert float(rr) == ref.scalars["r"] and cum.cpu().tolist() == [want, 1.0 / want], (c, float(rr), cum, want)
        assert bits_equal(g.buf, ref.buffer)
    assert want == 2.0 ** -18
    scr = ops._gs_state[str(g.buf.device)]
    assert bool((scr == 0).all())


def test_empty_inputs_return_ok_and_write_nothing():
    """M = 0 for the five entry points that document it: KG_OK (no exception), outputs untouched"""
    C = 24
    g = torch.Generator().manual_seed(3)
    for fmt, P in (("bf16", 2), ("half", 1)):
        a, b = dev_in(torch.randn(8, C, generator=g), fmt, P), dev_in(torch.randn(8, C, generator=g), fmt, P)
        y = dev_out(8, C, fmt, P)
        pl = ops.pl(a=a.arg, b=b.arg, y=y.arg)
        one = scalar(0.5)
        f = 1 if fmt == "half" else 0
        before_a = a.buf.clone()
        _lib.call("kg_add_rows", ptr(a.pt.t), ops.ld(a.pt), ptr(b.pt.t), ops.ld(b.pt), None, 0, ptr(y.pt.t), ops.ld(y.pt), ctypes.c_long(0), C, None, None, pl, stream_ptr(), fmt=f)
        pl2 = ops.pl(a=a.arg, y=y.arg)
        _lib.call("kg_bilinear_fwd", ptr(a.pt.t), ops.ld(a.pt), ptr(y.pt.t), ops.ld(y.pt), 0, 2, 2, 2, 2, C, None, None, ctypes.c_long(0), pl2, stream_ptr(), fmt=f)
        _lib.call("kg_bilinear_bwd", ptr(a.pt.t), ops.ld(a.pt), ptr(y.pt.t), ops.ld(y.pt), 0, 2, 2, 2, 2, C, None, None, ctypes.c_long(0), None, 0, pl2, stream_ptr(), fmt=f)
        out = torch.full((3,), FILL, dtype=torch.float32, device=DEV)
        scr = torch.zeros(2, dtype=torch.int32, device=DEV)
        cum = torch.tensor([1.0, 1.0], dtype=torch.float32, device=DEV)
        _lib.call("kg_rows_rescale", ptr(a.pt.t), ops.ld(a.pt), ctypes.c_long(0), C, 4, ptr(cum), ptr(out[0:2]), ptr(out[2:3]), ptr(scr), ops.pl(a=a.arg), stream_ptr(), fmt=f)
        _lib.call("kg_rows_scale", ptr(a.pt.t), ops.ld(a.pt), ctypes.c_long(0), C, ptr(one), None, ops.pl(a=a.arg), stream_ptr(), fmt=f)
        torch.cuda.synchronize()
        assert bool((y.buf.float() == FILL).all()) and bool((out == FILL).all()) and bool((scr == 0).all())
        assert bits_equal(a.buf, before_a.cpu())


def test_conditioning_30_sigma():
    """see CONDITIONING in the module docstring"""
    c = sc.CONDITIONING
    o = sc.Operands(c)
    x64 = o.x.double()
    mu, var = x64.mean(0), x64.var(0, unbiased=False)
    is64 = 1.0 / (var + sc.EPS32).sqrt()
    nb, rpb = sc.reduce_geometry(c.M, c.C, sc.default_scratch(c.C, False))
    m1, i1 = sc.onepass_f32(o.x, nb, rpb)
    x = dev_in(o.x, c.fmt, c.P)
    mean, invstd, _, _ = ops.bn_stats_train(x.arg, c.C, f32(o.gamma), f32(o.beta), None, None)
    torch.cuda.synchronize()
    e_mu, e_is = (mean.cpu().double() - mu).abs(), (invstd.cpu().double() - is64).abs()
    y_mu, y_is = (m1 - mu).abs(), (i1 - is64).abs()
    print(f"[conditioning] |mean| / sigma {float((mu.abs() / var.sqrt()).min()):.1f}; relative invstd error: kernel {float((e_is / is64).max()):.3g}, float32 one-pass "
          f"evaluation {float((y_is / is64).max()):.3g}; mean error: kernel {float(e_mu.max()):.3g}, evaluation {float(y_mu.max()):.3g}")
    assert float(e_is.max()) <= float((sc.U32 * is64).max()) + dc.MARGIN * float(y_is.max())
    assert float(e_mu.max()) <= float((sc.U32 * mu.abs()).max()) + dc.MARGIN * float(y_mu.max())


def test_worst_ratio_per_kernel():
    """(report) worst |d| / bound per kernel and output over the cases of this process: GPU (float32 CPU evaluation)"""
    for k, (g, y) in sorted(WORST.items()):
        print(f"[kernel {k}] GPU {g:.3f} (float32 {y:.3f})")
    assert all(g <= 1.0 for g, _ in WORST.values())
