"""Parity cases of the STEP TAIL: what runs after the last conv of a train step (TEST INFRASTRUCTURE, not product; imports no GPU library).

Covered here, each with (1) its launch geometry restated from the .hip host code, (2) a case table whose index paths are COMPUTED from (1) (`claims`),
(3) a float64 reference, (4) the float32 CPU evaluation of the same formula, (5) the bound and (6) the mutants the bound has to see:
    kg_scale_tensors, kg_adam_step        (gradscale.hip, optim.hip: a job table, 4096 elements per workgroup, 16-byte or scalar accesses per chunk)
    kg_grad_scale                         (gradscale.hip: a maximum of bit patterns over up to 24 tensors, at most 512 workgroups)
    kg_sigmoid_inplace                    (loss.hip: a grid-stride loop, at most 8192 workgroups)
    kg_wgrad_reduce / _multi / _bias      (conv_wgrad.hip reduce_shape, wgrad_reduce_body, and the deferred batch flush)
    kg_detection_loss_fwd / _bwd          (loss.hip: block partials, a one-wave final in double)
    kg_seg_loss                           (loss.hip: one workgroup per patch, pairs per patch)
    kg_bias_grad                          (conv_wgrad.hip: vector / scalar kernel, channel slabs, scratch-limited blocks, a 4-row unrolled loop)
    kg_grad_pack / kg_grad_pack3          (loss.hip: LDS-transpose kernels with a 2048-block cap, the per-pixel kernel)
    kg_pack_weight_batch                  (conv_igemm.hip: the job list and job -> block layout; the comparison is device against device)

Bounds.  No constant of its own: MARGIN (4), FLOOR (2e-6) and U_OUT come from densecases.
    exact    bit equality (scale_tensors: one IEEE multiply; grad_scale: a power of two; a reduction against its float32 evaluation in the restated ORDER,
             which only holds additions and is therefore reproducible on the host)
    product  |d| <= k * 2^-24 * |ref| per element, k = the fp32 roundings counted next to the formula; ref == 0 demands a zero (either sign)
    rows     2^-24 |ref| + max(MARGIN * worst |float32 evaluation - float64| over the group, FLOOR * rms(ref of the group)); a group is one job /
             one tensor / one planted value.  sigmoid adds 2^-126 (a result below the normal range may be flushed)
    sum      max(MARGIN * |float32 evaluation - float64|, FLOOR * sum |terms|)  (densecases.stats_reference), propagated linearly to what the final
             kernel derives; every fp32 rounding on the way adds 2^-24 of the rounded magnitude.
             BCE sums: the device logf / log1pf err by some ulps per term; that number is not guessed: it is MARGIN x the worst error, in ulps of the
             result, of the CPU float32 log / log1p against float64 over the case's own p values (`log_ulps`; measured: the CPU errs by 0.53 .. 0.62
             ulp, so the term is 2.13 .. 2.49 ulps = that many times 2^-23 |term| per term).
Nothing is fitted to a kernel's output."""
import math

import numpy as np
import torch

from .densecases import FLOOR, MARGIN, U_OUT, cdiv

U32 = U_OUT["f32"]
INF = float("inf")
FILL = 9.0
TINY = 2.0 ** -126
F32, F64 = torch.float32, torch.float64


class Case:
    def __init__(self, entry, name, **kw):
        self.entry, self.opt = entry, kw
        self.name = f"{entry} {name}"
        self.seed = sum((i + 1) * ord(ch) for i, ch in enumerate(self.name)) % (2 ** 31)

    def __getattr__(self, k):
        try:
            return self.__dict__["opt"][k]
        except KeyError:
            raise AttributeError(k)

    def get(self, k, default=None):
        return self.opt.get(k, default)

    def __repr__(self):
        return f"Case({self.name})"


def f32r(v):
    """a Python float rounded to fp32, as a C `float` argument of the ABI arrives"""
    return float(np.float32(v))


def ratio(d, b):
    """worst |d| / bound (inf where the bound is 0 and the element differs)"""
    d = d.abs().double()
    if d.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(d).all()):
        return INF
    b = torch.as_tensor(b, dtype=F64).expand_as(d)
    r = torch.where(b > 0, d / b.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, INF), torch.zeros_like(d)))
    return float(r.max())


def rows_bound(ref, f32, extra=0.0):
    """the rows bound of one group: [like ref] float64"""
    yard = float((f32.double() - ref).abs().max()) if ref.numel() else 0.0
    rms = float(ref.pow(2).mean().sqrt()) if ref.numel() else 0.0
    return U32 * ref.abs() + max(MARGIN * yard, FLOOR * rms) + extra


def sum_allow(s64, s32, terms_abs_sum):
    return torch.maximum(MARGIN * (s32.double() - s64).abs(), FLOOR * terms_abs_sum)


def bits(t):
    return t.contiguous().view(torch.int32)


# ==== job tables: kg_scale_tensors, kg_adam_step =================================================================================================
JOB_ELEMS, JOB_THREADS, JOB_UNROLL = 4096, 256, 4          # a workgroup: `base = (blockIdx.x - blk0) * 4096`, `i = base + (u * 256 + threadIdx.x) * 4`, u < 4


def job_layout(ns):
    """blk0 of every job and the block total, as ops.scale_tensors / optim.Adam lay them out: `blk += (n + 4095) // 4096`"""
    blk0, b = [], 0
    for n in ns:
        blk0.append(b)
        b += cdiv(n, JOB_ELEMS)
    return blk0, b


def job_search(blk0, b):
    """the kernels' binary search: the LAST job whose blk0 <= b (a zero-length job shares its blk0 with its successor and is never found).
    Returns (job, probes)"""
    lo, hi, probes = 0, len(blk0) - 1, 0
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        probes += 1
        if blk0[mid] <= b:
            lo = mid
        else:
            hi = mid - 1
    return lo, probes


def job_paths(n, offs):
    """index paths of one job: n elements, offs = the misalignment (in floats, from 16 bytes) of each of its pointers"""
    aligned = all(o % 4 == 0 for o in offs)
    p = set()
    if n == 0:
        return {"empty job"}
    if aligned and n >= 4:
        p.add("vector")
    if aligned and n % 4:
        p.add("scalar tail")                       # `i + 4 <= n` fails for the last chunk
    if not aligned:
        p.add("scalar unaligned")                  # `(p + i) & 15` fails for EVERY chunk (i is a multiple of 4)
    if n % JOB_ELEMS:
        p.add("idle chunks")                       # `if (i >= n) continue`
    else:
        p.add("full last block")
    if n > JOB_ELEMS:
        p.add("several blocks")
    if (n - 1) % JOB_ELEMS >= JOB_THREADS * 4:
        p.add("last block unroll > 0")
    return p


def table_claims(jobs):
    """jobs: [(n, offs)]"""
    blk0, total = job_layout([n for n, _ in jobs])
    found = [job_search(blk0, b) for b in range(total)]
    live = [j for j, (n, _) in enumerate(jobs) if n > 0]
    assert sorted({j for j, _ in found}) == live, "the search must reach every non-empty job and no empty one"
    for b, (j, _) in enumerate(found):
        assert blk0[j] <= b < blk0[j] + cdiv(jobs[j][0], JOB_ELEMS)
    paths = set()
    for n, offs in jobs:
        paths |= job_paths(n, offs)
    return {"njobs": len(jobs), "blocks": total, "probes": max([p for _, p in found] or [0]), "paths": paths}


JOB_NS = (1, 3, 4095, 4096, 4097, 12289)
SCALES = (0.25, 3.0, 2.0 ** -7, 1.7, 0.75, 8.0)


def _table(njobs, empty_at=None):
    """(n, misalignment, scale index) per job: sizes and alignments cycle through the issue's table"""
    out = []
    for j in range(njobs):
        n = 0 if j == empty_at else JOB_NS[(j * 5 + 2) % 6] if njobs > 1 else 4097
        out.append((n, (j + (njobs > 1)) % 4, j % len(SCALES)))
    return out


SCALE_CASES = [Case("scale_tensors", f"{k} jobs", jobs=_table(k, empty_at=11 if k == 37 else None), flag="given", plant=None) for k in (1, 2, 3, 37)]
SCALE_CASES.append(Case("scale_tensors", "6 sizes aligned", jobs=[(n, 0, j) for j, n in enumerate(JOB_NS)], flag="given", plant=None))
# flag cases: (job, element) of a 3-job table {4097 aligned, 4096 unaligned, 1030 aligned}; what is planted there
for _name, _plant in (("inf", (0, 2000, "inf")), ("nan", (1, 17, "nan")), ("finite overflow", (2, 512, "big")), ("tail element alone", (0, 4096, "inf")),
                      ("last wave alone", (2, 1022, "nan")), ("null flag", (0, 5, "inf")), ("large but finite", (1, 4095, "edge"))):
    SCALE_CASES.append(Case("scale_tensors", "flag " + _name, jobs=[(4097, 0, 1), (4096, 1, 3), (1030, 0, 5)], flag="null" if _name == "null flag" else "given",
                            plant=_plant))


def scale_operands(c):
    g = torch.Generator().manual_seed(c.seed)
    xs = []
    for j, (n, off, si) in enumerate(c.jobs):
        e = torch.randint(-20, 21, (n,), generator=g).float()
        x = (1 + torch.rand(n, generator=g)) * torch.exp2(e) * (2 * torch.randint(0, 2, (n,), generator=g).float() - 1)   # normal, results normal
        xs.append(x)
    if c.plant:
        j, k, what = c.plant
        xs[j][k] = {"inf": INF, "nan": float("nan"), "big": 3e38, "edge": 3.39e38 / SCALES[c.jobs[j][2]]}[what]
    return xs


def scale_reference(c, xs):
    """(expected tensors, expected flag): one IEEE fp32 multiply per element; the flag is `!(fabsf(v) <= 3.4e38f)` of any result"""
    want = [x * torch.tensor(SCALES[si], dtype=F32) for x, (n, off, si) in zip(xs, c.jobs)]
    lim = torch.tensor(3.4e38, dtype=F32)
    flag = int(any(bool((~(w.abs() <= lim)).any()) for w in want))
    return want, flag


def same_bits(a, b):
    """bit equality; a NaN matches any NaN"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool((na == nb).all()) and bool((bits(a)[~na] == bits(b)[~nb]).all())


def chunk_mutants(want, before, seed):
    """one 16-byte chunk left unwritten (it keeps `before`), one chunk that holds its neighbour's result: [(kind, lo, hi, values)] of a flat tensor"""
    n = want.numel()
    if n == 0:
        return []
    g = torch.Generator().manual_seed(seed + 17)
    nch = cdiv(n, 4)
    c0 = int(torch.randint(0, nch, (1,), generator=g))
    muts = [("unwritten", 4 * c0, min(4 * c0 + 4, n), before[4 * c0:4 * c0 + 4].clone())]
    for k in range(min(nch, 4096)):
        cc = (c0 + k) % nch
        nbc = cc + 1 if 4 * (cc + 1) + 4 <= n else cc - 1
        lo, hi = 4 * cc, min(4 * cc + 4, n)
        if nbc >= 0 and hi - lo == 4 and not torch.equal(want[lo:hi], want[4 * nbc:4 * nbc + 4]):
            muts.append(("neighbour", lo, hi, want[4 * nbc:4 * nbc + 4].clone()))
            break
    return muts


# ---- Adam ---------------------------------------------------------------------------------------------------------------------------------------
GMAGS = (0.0, 1e-8, 1.0, 1e4)
ADAM_HYPER = dict(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8)


def adam_scalars(lr, beta1, beta2, eps, wd, t):
    """the six floats kg_adam_step receives (optim.Adam.step: bias corrections in double, rounded to fp32 by ctypes)"""
    return dict(beta1=f32r(beta1), beta2=f32r(beta2), eps=f32r(eps), step=f32r(lr / (1.0 - beta1 ** t)), bc2s=f32r(math.sqrt(1.0 - beta2 ** t)), wd=f32r(wd))


def adam_eval(p, g, m, v, s, dt):
    """adam_step_kernel's expression, operation by operation (optim.hip is built with -ffp-contract=off): dt = float32 is the yardstick, float64 the
    reference.  Returns (m', v', step * m' / denom, p')"""
    T = lambda x: torch.tensor(x, dtype=dt)
    one = T(1.0)
    P, G, M, V = p.to(dt), g.to(dt), m.to(dt), v.to(dt)
    ge = G + T(s["wd"]) * P if s["wd"] != 0.0 else G
    m2 = M + (one - T(s["beta1"])) * (ge - M)
    v2 = V * T(s["beta2"]) + ((one - T(s["beta2"])) * ge) * ge
    denom = v2.sqrt() / T(s["bc2s"]) + T(s["eps"])
    upd = T(s["step"]) * (m2 / denom)
    return m2, v2, upd, P - upd


ADAM_CASES = []
for _wd in (0.0, 0.01):
    for _t in (1, 3):
        for _k in (1, 2, 3, 37):
            ADAM_CASES.append(Case("adam", f"{_k} jobs t{_t} wd{_wd}", t=_t, wd=_wd,
                                   jobs=[(n, (off,) * 4, GMAGS[(j + _k) % 4]) for j, (n, off, _) in enumerate(_table(_k))]))
        for _i, _which in enumerate("pgmv"):
            ADAM_CASES.append(Case("adam", f"unaligned {_which} t{_t} wd{_wd}", t=_t, wd=_wd,
                                   jobs=[(4097, tuple(1 + _i % 3 if q == _i else 0 for q in range(4)), 1.0), (4096, (0, 0, 0, 0), 1e-8)]))


def adam_operands(c):
    """per job (p, g, m, v) fp32.  |p| ~ 0.01 keeps the last rounding of p (2^-24 |p|) far below the update (~1e-4)."""
    g_ = torch.Generator().manual_seed(c.seed)
    out = []
    for n, offs, gmag in c.jobs:
        sgn = lambda: 2 * torch.randint(0, 2, (n,), generator=g_).float() - 1
        p = 0.01 * torch.randn(n, generator=g_)
        g = gmag * sgn() * (0.05 + torch.randn(n, generator=g_).abs())
        if c.t == 1:
            m, v = torch.zeros(n), torch.zeros(n)
        else:
            mag = gmag if gmag else 1.0
            m = 0.2 * mag * sgn() * (0.05 + torch.randn(n, generator=g_).abs())
            v = 0.002 * mag * mag * (0.05 + torch.rand(n, generator=g_))
        out.append((p, g, m, v))
    return out


class AdamReference:
    """per job: float64 m', v', update = p' - p, with the rows bound of each (one job = one group); p' gets 2^-24 |p'| on top"""

    def __init__(self, c, ops_=None, scalars=None):
        self.c = c
        self.ops = ops_ or adam_operands(c)
        self.s = scalars or adam_scalars(wd=c.wd, t=c.t, **ADAM_HYPER)
        self.jobs = []
        for p, g, m, v in self.ops:
            m64, v64, u64, p64 = adam_eval(p, g, m, v, self.s, F64)
            m32, v32, u32, p32 = adam_eval(p, g, m, v, self.s, F32)
            self.jobs.append({"m": (m64, m32, rows_bound(m64, m32)), "v": (v64, v32, rows_bound(v64, v32)),
                              "update": (-u64, p32.double() - p.double(), rows_bound(-u64, -u32) + U32 * p64.abs()), "p32": p32})

    def job_ratio(self, j, p_new, m_new, v_new, names=("m", "v", "update")):
        """{name: worst |d| / bound}; the update is formed in float64 from the fp32 parameters before and after"""
        p_old = self.ops[j][0]
        got = {"m": m_new.double(), "v": v_new.double(), "update": p_new.double() - p_old.double()}
        return {k: ratio(got[k] - self.jobs[j][k][0], self.jobs[j][k][2]) for k in names}

    def yardstick(self, j):
        return {k: ratio(self.jobs[j][k][1].double() - self.jobs[j][k][0], self.jobs[j][k][2]) for k in ("m", "v", "update")}


# ==== kg_grad_scale ================================================================================================================================
GS_THREADS, GS_PER_BLOCK, GS_CAP = 1024, 1024 * 16, 512
GS_TARGET = 4


def gs_blocks(total):
    """`blocks = (total + 1024 * 16 - 1) / (1024 * 16)`, at least 1, at most 512"""
    return max(1, min(GS_CAP, cdiv(total, GS_PER_BLOCK)))


def gs_reader(n, vec, blocks, k):
    """which loop of grad_scale_kernel reads element k of an n-element tensor, and on which grid-stride trip: ("vector" | "scalar", trip)"""
    n4 = n >> 2 if vec else 0
    stride = blocks * GS_THREADS
    if k < 4 * n4:
        return "vector", (k // 4) // stride
    return "scalar", (k - 4 * n4) // stride


def gs_claims(c):
    total = sum(n for n, *_ in c.tensors)
    blocks = gs_blocks(total)
    d = {"ntensors": len(c.tensors), "blocks": blocks, "cap": cdiv(total, GS_PER_BLOCK) > GS_CAP, "paths": set(), "empty tensor": any(n == 0 for n, *_ in c.tensors)}
    for n, poff, hasq, qoff in c.tensors:
        vec = poff % 4 == 0 and (not hasq or qoff % 4 == 0)
        if n:
            d["paths"].add("vector" if vec and n >= 4 else "scalar")
            if vec and n % 4:
                d["paths"].add("tail")
            if not vec:
                d["paths"].add("unaligned " + ("p" if poff % 4 else "q"))
    if c.get("plant") is not None:
        t, k = c.plant
        n, poff, hasq, qoff = c.tensors[t]
        vec = poff % 4 == 0 and (not hasq or qoff % 4 == 0)
        loop, trip = gs_reader(n, vec, blocks, k)
        d.update(plant_loop=loop, plant_trip=trip, plant_tensor=t, plant_last_tensor=t == len(c.tensors) - 1, plant_tail=vec and k >= 4 * (n >> 2),
                 plant_last=k == n - 1, plant_first=k == 0 and t == 0)
    return d


GS_BIG = (8_400_003, 100_001)            # 8 500 004 floats > 512 x 16384 = 8 388 608: the cap, five or more vector trips per thread
GS_CASES = [
    Case("grad_scale", "1 tensor n1000 max at element 0", tensors=[(1000, 0, False, 0)], plant=(0, 0), value="big"),
    Case("grad_scale", "1 tensor n1003 max at the last tail element", tensors=[(1003, 0, False, 0)], plant=(0, 1002), value="big"),
    Case("grad_scale", "1 tensor n1003 with q max at the last tail element", tensors=[(1003, 0, True, 0)], plant=(0, 1002), value="big"),
    Case("grad_scale", "3 tensors max in the last", tensors=[(4845, 0, True, 0), (3230, 0, False, 0), (12920, 0, False, 0)], plant=(2, 7001), value="big"),
    Case("grad_scale", "3 tensors negative max", tensors=[(4845, 0, True, 0), (3230, 0, False, 0), (12920, 0, False, 0)], plant=(1, 3229), value="negative"),
    Case("grad_scale", "24 tensors one empty max in the last", tensors=[(0 if j == 7 else 300 + 37 * j, 0, j % 3 == 0, 0) for j in range(24)], plant=(23, 1150), value="big"),
    Case("grad_scale", "4 blocks max on a later trip", tensors=[(50_003, 0, False, 0)], plant=(0, 4 * 4096 + 5), value="big"),
    Case("grad_scale", "4 blocks max in the tail", tensors=[(50_003, 0, True, 0)], plant=(0, 50_002), value="big"),
    Case("grad_scale", "p unaligned", tensors=[(5001, 1, False, 0)], plant=(0, 5000), value="big"),
    Case("grad_scale", "q unaligned", tensors=[(5001, 0, True, 1), (999, 0, False, 0)], plant=(0, 4099), value="big"),
    Case("grad_scale", "p unaligned 3 blocks second scalar trip", tensors=[(40_000, 3, False, 0)], plant=(0, 3 * 1024 + 7), value="big"),
    Case("grad_scale", "cap max at element 0", tensors=[(n, 0, False, 0) for n in GS_BIG], plant=(0, 0), value="big"),
    Case("grad_scale", "cap max at the last tail element", tensors=[(n, 0, False, 0) for n in GS_BIG], plant=(0, GS_BIG[0] - 1), value="big"),
    Case("grad_scale", "cap max in the last tensor", tensors=[(n, 0, False, 0) for n in GS_BIG], plant=(1, GS_BIG[1] - 1), value="negative"),
    Case("grad_scale", "cap max on the last trip", tensors=[(n, 0, False, 0) for n in GS_BIG], plant=(0, 4 * 4 * GS_CAP * GS_THREADS + 4 * 77 + 2), value="big"),
]
for _v in ("1e-38", "3e38", "inf", "nan", "zero"):
    GS_CASES.append(Case("grad_scale", "clamp " + _v, tensors=[(1003, 0, False, 0)], plant=(0, 501), value=_v))


def gs_operands(c):
    """[(p, q or None)]: background |p| in [1e-7, 2e-6) (q in (0.05, 0.95): the product is smaller still); the planted value is 1.25 * 2^-12 -- and
    where the tensor has a q, q = 0.5 there, so that p q (1 - q) = p / 4 exactly: float32 and float64 agree on the binade of the maximum by construction
    (tests/test_tail_cases_cpu.py asserts it for every case)"""
    g = torch.Generator().manual_seed(c.seed)
    out = []
    for n, poff, hasq, qoff in c.tensors:
        p = (1e-7 + 1.9e-6 * torch.rand(n, generator=g)) * (2 * torch.randint(0, 2, (n,), generator=g).float() - 1)
        q = 0.05 + 0.9 * torch.rand(n, generator=g) if hasq else None
        if c.value in ("1e-38", "zero"):
            p.zero_()
        out.append((p, q))
    t, k = c.plant
    val = {"big": 1.25 * 2.0 ** -12, "negative": -1.25 * 2.0 ** -12, "1e-38": 1e-38, "3e38": 3e38, "inf": INF, "nan": float("nan"), "zero": 0.0}[c.value]
    out[t][0][k] = val
    if out[t][1] is not None:
        out[t][1][k] = 0.5
    return out


def gs_max(tensors, dt, skip=None):
    """max |p * (q * (1 - q))| in dtype dt (the kernel's `v *= s * (1.f - s)`); NaN -> NaN, skip = (tensor, element) left out"""
    best = 0.0
    for t, (p, q) in enumerate(tensors):
        v = p.to(dt)
        if q is not None:
            v = v * (q.to(dt) * (1 - q.to(dt)))
        v = v.abs()
        if skip is not None and skip[0] == t:
            v = v.clone()
            v[skip[1]] = 0
        if v.numel():
            if bool(torch.isnan(v).any()):
                return float("nan")
            best = max(best, float(v.max()))
    return best


def gs_scale(m, target=GS_TARGET):
    """S = 2^clamp(target - e, -100, 100) with m = f 2^e, f in [0.5, 1); 1 for a zero, infinite or NaN maximum"""
    if m == 0.0 or not math.isfinite(m):
        return 1.0
    e = math.frexp(m)[1]
    return 2.0 ** max(-100, min(100, target - e))


# ==== kg_sigmoid_inplace ===========================================================================================================================
SIG_THREADS, SIG_CAP = 256, 8192
SUBNORMAL = 2.0 ** -140
SIG_SPECIALS = (0.0, -0.0, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0, SUBNORMAL, -SUBNORMAL)
SIG_CASES = [Case("sigmoid", f"n{n}", n=n) for n in (1, 255, SIG_CAP * SIG_THREADS + 1)] + [Case("sigmoid", "n10 specials only", n=10)]


def sig_claims(c):
    blocks = min(cdiv(c.n, SIG_THREADS), SIG_CAP)
    return {"blocks": blocks, "wraps": c.n > blocks * SIG_THREADS, "ragged": c.n % SIG_THREADS != 0, "specials": c.n >= len(SIG_SPECIALS)}


def sig_operands(c):
    """logits ~ N(0, 3); the special values are the LAST elements (in the large case the very last one is read on the second trip)"""
    g = torch.Generator().manual_seed(c.seed)
    x = 3.0 * torch.randn(c.n, generator=g)
    k = len(SIG_SPECIALS)
    if c.n >= k:
        x[c.n - k:] = torch.tensor(SIG_SPECIALS, dtype=F32)
    return x


class SigReference:
    """groups: the random body, and every special value by itself (its own magnitude: the rows bound is then relative to it)"""

    def __init__(self, c, x=None):
        self.x = sig_operands(c) if x is None else x
        ev = lambda dt: 1.0 / (1.0 + torch.exp(-self.x.to(dt)))
        self.ref, self.f32 = ev(F64), ev(F32)
        nsp = len(SIG_SPECIALS) if c.n >= len(SIG_SPECIALS) else 0
        body = c.n - nsp
        self.bound = torch.empty(c.n, dtype=F64)
        self.bound[:body] = rows_bound(self.ref[:body], self.f32[:body], TINY)
        for i in range(body, c.n):
            self.bound[i:i + 1] = rows_bound(self.ref[i:i + 1], self.f32[i:i + 1], TINY)

    def ratio(self, got, lo=0, hi=None):
        hi = self.ref.numel() if hi is None else hi
        return ratio(got.double() - self.ref[lo:hi], self.bound[lo:hi])


# ==== split weight-gradient reductions (conv_wgrad.hip) =============================================================================================
REDUCE_BATCH = 12


def reduce_shape(cout, cin, taps, S, bias_C=0):
    """reduce_shape + what wgrad_reduce_body derives from the launch: CH, threads, grid, thread groups G, the split range of every group"""
    if cout * cdiv(cin, 64) >= 2048:
        ch, nt = 64, 256
    else:
        ch, nt = 16, 256
        E = taps * 16
        if 2 * E <= 1024 and S >= 16:
            G = min(1024 // E, S // 8)
            if G >= 2:
                nt = E * G
    nw = nt >> 6
    E = taps * ch
    G = nt // E if nt >= 2 * E else 1          # (the KERNEL's G: with 1 tap it is 16 (CH = 16) or 4 (CH = 64) whatever the host chose)
    Sg = cdiv(S, G)
    ranges = [(g * Sg, min(g * Sg + Sg, S)) for g in range(G)]
    gx = cout + (cdiv(bias_C, nw) if bias_C else 0)
    return {"ch": ch, "nt": nt, "nw": nw, "gx": gx, "gy": cdiv(cin, ch), "G": G, "Sg": Sg, "ranges": ranges, "E": E}


def red_claims(c):
    cout = sum(c.counts)
    r = reduce_shape(cout, c.cin, c.taps, c.S, c.get("bias_C", 0))
    lens = [max(0, k1 - k0) for k0, k1 in r["ranges"]]
    return {"route": f"ch{r['ch']}", "taps": c.taps, "G": r["G"], "G>1": r["G"] > 1, "nt": r["nt"], "nt%64": r["nt"] % 64 != 0, "unroll8": any(n >= 8 for n in lens),
            "tail": any(n % 8 for n in lens), "empty last group": lens[-1] == 0, "S%G": c.S % r["G"] != 0, "part chunk": c.cin % r["ch"] != 0,
            "outputs": len(c.counts), "bias": bool(c.get("bias_C")), "bias_C%nw": bool(c.get("bias_C")) and c.bias_C % r["nw"] != 0,
            "e strides": r["G"] == 1 and r["E"] > r["nt"], "blocks": r["gx"] * r["gy"]}


def _red(name, cin, taps, S, counts, bias_C=0):
    return Case("wgrad_reduce", name, cin=cin, taps=taps, S=S, counts=list(counts), bias_C=bias_C)


RED_CASES = [
    _red("ch64 2048x24 1 tap S8", 24, 1, 8, [2048]),
    _red("ch64 2048x24 1 tap S3 (empty group)", 24, 1, 3, [2048]),
    _red("ch64 1024x65 9 taps S3", 65, 9, 3, [1024]),
    _red("ch16 one group 9 taps S7", 24, 9, 7, [16, 8]),
    _red("ch16 one group 9 taps S1", 64, 9, 1, [5]),
    _red("ch16 one group 9 taps S15", 40, 9, 15, [5, 10, 40]),
] + [_red(f"ch16 9 taps S{S}", 24, 9, S, [16], bias_C=bc) for S, bc in ((16, 0), (17, 16), (56, 0), (57, 16))] + [
    _red("ch16 9 taps S57 bias_C 21 four outputs", 72, 9, 57, [5, 10, 4, 2], bias_C=21),
    _red("ch16 9 taps S8 bias_C 6", 24, 9, 8, [6], bias_C=6),
    _red("ch16 25 taps S16", 24, 25, 16, [8, 8]),
    _red("ch16 25 taps S19", 20, 25, 19, [7]),
    _red("ch16 49 taps S9", 40, 49, 9, [5, 10, 40], bias_C=55),
    _red("ch16 49 taps S40", 32, 49, 40, [16, 16, 16]),
    _red("ch64 49 taps 256x449 S1", 449, 49, 1, [200, 56]),
    _red("ch16 1 tap S7", 24, 1, 7, [16, 8]),
    _red("ch16 1 tap S9", 70, 1, 9, [33]),
    _red("ch16 1 tap S17 (32 threads)", 24, 1, 17, [16]),
    _red("ch16 1 tap S64", 24, 1, 64, [16, 8]),
    _red("ch16 1 tap S300", 24, 1, 300, [16, 8, 4]),
]
# kg_wgrad_reduce_bias must refuse this one WITHOUT launching (reduce_shape would divide by nt / 64 == 0): 1 tap, CH = 16, 16 <= S < 32, bias partials
REFUSED = [dict(cin=24, taps=1, S=S, counts=[16], bias_C=16) for S in (16, 23, 24, 31)]


def red_operands(c):
    g = torch.Generator().manual_seed(c.seed)
    cout = sum(c.counts)
    part = torch.randn(c.S, cout, c.taps, c.cin, generator=g)
    prior = torch.randn(cout, c.cin, c.taps, generator=g)
    bpart = torch.randn(c.S, c.bias_C, generator=g) if c.bias_C else None
    bprior = torch.randn(c.bias_C, generator=g) if c.bias_C else None
    return part, prior, bpart, bprior


def red_f32(part, ranges, order=None):
    """the kernel's own float32 summation: every group adds its splits in order from 0.f, group 0 then adds the group sums in group order.
    Additions only: bit-reproducible on the host.  [cout, taps, cin]"""
    sums = []
    for k0, k1 in ranges:
        s = torch.zeros_like(part[0])
        for k in range(k0, k1):
            s = s + part[k]
        sums.append(s)
    order = list(range(len(sums))) if order is None else order
    tot = sums[order[0]]
    for q in order[1:]:
        tot = tot + sums[q]
    return tot


def bias_f32(bpart):
    """the bias column: lane l adds the splits l, l + 64, ... from 0.f; then the shfl_down tree 32, 16, .., 1.  [bias_C]"""
    S, C = bpart.shape
    v = torch.zeros(64, C)
    for b0 in range(0, S, 64):
        blk = bpart[b0:b0 + 64]
        v[:blk.shape[0]] = v[:blk.shape[0]] + blk
    o = 32
    while o:
        v = v[:o] + v[o:2 * o]
        o >>= 1
    return v[0]


class RedReference:
    """w: [cout, cin, taps] (the OIHW gradient), b: [bias_C]; each as (float64, float32-in-order, sum bound) for accumulate 0, and with the prior
    value added (one more rounding: + 2^-24 |result|) for accumulate 1"""

    def __init__(self, c, ops_=None):
        self.c = c
        self.part, self.prior, self.bpart, self.bprior = ops_ or red_operands(c)
        self.shape = reduce_shape(sum(c.counts), c.cin, c.taps, c.S, c.bias_C)
        p64 = self.part.double()
        self.w64 = p64.sum(0).permute(0, 2, 1).contiguous()
        self.w32 = red_f32(self.part, self.shape["ranges"]).permute(0, 2, 1).contiguous()
        self.wb = sum_allow(self.w64, self.w32, p64.abs().sum(0).permute(0, 2, 1))
        if c.bias_C:
            b64 = self.bpart.double()
            self.b64, self.b32 = b64.sum(0), bias_f32(self.bpart)
            self.bb = sum_allow(self.b64, self.b32, b64.abs().sum(0))

    def expect(self, acc):
        """{name: (float64, float32 in order, bound)}"""
        out = {}
        for name, r64, r32, b, prior in (("w", self.w64, self.w32, self.wb, self.prior),) + ((("b", self.b64, self.b32, self.bb, self.bprior),) if self.c.bias_C else ()):
            if acc:
                out[name] = (prior.double() + r64, prior + r32, b + U32 * (prior.double() + r64).abs())
            else:
                out[name] = (r64, r32, b)
        return out

    def mutants(self):
        """{kind: float32 [cout, cin, taps]}: one split dropped (the last of group 0, the last of all); group 1 summing group 0's range; the group
        sums added in reverse order (visible only to the bit comparison, and only with three or more groups)"""
        rg = self.shape["ranges"]
        m = {}
        for k in sorted({rg[0][1] - 1, self.c.S - 1}):
            keep = [i for i in range(self.c.S) if i != k]
            m[f"split {k} dropped"] = self.part[keep].double().sum(0).permute(0, 2, 1).float()
        live = [r for r in rg if r[1] > r[0]]
        if len(live) >= 2:
            m["range overlap"] = red_f32(self.part, [live[0], live[0]] + live[2:]).permute(0, 2, 1)
        if len(live) >= 3:
            m["reverse order"] = red_f32(self.part, live, order=list(range(len(live)))[::-1]).permute(0, 2, 1)
        return m


def defer_jobs():
    """the jobs of the deferred-flush test: every reduction case twice (accumulate 0, then 1): 44 jobs, both queues, several batches of 12 in each,
    1008-thread jobs next to 256-thread jobs"""
    return [(c, acc) for acc in (0, 1) for c in RED_CASES]


def batch_layout(jobs):
    """kg_wgrad_reduce_flush restated: per queue (CH = 16 first, then CH = 64) batches of 12 jobs in recording order: [(ch, threads, [(job index, blk0)])]"""
    out = []
    for ch in (16, 64):
        q = [(i, reduce_shape(sum(c.counts), c.cin, c.taps, c.S, c.bias_C)) for i, (c, _) in enumerate(jobs)]
        q = [(i, r) for i, r in q if r["ch"] == ch]
        for i0 in range(0, len(q), REDUCE_BATCH):
            blk, nt, lay = 0, 64, []
            for i, r in q[i0:i0 + REDUCE_BATCH]:
                lay.append((i, blk))
                blk += r["gx"] * r["gy"]
                nt = max(nt, r["nt"])
            out.append((ch, cdiv(nt, 64) * 64, lay))
    return out


# ==== kg_detection_loss_fwd / _bwd (loss.hip) ========================================================================================================
DET_THREADS, DET_FWD_CAP, DET_BWD_CAP, DET_SCRATCH = 256, 1024, 4096, 5 * 1024          # loss.py passes ops.scratch_f32(5 * 1024)
MID_FROM = (0, 0, 0, 0, 1, 1, 1, 2, 2, 3, 1, 2, 3, 4, 2, 3, 4, 3, 4, 4)                # config.py:2-13, KG_MID_FROM
KP_RADIUS = 5.0
EPS_DEN = f32r(1e-10)
CLAMP_D = f32r(1e-12)
K_GKP, K_GSH, K_GMD = 7, 7, 8
# fp32 roundings of the backward's expressions (product bound), mask sums exact or overridden:
#   g_kp = ((p - t) / max((1 - p) * p, 1e-12)) * (go * fin4): 1 - p, * p, p - t, /, fin4 = (float)(1 / ne), go * fin4, the last *          = 7
#   g_sh = sign * m * ((go * fin5) * inv_r): fin5 = 1.f / (m2 + 1e-10f) (+, /), inv_r = 1.f / radius, go * fin5, * inv_r, the last *, and
#          (float)m2 where the mask sum is not an integer below 2^24                                                                   = 7
#   g_md = sign * m * (((go * 0.25f) * fin6) * inv_r): the same with one more product                                                 = 8


def det_geometry(N, H, W, scratch_floats=DET_SCRATCH):
    total = N * H * W
    nb = min(cdiv(total, DET_THREADS), DET_FWD_CAP, scratch_floats // 5)
    nbb = min(cdiv(total, DET_THREADS), DET_BWD_CAP)
    trips = cdiv(total, nb * DET_THREADS)
    return {"total": total, "nb": nb, "trips": trips, "bwd_blocks": nbb, "bwd_trips": cdiv(total, nbb * DET_THREADS)}


def det_claims(c):
    g = det_geometry(c.N, c.H, c.W, c.get("scratch", DET_SCRATCH))
    total, HW = g["total"], c.H * c.W
    return dict(g, single_block=g["nb"] == 1, ragged=total % DET_THREADS != 0, image_boundary_in_block=c.N > 1 and HW % DET_THREADS != 0,
                second_trip=g["trips"] > 1, cap1024=cdiv(total, DET_THREADS) > DET_FWD_CAP, scratch_limited=c.get("scratch", DET_SCRATCH) // 5 < min(cdiv(total, 256), 1024),
                final_strides=g["nb"] > 64, den_override=bool(c.get("den")), grad_out=bool(c.get("go")), zero_gt=c.get("gt") == "zero",
                chain=(5 * g["trips"], 10 * g["trips"], 40 * g["trips"]))


def _det(name, N, H, W, **kw):
    return Case("det_loss", name, N=N, H=H, W=W, **kw)


DET_CASES = [
    _det("N1 11x13 one partial block", 1, 11, 13, go=2.5),
    _det("N2 16x16 whole blocks", 2, 16, 16),
    _det("N2 17x19 image boundary in a block", 2, 17, 19),
    _det("N2 17x19 den_override", 2, 17, 19, den=True, go=0.37),
    _det("N1 31x33 scratch 10 second trip", 1, 31, 33, scratch=10, go=1.0),
    _det("N1 129x131 more than 64 partials", 1, 129, 131, den=True),
    _det("N2 17x19 binary gt", 2, 17, 19, gt="binary", go=3.0),
    _det("N2 17x19 all-zero gt", 2, 17, 19, gt="zero", go=0.5),
    _det("N1 513x513 past the 1024 cap", 1, 513, 513, go=1.5),
]
DET_UNRUN = {"det_loss_bwd_kernel second trip": "more than 4096 x 256 = 1 048 576 pixels: 55 + 55 + 55 fp32 maps of that size, about 700 MB"}


def det_planted(c):
    """pixels (flat n * HW + p) that carry the special values: the first, the last, and the first pixel of the second block / second trip"""
    g = det_geometry(c.N, c.H, c.W, c.get("scratch", DET_SCRATCH))
    total = g["total"]
    return sorted({0, total - 1, min(total - 1, 256), min(total - 1, g["nb"] * DET_THREADS)})


def det_operands(c):
    """kp in (0, 1) with p in {0, 1, 1e-30, 1 - 2^-24} planted; t in {0, 1, fractional}; every fourth short / mid element equals its target"""
    g = torch.Generator().manual_seed(c.seed)
    N, H, W = c.N, c.H, c.W
    HW = H * W
    kp = (torch.rand(N, 5, HW, generator=g) * 0.98 + 0.01)
    gt = torch.randn(N, 55, HW, generator=g)
    t = (torch.rand(N, 5, HW, generator=g) * 1.6 - 0.3).clamp(0, 1)            # ~ 19 % zeros, 19 % ones, the rest fractional
    kind = c.get("gt", "mixed")
    if kind == "binary":
        t = (t > 0.5).float()
    gt[:, :5] = t
    sh = gt[:, 5:15] + torch.randn(N, 10, HW, generator=g)
    md = gt[:, 15:55] + torch.randn(N, 40, HW, generator=g)
    sh[:, :, ::4] = gt[:, 5:15, ::4]
    md[:, :, 1::4] = gt[:, 15:55, 1::4]
    for i in det_planted(c):
        n, p = divmod(i, HW)
        kp[n, :, p] = torch.tensor([0.0, 1.0, 1e-30, 1.0 - 2.0 ** -24, 0.0])
        gt[n, :5, p] = torch.tensor([1.0, 0.0, 1.0, 0.0, 0.0])
        sh[n, 1::2, p] = gt[n, 6:15:2, p] + 0.75                              # a live L1 difference where the mask is 1
    if kind == "zero":
        gt.zero_()
    shape = lambda x, C: x.reshape(N, C, H, W).contiguous()
    den = None
    if c.get("den"):
        den = torch.tensor([1234.0, 5678.0, 5.0 * N * HW * 3.0])              # {mask2 sum, mask4 sum, numel} of a larger global batch
    return {"kp": shape(kp, 5), "sh": shape(sh, 10), "md": shape(md, 40), "gt": shape(gt, 55), "den": den, "go": c.get("go")}


def log_ulps(p):
    """MARGIN x the worst error of the CPU float32 log(p) / log1p(-p) against float64, in ulps of the result, over the given fp32 p values (results
    the clamp at -100 replaces, and exact zeros, left out): the per-term allowance of the device logf / log1pf in a BCE sum"""
    worst = 0.0
    for f in (lambda x: torch.log1p(-x), torch.log):
        a32, a64 = f(p.float()), f(p.double())
        ok = (a64 > -100.0) & (a64 != 0)
        if bool(ok.any()):
            ulp = torch.exp2(torch.floor(torch.log2(a64[ok].abs())) - 23)
            worst = max(worst, float(((a32[ok].double() - a64[ok]).abs() / ulp).max()))
    return MARGIN * worst


class DetReference:
    def __init__(self, c, o=None):
        self.c, self.o = c, o or det_operands(c)
        o = self.o
        N, HW = c.N, c.H * c.W
        self.geom = det_geometry(c.N, c.H, c.W, c.get("scratch", DET_SCRATCH))
        flat = lambda x, C, dt: x.reshape(N, C, HW).to(dt)
        mid_idx = [MID_FROM[k >> 1] for k in range(40)]

        def pixel_terms(dt):
            P, T = flat(o["kp"], 5, dt), flat(o["gt"], 55, dt)[:, :5]
            G = flat(o["gt"], 55, dt)
            inv_r = torch.tensor(1.0, dtype=dt) / torch.tensor(KP_RADIUS, dtype=dt)
            l1, l0 = torch.log1p(-P).clamp_min(-100.0), torch.log(P).clamp_min(-100.0)
            bce = (T - 1) * l1 - T * l0
            m2, m4 = T.repeat_interleave(2, 1), T[:, mid_idx]
            short = (flat(o["sh"], 10, dt) - G[:, 5:15]).abs() * inv_r * m2
            mid = (flat(o["md"], 40, dt) - G[:, 15:55]).abs() * inv_r * m4
            pix = lambda x: x.sum(1).reshape(-1)
            return torch.stack([pix(bce), pix(short), pix(m2), pix(mid), pix(m4)]), pix((T - 1).abs() * l1.abs() + T.abs() * l0.abs()), (P, l1, l0)
        self.pix, bce_abs, (P64, l1, l0) = pixel_terms(F64)
        pix32, _, _ = pixel_terms(F32)
        self.log_ulps = log_ulps(flat(o["kp"], 5, F32))
        self.s = self.pix.sum(1)
        s32 = pix32.sum(1)
        self.bs = sum_allow(self.s, s32, self.pix.abs().sum(1))
        self.bs[0] = sum_allow(self.s[0], s32[0], bce_abs.sum()) + self.log_ulps * 2.0 ** -23 * bce_abs.sum()
        self.s32 = s32.double()
        self.exact_m2 = bool((flat(o["gt"], 55, F64)[:, :5].frac() == 0).all()) and float(self.s[2]) < 2 ** 24
        self.out8, self.b8 = self.final(self.s, self.bs)

    def final(self, s, bs):
        """det_loss_final_kernel from the five sums (float64) and their bounds: (out8, bound8), linear propagation + 2^-24 per fp32 rounding"""
        c, o = self.c, self.o
        ne = 5.0 * self.geom["total"]
        m2, m4, b2, b4 = float(s[2]), float(s[4]), float(bs[2]), float(bs[4])
        if o["den"] is not None:
            m2, m4, ne = (float(v) for v in o["den"])
            b2 = b4 = 0.0
        d2, d4 = m2 + EPS_DEN, m4 + EPS_DEN
        lkp, lsh, lmd = float(s[0]) / ne, float(s[1]) / d2, float(s[3]) / d4
        blkp = float(bs[0]) / ne + U32 * abs(lkp)
        blsh = float(bs[1]) / d2 + abs(lsh) * b2 / d2 + 4 * U32 * abs(lsh)          # (float)s1, (float)m2, +, /
        blmd = float(bs[3]) / d4 + abs(lmd) * b4 / d4 + 4 * U32 * abs(lmd)
        loss = lkp + lsh + 0.25 * lmd
        out = [loss, lkp, lsh, lmd, 1.0 / ne, 1.0 / d2, 1.0 / d4, m2]
        bnd = [blkp + blsh + 0.25 * blmd + 2 * U32 * (abs(lkp) + abs(lsh) + 0.25 * abs(lmd)), blkp, blsh, blmd,
               U32 / ne, (3 * U32 + b2 / d2) / d2, (3 * U32 + b4 / d4) / d4, 0.0 if (self.exact_m2 or o["den"] is not None) else b2 + U32 * m2]
        return torch.tensor(out, dtype=F64), torch.tensor(bnd, dtype=F64)

    def out8_ratio(self, got, out8=None):
        ref = self.out8 if out8 is None else out8
        return ratio(got.double() - ref, self.b8)

    def yardstick8(self):
        """out8 from the float32 pixel sums, finished in float32"""
        v, _ = self.final(self.s32, self.bs)
        return v.float()

    def mutants8(self):
        """{kind: out8} with one planted pixel dropped from the sums; with the second grid-stride trip skipped"""
        m = {f"pixel {i} dropped": self.final(self.s - self.pix[:, i], self.bs)[0] for i in det_planted(self.c)}
        if self.geom["trips"] > 1:
            m["second trip skipped"] = self.final(self.s - self.pix[:, self.geom["nb"] * DET_THREADS:].sum(1), self.bs)[0]
        return m

    def grads(self, dt=F64):
        """the three gradient maps from the inputs alone (fin recomputed in dtype dt)"""
        c, o = self.c, self.o
        T_ = lambda v: torch.tensor(v, dtype=dt)
        ne = 5.0 * self.geom["total"]
        m2, m4 = float(self.s[2]), float(self.s[4])
        if o["den"] is not None:
            m2, m4, ne = (float(v) for v in o["den"])
        go = T_(o["go"] if o["go"] is not None else 1.0)
        if dt == F64:
            fin4, fin5, fin6, inv_r = T_(1.0 / ne), T_(1.0 / (m2 + EPS_DEN)), T_(1.0 / (m4 + EPS_DEN)), T_(1.0 / KP_RADIUS)
        else:
            one = T_(1.0)
            fin4, fin5, fin6, inv_r = T_(1.0 / ne), one / (T_(m2) + T_(EPS_DEN)), one / (T_(m4) + T_(EPS_DEN)), one / T_(KP_RADIUS)
        P, G = o["kp"].to(dt), o["gt"].to(dt)
        T = G[:, :5]
        d = ((1 - P) * P).clamp_min(CLAMP_D)
        g_kp = (P - T) / d * (go * fin4)
        mid_idx = [MID_FROM[k >> 1] for k in range(40)]
        g_sh = torch.sign(o["sh"].to(dt) - G[:, 5:15]) * T.repeat_interleave(2, 1) * (go * fin5 * inv_r)
        g_md = torch.sign(o["md"].to(dt) - G[:, 15:55]) * T[:, mid_idx] * (go * T_(0.25) * fin6 * inv_r)
        return {"g_kp": g_kp, "g_sh": g_sh, "g_md": g_md}

    def grad_bounds(self, ref):
        """product bounds: k 2^-24 |ref| (+ the relative error of a mask sum that is neither exact nor overridden)"""
        rel2 = rel4 = 0.0
        if self.o["den"] is None and not self.exact_m2:
            rel2, rel4 = float(self.bs[2] / (self.s[2] + EPS_DEN)), float(self.bs[4] / (self.s[4] + EPS_DEN))
        return {"g_kp": K_GKP * U32 * ref["g_kp"].abs(), "g_sh": (K_GSH * U32 + rel2) * ref["g_sh"].abs(), "g_md": (K_GMD * U32 + rel4) * ref["g_md"].abs()}


# ==== kg_seg_loss ====================================================================================================================================
SEG_NPIX = (1, 255, 256, 257, 1000)


def seg_table(npatches):
    """[(prob_off, npix, pair0, npairs)], [(tgt_off, weight)]: patch sizes and pair counts cycle; a gap of 3 floats after every patch keeps prob_off off
    the 16-byte grid; pair weights as seg_loss.py forms them: 1 / nobj / nimg / npix"""
    patches, pairs = [], []
    off = toff = 0
    for b in range(npatches):
        npix, npairs = SEG_NPIX[b % 5], (1, 3)[(b // 2) % 2]
        patches.append((off + 1, npix, len(pairs), npairs))
        for k in range(npairs):
            pairs.append((toff, f32r(1.0 / (npatches + 3) / 2 / npix)))
            toff += npix
        off += npix + 3
    return patches, pairs, off + 1, toff


SEG_CASES = [Case("seg_loss", f"{n} patches", npatches=n, go=go) for n, go in ((3, 0.5), (5, None), (70, 2.0))]


def seg_claims(c):
    patches, pairs, nprob, ntgt = seg_table(c.npatches)
    return {"npatches": c.npatches, "final_strides": c.npatches > 64, "npix": {p[1] for p in patches}, "npairs": {p[3] for p in patches},
            "unaligned prob_off": any(p[0] % 4 for p in patches), "trips": {cdiv(p[1], 256) for p in patches}}


def seg_operands(c):
    patches, pairs, nprob, ntgt = seg_table(c.npatches)
    g = torch.Generator().manual_seed(c.seed)
    prob = torch.rand(nprob, generator=g) * 0.98 + 0.01
    tgt = (torch.rand(ntgt, generator=g) > 0.5).to(torch.uint8)
    for off, npix, p0, np_ in patches:
        prob[off] = 0.0 if (p0 % 2) else 1.0                   # p exactly 0 / 1 at the first pixel of every patch
    return {"patches": patches, "pairs": pairs, "prob": prob, "tgt": tgt, "go": c.get("go")}


class SegReference:
    """loss: the sum rule over every (pixel, pair) term; gprob: |d| <= k 2^-24 sum_k |w_k grad_k| with k = 6 + npairs (bce_grad 4, w *, the pair adds,
    * go) -- a patch matched with a 0-target and a 1-target pair adds terms of opposite sign, so the product bound is taken on the sum of their
    magnitudes, which is |ref| wherever the pairs agree"""

    def __init__(self, c, o=None):
        self.c, self.o = c, o or seg_operands(c)
        o = self.o

        def ev(dt):
            loss_terms, gref, gabs = [], torch.zeros(o["prob"].numel(), dtype=dt), torch.zeros(o["prob"].numel(), dtype=dt)
            go = torch.tensor(o["go"] if o["go"] is not None else 1.0, dtype=dt)
            for off, npix, p0, np_ in o["patches"]:
                p = o["prob"][off:off + npix].to(dt)
                l1, l0 = torch.log1p(-p).clamp_min(-100.0), torch.log(p).clamp_min(-100.0)
                d = ((1 - p) * p).clamp_min(CLAMP_D)
                gs, ga = torch.zeros(npix, dtype=dt), torch.zeros(npix, dtype=dt)
                for toff, w in o["pairs"][p0:p0 + np_]:
                    t = o["tgt"][toff:toff + npix].to(dt)
                    loss_terms.append(torch.tensor(w, dtype=dt) * ((t - 1) * l1 - t * l0))
                    gk = torch.tensor(w, dtype=dt) * ((p - t) / d)
                    gs, ga = gs + gk, ga + gk.abs()
                gref[off:off + npix], gabs[off:off + npix] = gs * go, ga * go.abs()
            return torch.cat(loss_terms), gref, gabs
        terms, self.g, gabs = ev(F64)
        terms32, self.g32, _ = ev(F32)
        self.loss, self.loss32 = terms.sum(), terms32.sum()
        self.log_ulps = log_ulps(o["prob"])
        self.bloss = sum_allow(self.loss, self.loss32, terms.abs().sum()) + self.log_ulps * 2.0 ** -23 * terms.abs().sum()
        self.terms = terms
        self.written = torch.zeros(o["prob"].numel(), dtype=torch.bool)
        kk = torch.zeros(o["prob"].numel(), dtype=F64)
        for off, npix, p0, np_ in o["patches"]:
            self.written[off:off + npix] = True
            kk[off:off + npix] = 6 + np_
        self.bg = kk * U32 * gabs


# ==== kg_bias_grad (conv_wgrad.hip) ==================================================================================================================
def bias_geometry(M, C, ld, aligned=True, scratch_floats=None):
    """per channel slab: route, row lanes, blocks, rows per block, and whether the 4-row unrolled loop and its remainder both run"""
    scratch_floats = 2048 * max(C, 1) if scratch_floats is None else scratch_floats          # ops.bias_grad
    vec = C % 8 == 0 and ld % 8 == 0 and aligned
    slabs = []
    step = 2048 if vec else 1024
    for c0 in range(0, C, step):
        Cs = min(C - c0, step)
        if vec:
            C8 = Cs // 8
            nrl = 256 // C8
            nb = min(scratch_floats // Cs, 2048, cdiv(M, 4 * nrl))
        else:
            nrl = max(1, 1024 // Cs)
            nb = min(scratch_floats // Cs, 1024, cdiv(M, 64))
        free = min(2048 if vec else 1024, cdiv(M, 4 * nrl) if vec else cdiv(M, 64))
        assert nb >= 1
        rpb = cdiv(M, nb)
        nb2 = cdiv(M, rpb)
        unrolled = remainder = False
        for b in {0, nb2 - 1}:
            rows = min((b + 1) * rpb, M) - b * rpb
            for rl in range(nrl):
                n = len(range(rl, rows, nrl))
                if vec:
                    unrolled |= n >= 4
                    remainder |= n % 4 != 0
        slabs.append({"Cs": Cs, "nrl": nrl, "nb": nb2, "rpb": rpb, "unrolled": unrolled, "remainder": remainder, "scratch_limited": nb < free,
                      "idle_threads": vec and 256 % (Cs // 8) != 0, "final_strides": nb2 > 64})
    return {"route": "vector" if vec else "scalar", "slabs": slabs}


def _bias(name, M, C, **kw):
    return Case("bias_grad", name, M=M, C=C, **kw)


BIAS_CASES = []
for _i, _C in enumerate((8, 24, 40, 64, 2056)):
    _nrl = 256 // (min(_C, 2048) // 8)
    for _j, _M in enumerate((1, 4 * _nrl - 1, 4 * _nrl, 4 * _nrl + 1, 5000)):
        if _C == 2056 and _j in (1, 2):
            continue
        BIAS_CASES.append(_bias(f"vector C{_C} M{_M}", _M, _C, fmt=("bf16", "half")[(_i + _j) % 2], P=2 if (_i + _j) % 3 == 0 else 1, accumulate=bool((_i + _j) % 2)))
for _i, _C in enumerate((5, 10, 55, 1027)):
    for _j, _M in enumerate((1, 63, 700)):
        BIAS_CASES.append(_bias(f"scalar C{_C} M{_M}", _M, _C, fmt=("bf16", "half")[(_i + _j) % 2], P=1, accumulate=bool(_j % 2)))
BIAS_CASES += [_bias("scalar C24 M700 base 2 bytes off", 700, 24, fmt="bf16", P=1, accumulate=False, misalign=True),
               _bias("vector C24 M5000 scratch for 3 blocks", 5000, 24, fmt="bf16", P=1, accumulate=True, scratch=3 * 24),
               _bias("scalar C55 M5000 scratch for 2 blocks", 5000, 55, fmt="half", P=1, accumulate=False, scratch=2 * 55),
               _bias("vector C64 M70000 more than 64 partials", 70000, 64, fmt="bf16", P=1, accumulate=False)]


def bias_layout(c):
    """(ctot, c0): the operand is a column slice [c0, c0 + C) of a buffer whose planes are ctot elements apart; c0 = 8 keeps 16-byte alignment,
    misalign -> c0 = 9 (2 bytes off)"""
    ctot = cdiv(c.C, 8) * 8 + 16
    return ctot, 9 if c.get("misalign") else 8


def bias_claims(c):
    ctot, c0 = bias_layout(c)
    g = bias_geometry(c.M, c.C, c.P * ctot, aligned=c0 % 8 == 0, scratch_floats=c.get("scratch"))
    s = g["slabs"]
    return {"route": g["route"], "nslabs": len(s), "unrolled": any(x["unrolled"] for x in s), "remainder": any(x["remainder"] for x in s),
            "scratch_limited": any(x["scratch_limited"] for x in s), "idle_threads": any(x["idle_threads"] for x in s), "final_strides": any(x["final_strides"] for x in s),
            "one_block": all(x["nb"] == 1 for x in s), "P": c.P, "fmt": c.fmt, "accumulate": c.accumulate, "misaligned": bool(c.get("misalign"))}


def bias_rows(c):
    """rows whose loss a mutant must show: the last row, row 0, the last row of block 0"""
    ctot, c0 = bias_layout(c)
    s = bias_geometry(c.M, c.C, c.P * ctot, aligned=c0 % 8 == 0, scratch_floats=c.get("scratch"))["slabs"][0]
    return sorted({0, c.M - 1, min(s["rpb"], c.M) - 1})


class BiasReference:
    def __init__(self, c):
        from .densecases import quantise
        g = torch.Generator().manual_seed(c.seed)
        dy = torch.randn(c.M, c.C, generator=g) * 0.5 + 0.125
        for r in bias_rows(c):
            dy[r] = 8.0 * (1 + (torch.arange(c.C) % 2))          # exact in one plane, far above FLOOR * sum |terms|
        self.c, self.dy = c, quantise(dy, c.fmt, c.P)
        self.prior = torch.randn(c.C, generator=g)
        d64 = self.dy.double()
        self.s64, self.s32 = d64.sum(0), self.dy.sum(0)
        self.b = sum_allow(self.s64, self.s32, d64.abs().sum(0))
        if c.accumulate:
            self.ref, self.f32 = self.prior.double() + self.s64, self.prior + self.s32
            self.bound = self.b + c.P * U32 * self.ref.abs()                                # one rounding per accumulating launch (one per plane)
        else:
            self.ref, self.f32, self.bound = self.s64, self.s32, self.b + (c.P - 1) * U32 * self.s64.abs()

    def dropped(self, r):
        return self.ref - self.dy[r].double()


# ==== kg_grad_pack / kg_grad_pack3 (loss.hip) ========================================================================================================
GP_THREADS, GP_TR_CAP, GP_PIX_CAP = 256, 2048, 8192


def gp_claims(c):
    total, HW = c.N * c.H * c.W, c.H * c.W
    cpad = sum(c.pads) if c.get("pads") else c.cpad
    tr = cpad <= 64
    cap = GP_TR_CAP if tr else GP_PIX_CAP
    blocks = min(cdiv(total, GP_THREADS), cap)
    Cs = c.Cs if c.get("pads") else (c.C,)
    return {"kernel": ("pack3" if c.get("pads") else "tr") if tr else "pixel", "vector_reads": tr and HW % 4 == 0, "tile_spans_images": c.N > 1 and HW % GP_THREADS != 0,
            "short_last_tile": 0 < total % GP_THREADS < 4, "one_quad_last_tile": tr and HW % 4 == 0 and total % GP_THREADS == 4, "ragged": total % GP_THREADS != 0, "wraps": total > blocks * GP_THREADS,
            "padding": any(C < p for C, p in zip(Cs, c.pads if c.get("pads") else (cpad,))), "channel_quads": tr and HW % 4 == 0 and max(Cs) > 4,
            "prob": bool(c.get("prob")), "scale": bool(c.get("scale")), "P": c.P, "fmt": c.fmt}


def _gp(name, N, C, cpad, H, W, **kw):
    return Case("grad_pack", name + f" {kw['fmt']} P{kw['P']}" + (" prob" if kw.get("prob") else "") + (" scale" if kw.get("scale") else ""), N=N, C=C, cpad=cpad, H=H, W=W, **kw)


GP_SHAPES = (("N2 C5 12x20 vector reads", 2, 5, 8, 12, 20), ("N2 C5 17x19 scalar reads", 2, 5, 8, 17, 19), ("N1 C10 7x37 short last tile", 1, 10, 16, 7, 37), ("N1 C10 13x20 one quad in the last tile", 1, 10, 16, 13, 20),
             ("N3 C40 17x19", 3, 40, 40, 17, 19), ("N1 C40 16x18 vector", 1, 40, 48, 16, 18), ("N2 C70 9x13 per-pixel kernel", 2, 70, 72, 9, 13))
GP_CASES = []
for _i, (_name, _N, _C, _cpad, _H, _W) in enumerate(GP_SHAPES):
    for _v, (_fmt, _P) in enumerate((("bf16", 1), ("bf16", 2), ("half", 1), ("half", 2))):
        _k = _i + _v
        GP_CASES.append(_gp(_name, _N, _C, _cpad, _H, _W, fmt=_fmt, P=_P, prob=_k % 2 == 0, scale=(_k // 2) % 2 == 0 or _fmt == "half"))
GP_CASES += [_gp("N1 C5 725x725 cap scalar reads", 1, 5, 8, 725, 725, fmt="bf16", P=1, prob=True, scale=False),
             _gp("N1 C5 724x728 cap vector reads", 1, 5, 8, 724, 728, fmt="half", P=1, prob=True, scale=True)]
GP3_CASES = [Case("grad_pack3", f"{name} {fmt} P{P}", N=N, H=H, W=W, Cs=Cs, pads=pads, fmt=fmt, P=P, prob=True, scale=True)
             for name, N, H, W, Cs, pads in (("N2 17x19 pads 64", 2, 17, 19, (5, 10, 40), (8, 16, 40)), ("N2 12x20 pads 64", 2, 12, 20, (5, 10, 40), (8, 16, 40)),
                                             ("N1 7x37 pads 24", 1, 7, 37, (5, 3, 1), (8, 8, 8)), ("N3 16x16 pads 24", 3, 16, 16, (2, 7, 8), (8, 8, 8)))
             for fmt, P in (("bf16", 1), ("half", 2))]
GP3_CASES += [Case("grad_pack3", "N1 725x725 cap pads 24 bf16 P1", N=1, H=725, W=725, Cs=(5, 3, 1), pads=(8, 8, 8), fmt="bf16", P=1, prob=True, scale=True),
              Case("grad_pack3", "N1 724x728 cap pads 24 half P1", N=1, H=724, W=728, Cs=(5, 3, 1), pads=(8, 8, 8), fmt="half", P=1, prob=True, scale=True)]
GP_UNRUN = {"grad_pack_kernel (cpad > 64) second trip": "more than 8192 x 256 = 2 097 152 pixels x 72 channels: 151 M output elements"}
GP_SCALE = 2.0 ** 9
HALF_SUB = 2.0 ** -25          # half the spacing of IEEE half's subnormals: an absolute term of every half output (the bf16 build has fp32's exponent range)


def gp_operands(c, C=None, salt=0):
    """loss-gradient magnitudes: |g| in [2^-17, 2^-7) log-uniform; prob in (0.02, 0.98)"""
    C = c.C if C is None else C
    g = torch.Generator().manual_seed(c.seed + salt)
    shape = (c.N, C, c.H, c.W)
    grad = torch.exp2(torch.rand(shape, generator=g) * 10 - 17) * (2 * torch.randint(0, 2, shape, generator=g).float() - 1)
    prob = torch.rand(shape, generator=g) * 0.96 + 0.02
    return grad, prob


class GradPackReference:
    """rows [N*H*W, C]: float64, the float32 evaluation rounded to the planes, the rows bound (+ 2^-25 for half)"""

    def __init__(self, c, grad, prob):
        from .densecases import quantise
        S = GP_SCALE if c.scale else 1.0
        rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])

        def ev(dt):
            v = grad.to(dt)
            if prob is not None:
                v = v * (prob.to(dt) * (1 - prob.to(dt)))
            return rows(v * S)
        self.ref, f32 = ev(F64), ev(F32)
        self.f32 = quantise(f32, c.fmt, c.P)
        u = U_OUT[(c.fmt, c.P)]
        yard = float((f32.double() - self.ref).abs().max())
        rms = float(self.ref.pow(2).mean().sqrt())
        self.bound = u * self.ref.abs() + max(MARGIN * yard, FLOOR * rms) + (HALF_SUB if c.fmt == "half" else 0.0)

    def ratio(self, got, lo=0, hi=None):
        hi = self.ref.shape[0] if hi is None else hi
        return ratio(got.double() - self.ref[lo:hi], self.bound[lo:hi])


# ==== kg_pack_weight_batch (conv_igemm.hip) ==========================================================================================================
def pack_jobs():
    """the jobs of the batched-pack test: (kind, Cout, Cin, k, xP, wP, row0, c0, extra).  kinds: fwd, tr (transposed), rows (row map + plane group),
    narrow (chan_slot).  46 jobs"""
    jobs = []
    planes = ((1, 1), (2, 2), (3, 3), (2, 1))
    i = 0
    for k in (1, 3, 7):
        for xP, wP in planes:
            cout, cin = (70, 100) if k == 1 else (33, 24) if k == 3 else (5, 72)
            jobs.append(("fwd", cout, cin, k, xP, wP, 64 * (i % 2), 0, None))
            jobs.append(("tr", cout, cin, k, xP, wP, 0, 64 * ((i + 1) % 2), None))
            i += 1
    for k, (xP, wP) in ((7, (1, 1)), (7, (2, 2)), (3, (2, 1)), (1, (3, 3))):
        for group, cout in enumerate((5, 10, 40)):
            jobs.append(("rows", cout, 24, k, xP, wP, 0, 0, group))
    for slot, cout in ((8, 5), (8, 8), (16, 10), (16, 16)):
        jobs.append(("narrow", cout, 70, 7, 1, 1, 64 * (slot == 16), 0, slot))
    for cout, cin in ((130, 65), (64, 64), (1, 1), (65, 130), (200, 8), (8, 200)):
        jobs.append(("fwd" if cout != 65 else "tr", cout, cin, 3, 1, 1, 0, 0, None))
    return jobs


def pack_grid(kind, cout, cin):
    """(gx, gy) of a job: PackQueue.add / the single-tensor launchers"""
    tr = kind in ("tr", "narrow")
    return (cdiv(cout, 64), cin) if tr else (cout, cdiv(cin, 64))


def pack_layout(jobs):
    """[(blk0, gx)] and the block total of one kg_pack_weight_batch launch over `jobs` in order"""
    out, blk = [], 0
    for kind, cout, cin, *_ in jobs:
        gx, gy = pack_grid(kind, cout, cin)
        out.append((blk, gx))
        blk += gx * gy
    return out, blk
