"""Parity cases of the STREAMING kernels of csrc/norm_pool.hip (TEST INFRASTRUCTURE, not product; imports no GPU library).

BatchNorm train / frozen forward and backward, the max-pool, the dense bilinear resize and its exact-2x kernel, add_rows, rows_rescale / rows_scale /
rows_scale_multi and img_pack are element-wise or column-reduction kernels whose risk is INDEXING: the kg_divmod branch, a second trip of a
grid-stride loop, the row range of a reduce block, a strip tail.  This module
  * restates the launch geometry of every entry point on the host (`ew_launch`, `reduce_geometry`, `frozen_tail`, `bilinear_route`, `absmax_geometry`),
    each next to the source line it comes from, so that the index paths a case claims (`claims`) are COMPUTED,
  * lists the cases (`CASES`): the smallest shapes at which each path exists, small ones in five storage variants (bf16 x {1, 2, 3} planes,
    half x {1, 2} planes), the ~33 M-element `wraps` cases on one bf16 plane,
  * builds seeded operands that the planes hold exactly (densecases.split_planes), the float64 reference, the float32 CPU evaluation, the bounds and
    the mutants the bounds have to see (`Reference`).

Bound per stored element (densecases.Reference's convention, its constants imported, not re-chosen):
    U_OUT[(fmt, P)] * |ref| + max(MARGIN * worst |float32 CPU evaluation - float64| over the case, FLOOR * rms(ref))
three bf16 planes count as "f32"; where the operation is exact (max-pool forward, rows_scale* by a power of two, img_pack padding channels, columns
outside the written slice) the bound is 0 and the comparison is bit equality.
Bound per reduced quantity (densecases.stats_reference's rule): a sum gets max(MARGIN * |float32 evaluation - float64|, FLOOR * sum |terms|)
(+ sum |dy| * the fp32 rounding of xhat for the backward's second sum), propagated LINEARLY to what the finalize kernels derive from it:
    mean = s / M                      d mean   = ds / M
    var  = q / M - mean^2             d var    = dq / M + 2 |mean| ds / M
    invstd = (var + eps)^-1/2         d invstd = 1/2 invstd^3 d var
    scale = gamma invstd, shift = beta - mean scale, running statistics, dgamma / dbeta, coef = {a, -a sx / M, -a s / M}: the product rule,
each plus U32 = 2^-24 times the magnitudes that are rounded to fp32 on the way (one per rounding).  Nothing is fitted to a kernel's output."""
import math

import torch
import torch.nn.functional as F

from .densecases import DT, FLOOR, MARGIN, U_OUT, cdiv, quantise, split_planes

FILL = 9.0
U32 = 2.0 ** -24
VARIANTS = (("bf16", 1), ("bf16", 2), ("bf16", 3), ("half", 1), ("half", 2))
EPS32 = float(torch.tensor(1e-5, dtype=torch.float32))          # the eps the C ABI receives (float)
INF = float("inf")


def u_out(fmt, P):
    return U_OUT["f32"] if P == 3 else U_OUT[(fmt, P)]


# ---- launch geometry, restated ------------------------------------------------------------------------------------------------------------

EW_CAP, EW_THREADS = 16384, 256            # bn_apply, bn_bwd_apply, bn_bwd_frozen_scale, maxpool, bilinear (generic), add_rows: `if (blocks > 16384)`
PACK_CAP = 8192                            # kg_img_pack: `if (blocks > 8192)`, one thread per PIXEL
BIL2_ROWS, BIL2_CAP = 8, 65536             # bilinear2x_fwd_kernel: input rows per thread; `if (blocks2 > 65536)`
ABS_THREADS, ABS_CAP, ABS_UNROLL = 1024, 256, 4      # rows_absmax_kernel: blocks = min(256, ceil(total / 4096)), 4 chunks in flight per thread
SCALE_CAPS = {"rescale": (512, 1024), "rows_scale": (2048, 256), "scale_multi": (512, 256)}      # rows_scale_kernel launches: (block cap, threads)
REDUCE_MAX_BLOCKS, REDUCE_ROWS = 512, 256  # reduce_geometry: `if (n > 512)`, need = (M + 255) / 256


def ew_launch(total, C8, cap=EW_CAP, threads=EW_THREADS):
    """a grid-stride launch over `total` 16-byte chunks: which kg_divmod branch (csrc/kg_common.h: shift when C8 is a power of two, 32-bit division
    while the index fits 32 bits), and whether the loop takes a second, partly filled trip"""
    sweep = cap * threads
    return {"blocks": min(cdiv(total, threads), cap), "pow2": (C8 & (C8 - 1)) == 0, "wraps": total > sweep and total % sweep != 0,
            "div64": total > 0xffffffff}


def reduce_geometry(M, C, scratch_floats):
    """norm_pool.hip reduce_geometry: (nb, rows_per_block) or None when the scratch holds no block"""
    n = min(scratch_floats // (2 * C), REDUCE_MAX_BLOCKS, (M + REDUCE_ROWS - 1) // REDUCE_ROWS)
    if n < 1:
        return None
    rpb = cdiv(M, n)
    return cdiv(M, rpb), rpb


def default_scratch(C, bwd):
    """what ops.bn_stats_train / ops.bn_bwd / ops.bn_bwd_frozen pass"""
    return 2 * C * 512 + (3 * C if bwd else 0)


def frozen_tail(M, nb, rpb):
    """bn_bwd_frozen_stats_kernel's loop `for (r = r0 + rl; r < r1; r += 64) { two = r + 32 < r1; ...}`: does some lane make a trip with two rows
    and then a last trip with one"""
    for b in {0, nb - 1}:
        r0, r1 = b * rpb, min((b + 1) * rpb, M)
        for rl in range(32):
            r, saw_two = r0 + rl, False
            while r < r1:
                if r + 32 < r1:
                    saw_two = True
                elif saw_two:
                    return True
                r += 64
    return False


def bilinear_route(IH, IW, OH, OW):
    """kg_bilinear_fwd, dense: the exact-2x kernel behind `OH == 2 * IH && OW == 2 * IW && IH >= 2 && IW >= 2` (KG_BILINEAR_2X unset)"""
    return "2x" if (OH == 2 * IH and OW == 2 * IW and IH >= 2 and IW >= 2) else "generic"


def absmax_geometry(M, C8):
    """rows_absmax_kernel as kg_rows_rescale launches it: blocks, the constant (row, chunk) advance dr / dc of a thread, sweeps of 4 * stride chunks"""
    total = M * C8
    blocks = min(cdiv(total, ABS_THREADS * ABS_UNROLL), ABS_CAP)
    stride = blocks * ABS_THREADS
    dr = stride // C8
    dc = stride - dr * C8
    sweep = ABS_UNROLL * stride
    return {"total": total, "blocks": blocks, "stride": stride, "dr": dr, "dc": dc, "sweeps": cdiv(total, sweep), "sweep": sweep,
            "pow2": (C8 & (C8 - 1)) == 0, "carry": dc > 0}


# ---- cases --------------------------------------------------------------------------------------------------------------------------------

class Case:
    """One case: entry (the family of C ABI entry points it runs), a shape, the 16-bit format, the planes of every operand (P, or `planes[name]`) and
    its options.  Element-wise operands are column slices (c0 = 8) of wider buffers whose planes are `ctot` elements apart (ld = P * ctot)."""

    def __init__(self, entry, name, fmt="bf16", P=1, planes=None, **kw):
        self.entry, self.fmt, self.P, self.planes = entry, fmt, P, planes or {}
        self.opt = kw
        self.name = f"{entry} {name} {fmt} P{P}" + ("".join(f" {k}{v}" for k, v in sorted(self.planes.items())))
        self.seed = sum((i + 1) * ord(ch) for i, ch in enumerate(self.name)) % (2 ** 31)

    def __getattr__(self, k):
        try:
            return self.__dict__["opt"][k]
        except KeyError:
            raise AttributeError(k)

    def get(self, k, default=None):
        return self.opt.get(k, default)

    def pl(self, operand):
        return self.planes.get(operand, self.P)

    def __repr__(self):
        return f"Case({self.name})"


def claims(c):
    """the index paths the case runs, from the restated geometry: a dict"""
    e, o = c.entry, c.opt
    if e in ("bn_apply", "bn_frozen_scale", "add_rows"):
        return dict(ew_launch(c.M * (c.C // 8), c.C // 8), kernel=e)
    if e in ("bn_stats", "bn_bwd", "bn_frozen"):
        bwd = e != "bn_stats"
        scratch = c.get("scratch") or default_scratch(c.C, bwd)
        nb, rpb = reduce_geometry(c.M, c.C, scratch - (3 * c.C if bwd else 0))
        free = reduce_geometry(c.M, c.C, 1 << 30)
        d = {"kernel": e, "nb": nb, "rpb": rpb, "nb>64": nb > 64, "rpb%32": rpb % 32 != 0, "rpb%64": rpb % 64 != 0, "scratch_limited": (nb, rpb) != free,
             "cap512": (c.M + REDUCE_ROWS - 1) // REDUCE_ROWS > REDUCE_MAX_BLOCKS, "slabs": cdiv(c.C, 64), "part_slab": c.C % 64 != 0,
             "two_row_tail": e == "bn_frozen" and frozen_tail(c.M, nb, rpb), "parts": bool(c.get("parts"))}
        if e == "bn_bwd":
            d.update({"apply_" + k: v for k, v in ew_launch(c.M * (c.C // 8), c.C // 8).items()})
            if c.get("parts"):
                d["nb_parts"] = c.parts
        if e == "bn_frozen":
            d["pow2"] = None
        return d
    if e == "bn_finalize":
        return {"kernel": e, "nb": c.nb, "nb>64": c.nb > 64}
    if e == "maxpool":
        OH, OW = (c.H - 1) // 2 + 1, (c.W - 1) // 2 + 1
        f, b = ew_launch(c.N * OH * OW * (c.C // 8), c.C // 8), ew_launch(c.N * c.H * c.W * (c.C // 8), c.C // 8)
        return {"kernel": e, "pow2": f["pow2"], "fwd_wraps": f["wraps"], "bwd_wraps": b["wraps"]}
    if e in ("bilinear_fwd", "bilinear_bwd"):
        route = bilinear_route(c.IH, c.IW, c.OH, c.OW) if e == "bilinear_fwd" else "generic"
        C8 = c.C // 8
        d = {"kernel": e, "route": route, "pow2": (C8 & (C8 - 1)) == 0, "down": c.OH < c.IH or c.OW < c.IW, "up": c.OH > c.IH or c.OW > c.IW,
             "guard_ih1": c.OH == 2 * c.IH and c.OW == 2 * c.IW and c.IH == 1, "guard_iw1": c.OH == 2 * c.IH and c.OW == 2 * c.IW and c.IW == 1,
             "mask": bool(c.get("mask"))}
        if route == "2x":
            strips = cdiv(c.IH, BIL2_ROWS)
            d.update(strips=strips, strip_tail=c.IH % BIL2_ROWS != 0, wraps=ew_launch(c.N * strips * c.IW * C8, C8, BIL2_CAP)["wraps"])
        else:
            rows = c.N * (c.OH * c.OW if e == "bilinear_fwd" else c.IH * c.IW)
            d["wraps"] = ew_launch(rows * C8, C8)["wraps"]
        return d
    if e == "img_pack":
        return {"kernel": e, "wraps": ew_launch(c.N * c.H * c.W, 1, PACK_CAP)["wraps"], "padding": c.C < 8}
    if e in ("rescale", "rows_scale"):
        g = absmax_geometry(c.M, c.C // 8) if e == "rescale" else {}
        cap, th = SCALE_CAPS[e]
        g = dict(g, kernel=e, scale_wraps=ew_launch(c.M * (c.C // 8) * c.P, 1, cap, th)["wraps"], plant=c.get("plant"), value=c.get("value"))
        if e == "rescale" and c.get("plant") is not None:
            p = plant_chunk(c)
            g["plant_sweep"] = p // g["sweep"]
            g["plant_partial_group"] = (p % g["stride"]) + (p // g["sweep"]) * g["sweep"] + (ABS_UNROLL - 1) * g["stride"] >= g["total"]
        return g
    if e == "scale_multi":
        return {"kernel": e, "n": len(c.items)}
    raise ValueError(e)


def plant_chunk(c):
    """flat chunk index (row * C8 + chunk) where a rescale case plants its maximum"""
    g = absmax_geometry(c.M, c.C // 8)
    total, stride, sweep = g["total"], g["stride"], g["sweep"]
    where = c.plant
    if where == "chunk0":
        return 0
    if where == "sweep2":                       # the first chunk of the second sweep
        assert total > sweep
        return sweep
    if where == "partial":                      # a chunk whose thread has fewer than 4 chunks left in its last trip
        last0 = (g["sweeps"] - 1) * sweep
        for u in (2, 1, 0):
            p = last0 + u * stride + min(stride, total - last0 - u * stride) - 1
            if last0 + u * stride <= p < total and (p - last0) % stride + (ABS_UNROLL - 1) * stride + last0 >= total:
                return p
        raise AssertionError("no partial group")
    if where == "mid":
        return total // 2 + 1
    return total - 1                            # "last", "elem7", "negative", "lofavour"


_CASES = []


def _add(entry, name, variants=VARIANTS, **kw):
    for fmt, P in variants:
        _CASES.append(Case(entry, name, fmt, P, **kw))


ONE = (("bf16", 1),)
EW_SHAPES = [(C, M) for C in (8, 24, 64, 320) for M in (1, 37, 1000)]
WRAP_M = 524300                            # x 8 chunks of 64 channels = 4 194 400 chunks > 16384 x 256 = 4 194 304
RED_SHAPES = [(1, 8), (1, 72), (33, 72), (33, 256), (257, 8), (257, 256), (8225, 72), (8225, 256), (16641, 8), (16641, 72), (131100, 8), (131100, 72)]
MIXED = {"bf16": ({"x": 1, "dy": 2, "res": 2, "b": 3, "y": 3}, {"x": 3, "dy": 1, "res": 1, "b": 1, "y": 2}),
         "half": ({"x": 1, "dy": 2, "res": 2, "b": 2, "y": 2}, {"x": 2, "dy": 1, "res": 1, "b": 1, "y": 1})}

for i, (C, M) in enumerate(EW_SHAPES):
    for v, var in enumerate(VARIANTS):
        k = i + v
        _add("bn_apply", f"M{M} C{C}", (var,), M=M, C=C, res=bool(k & 1), relu=bool(k & 2))
        _add("bn_frozen_scale", f"M{M} C{C}", (var,), M=M, C=C)
        _add("add_rows", f"M{M} C{C}", (var,), M=M, C=C, b=k % 2 == 0, mask=(k // 2) % 2 == 0, scale=("none", "one", "pair")[(k // 4) % 3])
        _add("bn_bwd", f"M{M} C{C}", (var,), M=M, C=C, accumulate=bool(k & 1))
for fmt, mixes in MIXED.items():
    for j, mix in enumerate(mixes):
        _CASES.append(Case("bn_apply", "M37 C24 mixed", fmt, 1, mix, M=37, C=24, res=True, relu=True))
        _CASES.append(Case("add_rows", "M37 C24 mixed", fmt, 1, mix, M=37, C=24, b=True, mask=True, scale="pair"))
        _CASES.append(Case("bn_bwd", "M37 C24 mixed", fmt, 1, mix, M=37, C=24, accumulate=bool(j)))
        _CASES.append(Case("bn_frozen", "M257 C72 mixed", fmt, 1, mix, M=257, C=72, accumulate=bool(j)))
        _CASES.append(Case("bn_frozen_scale", "M37 C24 mixed", fmt, 1, mix, M=37, C=24))
_add("bn_apply", f"M{WRAP_M} C64 wraps", ONE, M=WRAP_M, C=64, res=True, relu=True)
_add("bn_frozen_scale", f"M{WRAP_M} C64 wraps", ONE, M=WRAP_M, C=64)
_add("add_rows", f"M{WRAP_M} C64 wraps", ONE, M=WRAP_M, C=64, b=True, mask=True, scale="pair")
_add("bn_bwd", f"M{WRAP_M} C64 wraps", ONE, M=WRAP_M, C=64, accumulate=False)

for i, (M, C) in enumerate(RED_SHAPES):
    big = M * C > 2_000_000
    for v, var in enumerate(ONE if big else VARIANTS):
        k = i + v
        _add("bn_stats", f"M{M} C{C}", (var,), M=M, C=C, running=k % 2 == 0)
        _add("bn_bwd", f"M{M} C{C} red", (var,), M=M, C=C, accumulate=bool(k & 1))
        _add("bn_frozen", f"M{M} C{C}", (var,), M=M, C=C, accumulate=bool(k & 1))
# scratch for three blocks only (through the C ABI: the ops wrappers always pass 512 blocks' worth), partials from the host in the [nb][C][2] layout
for M, C in ((8225, 72), (16641, 8)):
    _add("bn_stats", f"M{M} C{C} scratch3", M=M, C=C, running=True, scratch=2 * C * 3)
    _add("bn_bwd", f"M{M} C{C} scratch3", M=M, C=C, accumulate=False, scratch=2 * C * 3 + 3 * C)
    _add("bn_frozen", f"M{M} C{C} scratch3", M=M, C=C, accumulate=True, scratch=2 * C * 3 + 3 * C)
for M, C, nbp in ((257, 72, 3), (16641, 8, 261), (8225, 256, 70)):
    _add("bn_bwd", f"M{M} C{C} parts{nbp}", M=M, C=C, accumulate=False, parts=nbp)
for M, C, nb in ((33, 8, 1), (8225, 72, 3), (16641, 256, 66), (131100, 8, 512), (8225, 8, 129)):
    _add("bn_finalize", f"M{M} C{C} nb{nb}", ONE, M=M, C=C, nb=nb, running=nb != 3)

POOL_HW = ((1, 1), (2, 3), (17, 22), (18, 21))
for i, (H, W) in enumerate(POOL_HW):
    for j, C in enumerate((8, 24, 64)):
        _add("maxpool", f"N{1 + (i + j) % 2} {H}x{W} C{C}", N=1 + (i + j) % 2, H=H, W=W, C=C)
_add("maxpool", "N1 725x725 C64 wraps", ONE, N=1, H=725, W=725, C=64)

BIL = ((5, 7, 13, 10), (13, 9, 5, 4), (1, 6, 2, 12), (6, 1, 12, 2), (9, 5, 18, 10), (8, 8, 16, 16), (19, 3, 38, 6))
for IH, IW, OH, OW in BIL:
    for N, C in ((1, 8), (3, 24), (1, 64), (3, 8)):
        _add("bilinear_fwd", f"N{N} {IH}x{IW} to {OH}x{OW} C{C}", N=N, IH=IH, IW=IW, OH=OH, OW=OW, C=C)
        for mask in (False, True):
            _add("bilinear_bwd", f"N{N} {IH}x{IW} from {OH}x{OW} C{C}" + (" mask" if mask else ""), N=N, IH=IH, IW=IW, OH=OH, OW=OW, C=C, mask=mask)
_add("bilinear_fwd", "N1 400x400 to 725x725 C64 wraps", ONE, N=1, IH=400, IW=400, OH=725, OW=725, C=64)
_add("bilinear_bwd", "N1 725x725 from 800x800 C64 wraps mask", ONE, N=1, IH=725, IW=725, OH=800, OW=800, C=64, mask=True)

for N, C, H, W in ((1, 3, 5, 7), (2, 1, 9, 4), (3, 8, 6, 6), (2, 3, 33, 31)):
    _add("img_pack", f"N{N} C{C} {H}x{W}", N=N, C=C, H=H, W=W)
_add("img_pack", "N1 C3 1449x1448 wraps", ONE, N=1, C=3, H=1449, W=1448)          # 2 098 152 pixels > 8192 x 256

T_LOG2 = 4
ABS_SHAPES = ((777, 64), (5000, 24), (131100, 64), (349600, 24))          # the last two: a second sweep of 224 chunks, C8 = 8 and C8 = 3
for M, C in ABS_SHAPES:
    big = M > 10000
    sweeps = absmax_geometry(M, C // 8)["sweeps"]
    for plant in ("chunk0", "last", "partial", "elem7", "negative", "mid") + (("sweep2",) if sweeps > 1 else ()):
        _add("rescale", f"M{M} C{C} max at {plant}", ONE if big else VARIANTS, M=M, C=C, plant=plant, value="big")
    _add("rescale", f"M{M} C{C} max at last in the low plane's favour", (("bf16", 2),) if big else (("bf16", 2), ("bf16", 3), ("half", 2)), M=M, C=C,
         plant="lofavour", value="big")
for value in ("pow2", "pow2-ulp", "small", "zero", "inf"):
    _add("rescale", f"M777 C64 {value}", M=777, C=64, plant="last", value=value)
for M, C in ((777, 64), (5000, 24)):
    for k, sc in enumerate(("one", "pair", "unit")):
        _add("rows_scale", f"M{M} C{C} scale {sc}", M=M, C=C, scale=sc)
_add("rows_scale", "M131100 C64 scale pair", ONE, M=131100, C=64, scale="pair")          # 1 048 800 chunks > 2048 x 256
for fmt in ("bf16", "half"):
    _CASES.append(Case("scale_multi", "8 tensors", fmt, 1, M=0, C=0, scale="pair",
                       items=((777, 64, 1, False), (1, 8, 2, False), (37, 24, 2, True), (1000, 320, 1, False), (5, 8, 3 if fmt == "bf16" else 2, False),
                              (4100, 64, 1, True), (33, 72, 2, False), (140000, 8, 1, False))))          # (M, C, P, column slice); 140000 > 512 x 256
    _CASES.append(Case("scale_multi", "1 tensor", fmt, 2, M=0, C=0, scale="one", items=((37, 24, 2, True),)))

CASES = tuple(_CASES)
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# one BatchNorm statistics case that is NOT a parity case: channels with |mean| = 30 sigma (the one-pass variance cancels 900 : 1)
CONDITIONING = Case("bn_stats", "M8225 C72 mean 30 sigma", "bf16", 3, M=8225, C=72, running=False, mean_sigmas=30.0)

# (claim, value) pairs that at least one case of the named kernels must compute: the paths the issue lists
REQUIRED = (
    [(k, "pow2", False) for k in ("bn_apply", "bn_frozen_scale", "add_rows", "maxpool", "bilinear_fwd", "bilinear_bwd")] + [("bn_bwd", "apply_pow2", False)]
    + [(k, "pow2", True) for k in ("bn_apply", "bn_frozen_scale", "add_rows", "maxpool", "bilinear_fwd", "bilinear_bwd")]
    + [(k, "wraps", True) for k in ("bn_apply", "bn_frozen_scale", "add_rows", "bilinear_fwd", "bilinear_bwd", "img_pack")]
    + [("bn_bwd", "apply_wraps", True), ("maxpool", "bwd_wraps", True)]
    + [(k, cl, True) for k in ("bn_stats", "bn_bwd", "bn_frozen") for cl in ("nb>64", "rpb%32", "rpb%64", "scratch_limited", "cap512", "part_slab")]
    + [(k, "slabs", 4) for k in ("bn_stats", "bn_bwd", "bn_frozen")] + [(k, "rpb", 129) for k in ("bn_stats", "bn_bwd", "bn_frozen")]
    + [("bn_frozen", "two_row_tail", True), ("bn_frozen", "two_row_tail", False), ("bn_bwd", "parts", True), ("bn_finalize", "nb>64", True)]
    + [("bilinear_fwd", "route", "generic"), ("bilinear_fwd", "route", "2x"), ("bilinear_fwd", "down", True), ("bilinear_fwd", "guard_ih1", True),
       ("bilinear_fwd", "guard_iw1", True), ("bilinear_fwd", "strip_tail", True), ("bilinear_fwd", "strip_tail", False), ("bilinear_fwd", "strips", 3),
       ("bilinear_bwd", "mask", True), ("bilinear_bwd", "mask", False), ("bilinear_bwd", "down", True)]
    + [("rescale", "plant_sweep", 1), ("rescale", "plant_partial_group", True), ("rescale", "scale_wraps", True), ("rows_scale", "scale_wraps", True)]
)
# paths that stay unrun, with the size they would need
UNRUN = {"kg_divmod 64-bit branch": "a flat chunk index above 2^32: 550 GB of bf16 rows",
         "maxpool forward second trip": "a 134 M-element input (4 194 304 output chunks x 8 channels x 4 inputs per output)",
         "bilinear2x second trip": "65 536 x 256 threads x 8 rows x 8 channels: about 1 G input elements"}


def required_missing(cases=CASES):
    cl = [claims(c) for c in cases]
    out = [(k, name, val) for k, name, val in REQUIRED if not any(d["kernel"] == k and d.get(name) == val for d in cl)]
    # the absmax carry `c >= C8` exists only where dc > 0: a C8 that does not divide the stride -- once in a case with a second sweep
    if not any(d["kernel"] == "rescale" and d["carry"] and not d["pow2"] and d["sweeps"] > 1 and d.get("plant_sweep") == 1 for d in cl):
        out.append(("rescale", "carry in a second sweep", True))
    return out


# ---- operands ---------------------------------------------------------------------------------------------------------------------------------

def layout(v, fmt, P, sliced=True, fill=FILL):
    """host buffer of a rows operand: [rows, P * ctot] in the 16-bit format, plane p at columns p * ctot + c0 .. + C, every other column = fill.
    Returns (buffer, c0, ctot): ld = P * ctot, plane stride ctot."""
    r, C = v.shape
    ctot, c0 = (C + 16, 8) if sliced else (C, 0)
    buf = torch.full((r, P * ctot), fill, dtype=DT[fmt])
    for p, plane in enumerate(split_planes(v, fmt, P)):
        buf[:, p * ctot + c0:p * ctot + c0 + C] = plane.to(DT[fmt])
    return buf, c0, ctot


def _randn(g, shape, scale=1.0, shift=0.0):
    return torch.randn(shape, generator=g) * scale + shift


def reduce_rows(c, scratch=None):
    """the rows a reduction mutant drops: last row of block 0's range, last row overall, row r0 + 32 (the frozen kernel's second slot)"""
    bwd = c.entry != "bn_stats"
    if c.get("parts"):
        return sorted({c.M - 1, min(63, c.M - 1)})
    nb, rpb = reduce_geometry(c.M, c.C, (c.get("scratch") or default_scratch(c.C, bwd)) - (3 * c.C if bwd else 0))
    rows = {min(rpb, c.M) - 1, c.M - 1}
    if c.M > 32:
        rows.add(32)
    return sorted(rows)


class Operands:
    """seeded host operands (fp32 tensors that the case's planes hold exactly)"""

    def __init__(self, c):
        g = torch.Generator().manual_seed(c.seed)
        e, fmt = c.entry, c.fmt
        q = lambda t, name: quantise(t, fmt, c.pl(name))
        self.c = c
        if e in ("bn_apply", "bn_frozen_scale", "add_rows", "bn_bwd", "bn_stats", "bn_frozen"):
            M, C = c.M, c.C
            sigma = torch.rand(C, generator=g) + 0.5
            ms = c.get("mean_sigmas")
            mean = sigma * ((torch.rand(C, generator=g) * 4 - 2) if ms is None else ms * (2 * torch.randint(0, 2, (C,), generator=g).float() - 1))
            x = _randn(g, (M, C)) * sigma + mean                      # well-conditioned channels: |mean| <= 2 sigma
            dy = _randn(g, (M, C), 0.5, 0.125)
            if e in ("bn_stats", "bn_bwd", "bn_frozen") and M > 1000 and ms is None:
                # planted rows, exact in one bf16 / half plane, larger than the sum's allowance FLOOR * sum |terms|: one lost row is visible
                for r in reduce_rows(c):
                    x[r] = mean.sign() * 4.0 * (1 + (torch.arange(C) % 2))
                    dy[r] = 8.0
            self.x, self.dy = q(x, "x"), q(dy, "dy")
            self.gamma, self.beta = _randn(g, (C,), 0.5, 1.0), _randn(g, (C,), 0.5)
            self.scale, self.shift = _randn(g, (C,), 0.5, 1.0), _randn(g, (C,), 0.5)
            self.rmean, self.rvar = _randn(g, (C,), 0.3), torch.rand(C, generator=g) + 0.5
            x64 = self.x.double()
            self.mean = x64.mean(0).float()
            self.invstd = (1.0 / (x64.var(0, unbiased=False) + EPS32).sqrt()).float()
            self.dgamma0, self.dbeta0 = _randn(g, (C,)), _randn(g, (C,))
            if e == "bn_apply":
                self.res = q(_randn(g, (M, C)), "res") if c.res else None
            if e == "add_rows":
                self.a = self.x
                self.b = q(_randn(g, (M, C)), "b") if c.b else None
                self.mask = quantise(_randn(g, (M, C)), fmt, 1) if c.mask else None
                self.s1, self.s2 = {"none": (None, None), "one": (2.0 ** -3, None), "pair": (2.0 ** -3, 2.0 ** 2)}[c.scale]
        elif e == "bn_finalize":
            M, C, nb = c.M, c.C, c.nb
            sigma = torch.rand(C, generator=g) + 0.5
            mean = sigma * (torch.rand(C, generator=g) * 4 - 2)
            x = (_randn(g, (M, C)) * sigma + mean).double()
            rpb = cdiv(M, nb)
            part = torch.zeros(nb, C, 2, dtype=torch.float64)
            for b in range(nb):
                blk = x[b * rpb:(b + 1) * rpb]
                part[b, :, 0], part[b, :, 1] = blk.sum(0), (blk * blk).sum(0)
            self.part = part.float()                                   # (the partials ARE the operand: the reference sums these fp32 values)
            self.gamma, self.beta = _randn(g, (C,), 0.5, 1.0), _randn(g, (C,), 0.5)
            self.rmean, self.rvar = _randn(g, (C,), 0.3), torch.rand(C, generator=g) + 0.5
        elif e == "maxpool":
            N, H, W, C = c.N, c.H, c.W, c.C
            P = c.pl("x")
            nine = quantise(torch.tensor([-2.0, -1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0]) * (1.0 + (2.0 ** -9 + 2.0 ** -18 if P > 1 else 0.0)), fmt, P)
            idx = torch.randint(0, 9, (N, C, H, W), generator=g)
            neg = torch.randint(0, 4, (N, C, H, W), generator=g)
            idx[:, :, :3, :3] = neg[:, :, :3, :3]                      # all-negative windows at the padding: a kernel that reads the padding as 0 fails
            if H >= 6 and W >= 6:
                idx[:, :, H - 2:, W - 2:] = neg[:, :, H - 2:, W - 2:]
            self.x = nine[idx]
            OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
            self.dy = q(_randn(g, (N, C, OH, OW), 0.5, 0.125), "dy")
        elif e == "bilinear_fwd":
            self.x = q(_randn(g, (c.N, c.C, c.IH, c.IW)), "x")
        elif e == "bilinear_bwd":
            self.dy = q(_randn(g, (c.N, c.C, c.OH, c.OW), 0.5, 0.125), "dy")
            self.mask = quantise(_randn(g, (c.N, c.C, c.IH, c.IW)), fmt, 1) if c.mask else None
        elif e == "img_pack":
            self.img = _randn(g, (c.N, c.C, c.H, c.W), 60.0, 120.0)
        elif e in ("rescale", "rows_scale"):
            self.g = self._gradient(g, c.M, c.C, fmt, c.P)
            if e == "rescale":
                self._plant(c)
            self.s1, self.s2 = {"one": (2.0 ** -3, None), "pair": (2.0 ** -5, 2.0 ** 2), "unit": (2.0 ** -2, 2.0 ** 2), None: (None, None)}[c.get("scale")]
        elif e == "scale_multi":
            self.gs = [self._gradient(g, M, C, fmt, P) for M, C, P, _ in c.items]
            self.s1, self.s2 = {"one": (2.0 ** -3, None), "pair": (2.0 ** -5, 2.0 ** 2)}[c.scale]

    @staticmethod
    def _gradient(g, M, C, fmt, P):
        """background of the rescale family: magnitudes in [2^-6, 1): below 2^(T - 1) whatever the plane count, a power-of-two factor down to 2^-6
        keeps every plane clear of the half format's subnormals' rounding (the reference rounds each plane like the kernel in any case)"""
        v = (torch.rand(M, C, generator=g) * (1 - 2.0 ** -6) + 2.0 ** -6) * (2 * torch.randint(0, 2, (M, C), generator=g).float() - 1)
        return quantise(v * 0.99, fmt, P)

    def _plant(self, c):
        p = plant_chunk(c)
        C8 = c.C // 8
        r, ch = p // C8, (p % C8) * 8
        T = T_LOG2
        one_ulp = 2.0 ** (T - 1) * (2.0 ** -7 if c.fmt == "bf16" else 2.0 ** -10)          # of a value in [2^(T-1), 2^T), in plane 0
        e = 7 if c.plant in ("elem7", "lofavour") else 3
        val = {"big": 2.0 ** (T + 5) * 1.25, "pow2": 2.0 ** T, "pow2-ulp": 2.0 ** T - one_ulp, "small": 2.0 ** (T - 1) - one_ulp / 2, "zero": 0.0, "inf": INF}[c.value]
        if c.value == "zero":
            self.g.zero_()
            self.planted = None
            return
        if c.plant == "negative":
            val = -val
        if c.plant == "lofavour":
            # plane 0 rounds UP to 2^(T+3); the lower planes bring the sum back below it: the maximum of plane 0 alone would ask for 2^-4, the value for 2^-3
            val = float(quantise(torch.tensor(2.0 ** (T + 3) * (1 - (2.0 ** -10 if c.fmt == "bf16" else 2.0 ** -13))), c.fmt, c.P))
            assert float(split_planes(torch.tensor(val), c.fmt, c.P)[0]) == 2.0 ** (T + 3) and val < 2.0 ** (T + 3)
        self.g[r, ch + e] = val
        self.planted = (r, ch + e)


# ---- reference, bounds, mutants ---------------------------------------------------------------------------------------------------------------

class RowsOut:
    """an element-wise output [rows, C] in P planes of fmt: float64 reference, the float32 CPU evaluation, the bound of the module docstring"""

    def __init__(self, ref, f32, fmt, P, exact=False):
        self.ref, self.fmt, self.P, self.exact = ref, fmt, P, exact
        self.rms = float(ref.pow(2).mean().sqrt()) if ref.numel() else 0.0
        if exact:
            self.u = self.yard = self.allow = 0.0
            self.f32 = ref.float()
        else:
            self.u = u_out(fmt, P)
            self.yard = float((f32.double() - ref).abs().max()) if ref.numel() else 0.0
            self.allow = max(MARGIN * self.yard, FLOOR * self.rms)
            self.f32 = quantise(f32, fmt, P)                            # the float32 evaluation as the output planes would hold it

    def ratio(self, got, ref=None):
        """worst |got - ref| / bound over every element (inf where the bound is 0 and the element differs)"""
        ref = self.ref if ref is None else ref
        d = (got.double() - ref).abs()
        if not bool(torch.isfinite(got).all()):
            return INF
        if d.numel() == 0:
            return 0.0
        if self.exact:
            return INF if bool((d > 0).any()) else 0.0
        b = self.u * ref.abs() + self.allow
        r = torch.where(b > 0, d / b.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, INF), torch.zeros_like(d)))
        return float(r.max())


class VecOut:
    """a reduced quantity [C] (fp32 on the device): float64 reference, float32 evaluation, bound"""

    def __init__(self, ref, f32, bound):
        self.ref, self.f32, self.bound = ref, f32, bound

    def ratio(self, got, ref=None):
        ref = self.ref if ref is None else ref
        if not bool(torch.isfinite(got).all()):
            return INF
        d = (got.double() - ref).abs()
        r = torch.where(self.bound > 0, d / self.bound.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, INF), torch.zeros_like(d)))
        return float(r.max()) if r.numel() else 0.0


def sum_bound(t64, t32, extra=None):
    """densecases.stats_reference's rule for a column sum: (float64 sum, float32 evaluation, bound)"""
    s64, s32 = t64.sum(0), t32.sum(0)
    b = torch.maximum(MARGIN * (s32.double() - s64).abs(), FLOOR * t64.abs().sum(0))
    return s64, s32, (b + extra if extra is not None else b)


def rows_of(t):
    n, c, h, w = t.shape
    return t.permute(0, 2, 3, 1).reshape(n * h * w, c)


def pool_scan(x, ninf):
    """MaxPool2d(3, 2, 1) restated: FIRST maximum in (kh, kw) scan order wins.  Returns (best, arg) [N, C, OH, OW]; arg = kh * 3 + kw"""
    N, C, H, W = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = F.pad(x, (1, 2, 1, 2), value=ninf)
    best = torch.full((N, C, OH, OW), ninf, dtype=x.dtype)
    arg = torch.full((N, C, OH, OW), -1, dtype=torch.int64)
    for kh in range(3):
        for kw in range(3):
            v = xp[:, :, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2][:, :, :OH, :OW]
            iy = (torch.arange(OH) * 2 - 1 + kh).view(1, 1, OH, 1)
            ix = (torch.arange(OW) * 2 - 1 + kw).view(1, 1, 1, OW)
            valid = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            upd = valid & ((v > best) | (arg < 0))
            best = torch.where(upd, v, best)
            arg = torch.where(upd, torch.full_like(arg, kh * 3 + kw), arg)
    return best, arg


def pool_scatter(dy, arg, H, W):
    """dx of the max-pool: every output's dy goes to the input pixel its winning tap names"""
    N, C, OH, OW = dy.shape
    dxp = torch.zeros(N, C, 2 * OH + 2, 2 * OW + 2, dtype=dy.dtype)
    for kh in range(3):
        for kw in range(3):
            dxp[:, :, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2] += dy * (arg == kh * 3 + kw)
    return dxp[:, :, 1:1 + H, 1:1 + W]


class Reference:
    """float64 reference of a case with its bounds.  rows: {name: RowsOut}; vecs: {name: VecOut}; scalars: {name: exact value} (rescale family).
    mutants(): the reference with the smallest unit a kernel can lose -- see the module docstring."""

    def __init__(self, c, o=None):
        self.c, self.o = c, o or Operands(c)
        self.rows, self.vecs, self.bits = {}, {}, {}
        self._drop = None
        getattr(self, "_" + c.entry)(c, self.o)

    # -- element-wise -------------------------------------------------------------------------------------------------------------------------
    def _bn_apply(self, c, o):
        def ev(dt):
            v = o.x.to(dt) * o.scale.to(dt) + o.shift.to(dt)
            if o.res is not None:
                v = v + o.res.to(dt)
            return F.relu(v) if c.relu else v
        self.rows["y"] = RowsOut(ev(torch.float64), ev(torch.float32), c.fmt, c.pl("y"))

    def _bn_frozen_scale(self, c, o):
        self.rows["dx"] = RowsOut(o.dy.double() * o.scale.double(), o.dy * o.scale, c.fmt, c.pl("y"))

    def _add_rows(self, c, o):
        def ev(dt):
            v = o.a.to(dt)
            if o.b is not None:
                v = v + o.b.to(dt)
            if o.s1 is not None:
                v = v * (o.s1 * (o.s2 if o.s2 is not None else 1.0))
            return v * (o.mask > 0) if o.mask is not None else v
        self.rows["y"] = RowsOut(ev(torch.float64), ev(torch.float32), c.fmt, c.pl("y"))

    def _bilinear_fwd(self, c, o):
        ev = lambda dt: rows_of(F.interpolate(o.x.to(dt), size=(c.OH, c.OW), mode="bilinear", align_corners=False))
        self.rows["y"] = RowsOut(ev(torch.float64), ev(torch.float32), c.fmt, c.pl("y"))

    def _bilinear_bwd(self, c, o):
        def ev(dt):
            x = torch.zeros(c.N, c.C, c.IH, c.IW, dtype=dt, requires_grad=True)
            y = F.interpolate(x, size=(c.OH, c.OW), mode="bilinear", align_corners=False)
            gx, = torch.autograd.grad(y, x, o.dy.to(dt))
            return rows_of(gx * (o.mask > 0) if o.mask is not None else gx)
        self.rows["dx"] = RowsOut(ev(torch.float64), ev(torch.float32), c.fmt, c.pl("y"))

    def _img_pack(self, c, o):
        v = F.pad(o.img, (0, 0, 0, 0, 0, 8 - c.C))
        self.rows["y"] = RowsOut(rows_of(v.double()), rows_of(v), c.fmt, c.P)
        self.pad_cols = slice(c.C, 8)          # exact zeros, compared bit for bit

    def _maxpool(self, c, o):
        y64, arg = pool_scan(o.x.double(), -INF)
        assert torch.equal(y64, F.max_pool2d(o.x.double(), 3, 2, 1))
        self.rows["y"] = RowsOut(rows_of(y64), None, c.fmt, c.pl("x"), exact=True)
        self.arg = rows_of(arg).to(torch.uint8)
        self.rows["dx"] = RowsOut(rows_of(pool_scatter(o.dy.double(), arg, c.H, c.W)), rows_of(pool_scatter(o.dy, arg, c.H, c.W)), c.fmt, c.pl("y"))

    # -- reductions ---------------------------------------------------------------------------------------------------------------------------
    def _bn_stats(self, c, o, part=None):
        M, C = c.M, c.C
        if part is None:
            x64 = o.x.double()
            s, s32, bs = sum_bound(x64, o.x)
            q, q32, bq = sum_bound(x64 * x64, o.x * o.x)
            self._drop = lambda r: derive(s - x64[r], q - x64[r] ** 2)
        else:
            p64 = part.double()
            s, s32, bs = sum_bound(p64[:, :, 0], part[:, :, 0])
            q, q32, bq = sum_bound(p64[:, :, 1], part[:, :, 1])
            self._drop = lambda b: derive(s - p64[b, :, 0], q - p64[b, :, 1])
        run = c.running
        g64, b64, rm, rv = o.gamma.double(), o.beta.double(), o.rmean.double(), o.rvar.double()

        def derive(s, q, dt=torch.float64):
            f = lambda t: t.to(dt)
            mu = f(s) / M
            var = (f(q) / M - mu * mu).clamp_min(0)
            is_ = 1.0 / (var + EPS32).sqrt()
            sc = f(o.gamma) * is_
            d = {"mean": mu, "invstd": is_, "scale": sc, "shift": f(o.beta) - mu * sc}
            if run:
                unb = var * M / (M - 1) if M > 1 else var
                d["running_mean"], d["running_var"] = 0.9 * f(o.rmean) + 0.1 * mu, 0.9 * f(o.rvar) + 0.1 * unb
            return d
        ref, f32 = derive(s, q), derive(s32, q32, torch.float32)
        mu, is_, sc = ref["mean"], ref["invstd"], ref["scale"]
        dmu = bs / M
        dvar = bq / M + 2 * mu.abs() * bs / M
        dis = 0.5 * is_ ** 3 * dvar
        dsc = g64.abs() * dis
        bound = {"mean": dmu + U32 * mu.abs(), "invstd": dis + U32 * is_, "scale": dsc + 2 * U32 * sc.abs(),
                 "shift": mu.abs() * dsc + sc.abs() * dmu + 3 * U32 * (b64.abs() + (mu * sc).abs())}
        if run:
            bound["running_mean"] = 0.1 * dmu + 3 * U32 * (rm.abs() + mu.abs())
            bound["running_var"] = 0.1 * dvar * (M / (M - 1) if M > 1 else 1) + 3 * U32 * (rv.abs() + ref["running_var"].abs())
        self.vecs = {k: VecOut(ref[k], f32[k], bound[k]) for k in ref}
        self.sums = (s, q, bs, bq)

    def _bn_finalize(self, c, o):
        self._bn_stats(c, o, part=o.part)

    def _bwd_sums(self, c, o, mu32, is64, is_err):
        """(sum dy, sum dy * xhat) with bounds; xhat = (x - mu) * is evaluated in fp32 by the kernels: 2^-23 (|x| + |mu|) is of rounding per term,
        + is_err (relative) where `is` itself is computed in fp32 on the device"""
        x64, dy64 = o.x.double(), o.dy.double()
        xh = (x64 - mu32.double()) * is64
        xh32 = (o.x - mu32) * is64.float()
        xerr = 2.0 ** -23 * (x64.abs() + mu32.double().abs()) * is64 + is_err * xh.abs()
        s, s32, bs = sum_bound(dy64, o.dy)
        sx, sx32, bsx = sum_bound(dy64 * xh, o.dy * xh32, (dy64.abs() * xerr).sum(0))
        if c.get("parts"):                       # every partial is rounded to fp32 once more on the host
            bs, bsx = bs + U32 * dy64.abs().sum(0), bsx + U32 * (dy64 * xh).abs().sum(0)
        return xh, xh32, (s, s32, bs), (sx, sx32, bsx)

    def _grads(self, c, o, s, sx, bs, bsx, dt):
        f = lambda t: t.to(dt)
        acc = bool(c.accumulate)
        return {"dgamma": f(sx) + (f(o.dgamma0) if acc else 0), "dbeta": f(s) + (f(o.dbeta0) if acc else 0)}

    def _grad_bounds(self, c, o, s, sx, bs, bsx):
        acc = 1.0 if c.accumulate else 0.0
        return {"dgamma": bsx + 2 * U32 * (sx.abs() + acc * o.dgamma0.double().abs()), "dbeta": bs + 2 * U32 * (s.abs() + acc * o.dbeta0.double().abs())}

    def _bn_bwd(self, c, o):
        M = c.M
        is64 = o.invstd.double()
        xh, xh32, (s, s32, bs), (sx, sx32, bsx) = self._bwd_sums(c, o, o.mean, is64, 0.0)
        a64 = o.gamma.double() * is64

        def derive(s, sx, dt=torch.float64):
            f = lambda t: t.to(dt)
            a = f(o.gamma) * f(o.invstd)
            d = self._grads(c, o, s, sx, bs, bsx, dt)
            d["coef"] = torch.stack([a, -a * f(sx) / M, -a * f(s) / M])
            return d
        ref, f32 = derive(s, sx), derive(s32, sx32, torch.float32)
        bound = self._grad_bounds(c, o, s, sx, bs, bsx)
        bound["coef"] = torch.stack([U32 * a64.abs(), a64.abs() * bsx / M + 3 * U32 * ref["coef"][1].abs(), a64.abs() * bs / M + 3 * U32 * ref["coef"][2].abs()])
        self.vecs = {k: VecOut(ref[k], f32[k], bound[k]) for k in ref}
        x64, dy64 = o.x.double(), o.dy.double()
        self._drop = lambda r: derive(s - dy64[r], sx - dy64[r] * xh[r])
        k64, k32 = ref["coef"], f32["coef"]
        self.rows["dx"] = RowsOut(k64[0] * dy64 + k64[1] * xh + k64[2], k32[0] * o.dy + k32[1] * xh32 + k32[2], c.fmt, c.pl("y"))
        self.sums = (s, sx, bs, bsx)

    def _bn_frozen(self, c, o):
        is64 = 1.0 / (o.rvar.double() + EPS32).sqrt()
        xh, xh32, (s, s32, bs), (sx, sx32, bsx) = self._bwd_sums(c, o, o.rmean, is64, 4 * U32)          # is = 1.f / sqrtf(rvar + eps): three roundings
        derive = lambda s, sx, dt=torch.float64: self._grads(c, o, s, sx, bs, bsx, dt)
        ref, f32 = derive(s, sx), derive(s32, sx32, torch.float32)
        bound = self._grad_bounds(c, o, s, sx, bs, bsx)
        self.vecs = {k: VecOut(ref[k], f32[k], bound[k]) for k in ref}
        dy64 = o.dy.double()
        self._drop = lambda r: derive(s - dy64[r], sx - dy64[r] * xh[r])
        self.rows["dx"] = RowsOut(dy64 * o.scale.double(), o.dy * o.scale, c.fmt, c.pl("y"))
        self.sums = (s, sx, bs, bsx)

    # -- the rescale family: bit-exact --------------------------------------------------------------------------------------------------------
    @staticmethod
    def rescale_factor(g, fmt, P, T=T_LOG2):
        """kg_rows_rescale's r: max |sum of the planes| (summed lowest plane first in fp32: exact) -> frexp -> 2^min(T - e, 0), at least 2^-60;
        1 for an all-zero or non-finite maximum"""
        m = float(g.abs().max()) if g.numel() else 0.0
        if m == 0.0 or not math.isfinite(m):
            return 1.0
        e = math.frexp(m)[1]
        return 2.0 ** max(min(T - e, 0), -60)

    @staticmethod
    def scaled_buffer(v, fmt, P, s, sliced=True):
        """the buffer after rows_scale_kernel: every plane * s, rounded to the format (exact for a power of two clear of the subnormals)"""
        buf, c0, ctot = layout(v, fmt, P, sliced)
        C = v.shape[1]
        if s != 1.0:
            for p in range(P):
                sl = slice(p * ctot + c0, p * ctot + c0 + C)
                buf[:, sl] = (buf[:, sl].float() * s).to(DT[fmt])
        return buf

    def _rescale(self, c, o):
        r = self.rescale_factor(o.g, c.fmt, c.P)
        cum_in = (0.25, 4.0)
        cum = float(torch.tensor(cum_in[0], dtype=torch.float32) * r)
        self.cum_in = cum_in
        self.scalars = {"r": r, "cum": cum, "inv": float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(cum, dtype=torch.float32))}
        self.buffer = self.scaled_buffer(o.g, c.fmt, c.P, r)
        if o.planted is not None:
            g2 = o.g.clone()
            g2[o.planted] = 0.0
            self.r_without_plant = self.rescale_factor(g2, c.fmt, c.P)
        if c.plant == "lofavour":
            self.r_of_plane0 = self.rescale_factor(split_planes(o.g, c.fmt, c.P)[0], c.fmt, 1)

    def _rows_scale(self, c, o):
        self.s = o.s1 * (o.s2 if o.s2 is not None else 1.0)
        self.buffer = self.scaled_buffer(o.g, c.fmt, c.P, self.s)

    def _scale_multi(self, c, o):
        self.s = o.s1 * (o.s2 if o.s2 is not None else 1.0)
        self.buffers = [self.scaled_buffer(v, c.fmt, P, self.s, sliced) for v, (M, C, P, sliced) in zip(o.gs, c.items)]

    # -- mutants ------------------------------------------------------------------------------------------------------------------------------
    def row_mutants(self, name):
        """[(kind, row, column slice, values)]: one 16-byte chunk taken from the neighbouring row; one chunk left at the fill value.  Positions are
        seeded; a neighbour chunk must differ from the chunk it replaces somewhere (else nothing was lost), which the bound plays no part in."""
        out = self.rows[name]
        ref = out.ref
        R, C = ref.shape
        g = torch.Generator().manual_seed(self.c.seed + 17)
        muts = []
        r, ch = int(torch.randint(0, R, (1,), generator=g)), 8 * int(torch.randint(0, C // 8, (1,), generator=g))
        sl = slice(ch, ch + 8)
        muts.append(("fill", r, sl, torch.full((8,), FILL, dtype=torch.float64)))
        for k in range(R * (C // 8)):
            rr, cc = (r + k // (C // 8)) % R, (ch + 8 * (k % (C // 8))) % C
            nb = rr + 1 if rr + 1 < R else rr - 1
            if nb >= 0 and not torch.equal(ref[rr, cc:cc + 8], ref[nb, cc:cc + 8]):
                muts.append(("neighbour", rr, slice(cc, cc + 8), ref[nb, cc:cc + 8].clone()))
                break
            if k > 4096:
                break
        return muts

    def row_mutant_ratio(self, name, mut):
        _, r, sl, vals = mut
        out = self.rows[name]
        return out.ratio(vals.view(1, -1), out.ref[r:r + 1, sl])

    def drop_mutants(self):
        """reductions: {row (or partial block) dropped: {name: float64 value}}"""
        if self.c.entry == "bn_finalize":
            return {b: self._drop(b) for b in sorted({0, (self.c.nb - 1) // 2})}          # (the last partial may cover no row)
        return {r: self._drop(r) for r in reduce_rows(self.c)}

    def vec_ratio(self, values):
        return max(self.vecs[k].ratio(values[k].float() if values[k].dtype != torch.float64 else values[k]) for k in self.vecs)


def host_partials(o, c, nbp, rs):
    """[nbp][C][2] fp32 partials of (sum dy, sum dy * xhat) over blocks of ceil(M / nbp) rows, taken BEFORE dy was multiplied by rs (a power of two):
    what kg_conv_bstats_begin's armed launch leaves for kg_bn_bwd"""
    x64, dy64 = o.x.double(), o.dy.double() / rs
    xh = (x64 - o.mean.double()) * o.invstd.double()
    rpb = cdiv(c.M, nbp)
    part = torch.zeros(nbp, c.C, 2, dtype=torch.float64)
    for b in range(nbp):
        sl = slice(b * rpb, (b + 1) * rpb)
        part[b, :, 0], part[b, :, 1] = dy64[sl].sum(0), (dy64[sl] * xh[sl]).sum(0)
    return part.float()


def onepass_f32(x, nb, rpb):
    """The float32 evaluation of the kernels' OWN one-pass statistics: sum x and sum x^2 in float32 in colreduce_kernel's decomposition (per block: 32
    row lanes that stride by 32, then the 32 lane sums one after the other), the block partials combined in double, var = q / M - mean^2 in double
    (bn_finalize_train_kernel).  Returns (mean, invstd) float64."""
    M, C = x.shape
    S, Q = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    for b in range(nb):
        blk = x[b * rpb:min((b + 1) * rpb, M)].float()
        pad = (-blk.shape[0]) % 32
        blk = torch.cat([blk, torch.zeros(pad, C)]).view(-1, 32, C)
        s, q = torch.zeros(32, C), torch.zeros(32, C)
        for t in range(blk.shape[0]):
            s, q = s + blk[t], q + blk[t] * blk[t]
        ts, tq = torch.zeros(C), torch.zeros(C)
        for k in range(32):
            ts, tq = ts + s[k], tq + q[k]
        S, Q = S + ts.double(), Q + tq.double()
    mu = S / M
    var = (Q / M - mu * mu).clamp_min(0)
    return mu, 1.0 / (var + EPS32).sqrt()
