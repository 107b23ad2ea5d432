"""Which kernel a convolution runs on: the host-side routing rules, as plain functions over integers and booleans.

ops (the launches), seg (the ragged launches) and the oracles (oracle/densecases.py, oracle/segcases.py: the planned launch classes the
route tests compare the observed launches with) all ask this module; none of them keeps a predicate of its own.  No tensors, no library:
a caller extracts the primitives (sizes, plane counts, which operands exist) and gets a tuple back.  What the LIBRARY decides after that
(kernel variants, channel / K splits inside an entry point) is csrc's business and is restated, for the tests only, in the oracles.

Vocabulary: cin_pad = channels of one plane of the packed weight's input; xcols = columns of the x rows tensor; w_rows = rows of the packed
weight; xP / wP / yP / rP = planes of x, the packed weight, y and res (1 where the operand is absent); rows_out = the output is a rows tensor
(False: fp32 export); armed = the statistics side channel is claimed for the next launch (ops.conv_stats_armed)."""
import functools
import math

CONV_TINY_WGS = 96        # regular workgroups below which a launch goes to the split-K kernel (0 = never)
CONV_TINY_TILES = 384
USE_WS = True             # the weight-stationary 64 -> 64 kernel (conv3_ws.hip); tools/ws_probe.py measures the launch without it
WGRAD_RING_WGS = 256      # workgroups of a ring launch (one 96 / 144 KB workgroup per CU)
RAGGED_FILL = 0.35        # ragged launches: rows / (tiles * pixels per tile) from which the LDS-halo kernels pay (tiny deep-level crops stay on the gather kernels)
WGRAD_TR = [True]         # mirror of the library's kg_set_wgrad_tr switch (ops.set_wgrad_tr keeps the two in step)


def vplanes(xP, wP):
    """number of virtual channel planes of a packed weight = kept products x_i * w_j, i + j < max(xP, wP) (csrc/kg_common.h kg_plane_pairs)"""
    T = max(xP, wP)
    return sum(1 for i in range(xP) for j in range(wP) if i + j < T)


def round_up(a, b):
    return (a + b - 1) // b * b


def halo_entry(k, cin_pad, cout, xP, wP, yP, rP, rows_out, res, mask, flip, oscale, armed, ragged, tiles8, tiles16):
    """Entry point of a launch that goes to the LDS-halo family (ops.conv_halo), dense or ragged.  ragged: the launch walks a table of 16 x 32
    tiles; tiles8 / tiles16: it also has the table of 8- / 16-pixel tiles that conv3_ws / conv3_c64 walk instead."""
    if (USE_WS and k == 3 and cin_pad == 64 and cout == 64 and xP == 2 and wP == 2 and yP <= 2 and rows_out and not res and not mask and not flip
            and not oscale and not armed and (tiles8 or not ragged)):
        return "kg_conv3x3_ws"         # full-resolution 64 -> 64 convs on hi + lo planes: weights in registers, two workgroups per CU
    if k == 3 and cin_pad == 64 and xP == wP == yP == rP == 1 and not oscale and rows_out and (tiles16 or not ragged):
        return "kg_conv3x3_c64"        # 64 single-plane input channels: persistent kernel with resident weights and double-buffered halos
    return "kg_conv2d_halo"


def can_1x1(k, stride, pad, cin_pad, xcols, w_rows, planed, rows_out, same_rows):
    """1x1 stride-1 conv as a streaming GEMM over the rows of x (kg_conv1x1).  planed: x, the weight, y or res has more than one plane;
    same_rows: y has as many rows as x (asked for 1x1 convs only)."""
    if planed:
        return False      # split-bf16 planes: the gather kernel (conv_gather.hip) walks the virtual channels
    if cin_pad >= 192 and w_rows > 64:
        return False      # compute-heavy 1x1 (K >= 192, Cout > 64): the LDS-ring gather kernel (conv_gather.hip) is faster
    return k == 1 and stride == 1 and pad == 0 and rows_out and cin_pad % 64 == 0 and 64 <= cin_pad <= 1024 and xcols >= cin_pad and same_rows


def dense_kind(M, N, OH, OW, k, stride, pad, cin_pad, xcols, w_rows, planed, cout, rows_out, res, mask, oscale, same_rows, tile, tiny):
    """Dense conv forward or input gradient of N images with OH x OW outputs (M = N * OH * OW rows): what ops.conv_auto does and returns --
    "tiny" (split-K kernel behind kg_conv2d_igemm, tile 6), "halo" (ops.conv_halo: halo_entry picks the entry point), "1x1", "igemm".
    tile: the caller's tile override of kg_conv2d_igemm (0 = none); tiny: the split-K kernel is allowed (False for a conv that is armed
    for BatchNorm statistics: that epilogue lives in the regular kernels)."""
    fits = cin_pad % 64 == 0 and xcols >= cin_pad      # whole 64-channel chunks; halo: stride-1 "same" 3x3 / 7x7 over such an input
    halo = fits and stride == 1 and k in (3, 7) and pad == k // 2 and (rows_out or not (res or mask))
    if tiny and tile == 0 and CONV_TINY_WGS and rows_out and fits and k * k <= 9:
        wgs = (N * math.ceil(OH / 16) * math.ceil(OW / 32) * math.ceil(cout / 64)) if halo else math.ceil(M / 256) * math.ceil(cout / 128)
        tiles = math.ceil(M / 64) * math.ceil(cout / 64)
        # (no operand reuse inside a 64 x 64 tile: measured 1.75 ns per (tile, K unit) against 0.85 us per K unit of a regular workgroup
        # -- past ~400 tiles the regular kernel's single round is as fast)
        if wgs < CONV_TINY_WGS and wgs < tiles <= CONV_TINY_TILES:
            return "tiny"
    if halo:
        return "halo"
    if not oscale and can_1x1(k, stride, pad, cin_pad, xcols, w_rows, planed, rows_out, same_rows):
        return "1x1"
    return "igemm"


def dense_conv(M, N, OH, OW, k, stride, pad, cin_pad, xcols, w_rows, xP, wP, yP, rP, cout, transposed, rows_out, res, mask, oscale, same_rows,
               tile, tiny, armed):
    """(kind, entry point) of the dense conv ops.conv_auto is given.  ops does NOT call this: conv_auto asks dense_kind, and conv_halo then asks
    halo_entry with the arguments below (flip = transposed, no tile tables).  The oracles and tests ask here; change the two paths together."""
    kind = dense_kind(M, N, OH, OW, k, stride, pad, cin_pad, xcols, w_rows, xP > 1 or wP > 1 or yP > 1 or rP > 1, cout, rows_out, res, mask, oscale,
                      same_rows, tile, tiny)
    if kind == "halo":
        return kind, halo_entry(k, cin_pad, cout, xP, wP, yP, rP, rows_out, res, mask, transposed, oscale, armed, False, False, False)
    return kind, "kg_conv1x1" if kind == "1x1" else "kg_conv2d_igemm"


def ragged_conv(k, M, tiles32, cin_pad, xcols, w_rows, planed, rows_out, same_rows):
    """Ragged conv or input gradient over the M rows of a box population (seg.SegBranch.rconv): "halo" / "1x1" / "gather".
    tiles32: entries of the launch's table of 16 x 32 tiles (0: none) -- the halo kernel pays when its tiles are mostly full."""
    if k == 3 and tiles32 > 0 and cin_pad % 64 == 0 and xcols >= cin_pad and M >= RAGGED_FILL * tiles32 * 512:
        return "halo"
    if k == 1 and can_1x1(1, 1, 0, cin_pad, xcols, w_rows, planed, rows_out, same_rows):
        return "1x1"
    return "gather"


def ragged_wgrad_halo(k, M, tiles16):
    """Ragged weight gradient (seg.SegBranch.conv_bwd): True = kg_conv2d_wgrad_halo over the table of tiles16 16 x 16 tiles (None: no table)"""
    return k == 3 and tiles16 is not None and M >= RAGGED_FILL * tiles16 * 256


def wgrad_splits(M, cin_lim, cout_lim, taps, nelem):
    """pixel splits of kg_conv2d_wgrad, sized for the tile the library will pick: the condition below is kg_conv2d_wgrad's own
    (conv_wgrad.hip: ring iff transpose reads && cin >= 128 && cout >= 64, else 64 x 64 tiles)"""
    chunks = math.ceil(M / 64)
    if WGRAD_TR[0] and cin_lim >= 128 and cout_lim >= 64:
        # conv_wgrad_ring_kernel (256 x 128 tiles, or 128 x 128 below 256 couts; 144 / 96 KB of LDS: one workgroup per CU): one round of at
        # most 256 workgroups
        base = math.ceil(cin_lim / 128) * math.ceil(cout_lim / (256 if cout_lim >= 256 else 128)) * taps
        s = max(1, min(WGRAD_RING_WGS // base if base <= WGRAD_RING_WGS else 1, max(1, chunks // 3)))
        while s > 1 and s * nelem * 4 > (768 << 20):
            s -= 1
        return s
    base = math.ceil(cin_lim / 64) * math.ceil(cout_lim / 64) * taps
    s = max(1, min(math.ceil(2048 / base), max(1, chunks // 4)))
    while s > 1 and s * nelem * 4 > (768 << 20):
        s -= 1
    return s


@functools.lru_cache(maxsize=4096)      # (the search walks up to 2048 candidates; ~110 calls per step with a few dozen distinct shapes)
def halo_wgrad_splits(nblk, tiles, cit, taps, nelem, cus=256):
    """Pixel splits of kg_conv2d_wgrad_halo: one workgroup per CU is resident (2 x 47..78 KB of LDS + ~250 VGPRs x 8 waves), so
    the launch runs in ceil(nblk * S / 256) rounds; pick S by a small cost model (round count x tiles per workgroup + per-workgroup
    prologue / partial write + the reduction's bytes) instead of a fixed 2 rounds -- 192 x 2 = 384 workgroups is 1.5 rounds."""
    tile_us = 256 * 64 * cit * taps * 2 / 5.3e6          # one 16x16 tile at ~1.35 PFLOP/s / 256 CUs
    best, best_t = 1, None
    for S in range(1, max(1, min(tiles, 2048 // nblk if nblk <= 2048 else 1)) + 1):
        if S > 1 and S * nelem * 4 > (768 << 20):
            break
        rounds = math.ceil(nblk * S / cus)
        t = rounds * (math.ceil(tiles / S) * tile_us + 10.0) + S * nelem * 8 / 3e6
        if S >= 8 and S % 8 == 0:
            t *= 0.97                                    # multiples of 8 enable the kernel's XCD-aware block mapping
        if best_t is None or t < best_t:
            best, best_t = S, t
    return best


def wgrad(M, N, H, W, k, stride, pad, cin, cout, xcols, dcols, xP, dP, mode, one_grad, accumulate, tiles16, bias_out):
    """Weight gradient of a conv (ops.conv_wgrad): (kind, cin_lim, cout_lim, cit, nblk, S, fused_bias).
    kind "im2col": the stem (cin <= 4, 5x5 / 7x7) as im2col + ONE 1x1 weight gradient, which the caller routes again -- the other fields are 0;
    "halo": kg_conv2d_wgrad_halo over the 16 x 16 tiles of N images of H x W (mode 0) or of the ragged table of tiles16 entries (mode 2), cit
    input channels per workgroup, nblk channel blocks, fused_bias = the kernel sums the bias gradient as well; "gather": kg_conv2d_wgrad.
    S = pixel splits.  N: None for a launch that is not N dense images; one_grad: a single gradient tensor (no fused heads)."""
    if mode == 0 and N is not None and cin <= 4 and k * k >= 25 and one_grad and not accumulate:
        return "im2col", 0, 0, 0, 0, 0, False
    cin_lim, cout_lim = min(round_up(cin, 8), xcols), min(round_up(cout, 8), dcols)
    nelem = cout * k * k * cin
    np_ = vplanes(xP, dP)                  # plane products: every kept one is one more pass over the pixels
    if stride == 1 and k in (3, 7) and pad == k // 2 and ((mode == 0 and N is not None) or (mode == 2 and tiles16 is not None)):
        fused_bias = bias_out and xP == 1 and dP == 1      # (planed operands: the all-ones unit would count every plane product)
        cit = (32 if (cout_lim <= 16 and cin_lim >= 32 and fused_bias) else 16) if k == 7 else 64      # input channels per workgroup (wgrad_halo.hip)
        nblk = math.ceil(cin_lim / cit) * math.ceil(cout_lim / 64)
        tiles = tiles16 if tiles16 is not None else N * math.ceil(H / 16) * math.ceil(W / 16)
        return "halo", cin_lim, cout_lim, cit, nblk, halo_wgrad_splits(nblk, tiles * np_, cit, k * k, nelem), fused_bias
    return "gather", cin_lim, cout_lim, 0, 0, wgrad_splits(M * np_, cin_lim, cout_lim, k * k, nelem), False
