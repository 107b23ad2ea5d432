// label_common.h -- what the label-map kernels share (instances.hip, tiling.hip, labelmetrics.hip, components.hip, measure.hip,
// distance.hip, neighbours.hip, runlengths.hip, contours.hip, polygons.hip, hulls.hip, intensity.hip, split.hip, texture.hip,
// thinning.hip, boundaries.hip, crops.hip, linking.hip; paste.hip for the bit-mask leading dimension; sampleprep.hip for the job box and the host
// checks of kg_sp_warp_labels): wave reductions, the clamped job box and its walk, the block combine of four wave partials, the
// row-segment run walk, per-image ranges passed by value, and the host argument checks -- among them the side bound KG_LABEL_MAX_SIDE,
// the block that opens a per-job entry (kg_check_job_stack), the image check (kg_check_image) and the overlap test (kg_apart).
// Integers only, plain C++ and vector memory operations only.
//
// INDEX RULE of the family.  Every entry validates on the host before any HIP call and never synchronises; the number of launches does
// not depend on a count read from the device; every output element is written.  No address in a kernel depends on a value read from
// device memory, with six kinds of exception, each bounded where it is made:
//   - a job table (a device table the caller wrote): its box is clamped to the map BEFORE any address is formed (kg_job_box), and any
//     other index it carries is used only inside an unsigned range predicate that empties the box when it fails, so even a wrong table
//     cannot make a kernel leave its buffers.  kg_label_crops (crops.hip) is of this kind without a box: the sampling positions of its
//     job table are int64 sums of the table's coefficients, img is used inside (unsigned)img < (unsigned)nimg, and every tap (y, x) only
//     inside the unsigned 64-bit predicates (unsigned long long)y < H and (unsigned long long)x < W, formed BEFORE any narrowing; a tap
//     that fails them is the fill value, so extreme coefficients and far origins cannot leave the buffers either.  kg_sp_warp_labels
//     (sampleprep.hip) is of this kind with the box as a predicate: img selects an image record only inside (unsigned)img < (unsigned)N,
//     the clamped box only gates the load, and the load's address comes from the output pixel's own source index (sp_src);
//   - a row a label selects (kg_label_stats, kg_component_stats / remap, the union-find parents): stated in labelmetrics.hip and
//     components.hip, the index is formed only inside (unsigned)(v - 1) < (unsigned)n;
//   - the run slot of kg_label_runs (runlengths.hip): an offset of the job table plus a prefix count of predicates -- not a label value --
//     and the store happens only inside the 64-bit unsigned predicate slot < R.  (kg_runs_paint reads a row only at a binary-search
//     position in [0, R).)  kg_label_contours (contours.hip) stores the same way: ring slot and vertex offset are offsets of the job
//     table plus prefix counts, inside slot < R and first + k < V; and so does kg_label_hulls (hulls.hip): the vertex slot is vert_at of
//     the job table plus a prefix count, inside k < cap and vert_at + k < V; the d2 slot of kg_label_border_d2 (boundaries.hip) is of
//     this kind too: first of the job table plus a prefix count, inside first + k < D;
//   - the tracer of contours.hip: its position is an LDS bit index that depends on bits derived from labels.  It is bounded by
//     construction (a crack touches a P pixel of the box) and by an explicit clamp to [0, h] x [0, w] after every step.  No GLOBAL
//     address depends on a label there either;
//   - the two table levels of kg_polygons_fill (polygons.hip), both written by the caller: tile_ptr[t], tile_ptr[t + 1] are used only as a
//     range clamped inside [0, n_items] (a decreasing pair is an empty range), and an item's edge_first, edge_count only inside the 64-bit
//     unsigned predicates first <= E and count <= E - first, which empty the item when they fail.  No address depends on an edge
//     coordinate, a value or a row: a wrong table gives wrong pixels and cannot reach outside edges, items, out or cover.
//   - the LDS histogram of intensity.hip (kg_label_quantiles, kg_label_histograms): an LDS bin index formed from a PIXEL VALUE, the first
//     of the family.  It is bounded by construction: `& 255` (after min(., 255) where the last bin collects) immediately before use, inside
//     int [256]; the low-byte histogram a rank selected is an LDS row index used only inside (unsigned)s < (unsigned)KEEP.  No GLOBAL
//     address depends on a pixel or label value there either.  The co-occurrence matrices of texture.hip (kg_label_glcm) are of the same
//     kind: the LDS index i * L + j is formed from two pixel LEVELS, each bounded by min(., L - 1) immediately before use, inside
//     int [4][1024] with L <= 32; its staged bytes are indexed by box-local coordinates alone.
// Labels and pixel values are otherwise predicates, summands and stored values only.  kg_label_split (split.hip) adds NO exception: its
// LDS state is indexed by box-local coordinates alone, never by a label, a seed or a rank, and nseeds / first_new of its job table are a
// predicate bound and a stored value.  kg_label_thin (thinning.hip) adds NO exception either: its two LDS bitmaps are indexed by box-local
// coordinates alone (plus a fixed offset inside the zero halo), the predicate of its store is an LDS bit and the address a box coordinate.
#pragma once
#include "kg_common.h"
#include <limits.h>

// ---- wave reductions (64 lanes, every lane gets the result) ----------------------------------------------------------------------------
__device__ __forceinline__ int kg_wave_sum(int v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ long long kg_wave_sum(long long v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int kg_wave_min(int v) {
    for (int o = 32; o; o >>= 1) { const int t = __shfl_xor(v, o); v = t < v ? t : v; }
    return v;
}
__device__ __forceinline__ int kg_wave_max(int v) {
    for (int o = 32; o; o >>= 1) { const int t = __shfl_xor(v, o); v = t > v ? t : v; }
    return v;
}

// ---- the clamped box of a job and its walk ----------------------------------------------------------------------------------------------
// jb = the (y1, x1, y2, x2) of a job row, half-open.  The box is clamped to the H x W map first; an empty or inverted box gets
// h = w = 0 and reads nothing.  (label_measure_kernel keeps its own copy of the clamp and the walk: measure.hip says why.)
struct KgBox { int y1, x1, h, w; };
__device__ __forceinline__ KgBox kg_job_box(const int* jb, int H, int W) {
    int y1 = jb[0], x1 = jb[1], y2 = jb[2], x2 = jb[3];
    y1 = y1 < 0 ? 0 : y1; x1 = x1 < 0 ? 0 : x1;
    y2 = y2 > H ? H : y2; x2 = x2 > W ? W : x2;
    return KgBox{y1, x1, y2 > y1 ? y2 - y1 : 0, x2 > x1 ? x2 - x1 : 0};
}
// The 256 threads of a block walk the box as one flat row-major list: thread t calls f(Y, X) for the elements t, t + 256, ...; the
// position advances by additions, no division in the loop, and consecutive lanes visit consecutive pixels of a box row.
template <typename F>
__device__ __forceinline__ void kg_box_walk(const KgBox& b, F&& f) {
    if (b.h > 0 && b.w > 0) {
        const int sy = 256 / b.w, sx = 256 - sy * b.w;
        int yy = (int)threadIdx.x / b.w, xx = (int)threadIdx.x - yy * b.w;
        while (yy < b.h) {
            f(b.y1 + yy, b.x1 + xx);
            xx += sx; yy += sy;
            if (xx >= b.w) { xx -= b.w; ++yy; }
        }
    }
}

// ---- block combine ----------------------------------------------------------------------------------------------------------------------
// part[w][c] = the partial of wave w for column c, written by lane 0 of every wave before a __syncthreads().  Returns column c over the
// four waves: kind says whether the column is a sum, a minimum or a maximum, and when the sum of column `count_col` is 0 (no pixel) a
// minimum (still INT_MAX) or a maximum is 0.  (instance_table_kernel and label_measure_kernel keep their own copies of this combine:
// with the shared one each missed the parent's time twice, profiles/labelcommon_ab.json.)
enum { KG_COL_SUM, KG_COL_MIN, KG_COL_MAX };
template <int NCOL>
__device__ __forceinline__ long long kg_block_combine(const long long (*part)[NCOL], int c, int kind, int count_col) {
    long long v = part[0][c];
    for (int w = 1; w < 4; ++w) {
        const long long t = part[w][c];
        if (kind == KG_COL_MIN) v = t < v ? t : v;
        else if (kind == KG_COL_MAX) v = t > v ? t : v;
        else v += t;
    }
    const long long count = part[0][count_col] + part[1][count_col] + part[2][count_col] + part[3][count_col];
    return count == 0 && kind != KG_COL_SUM ? 0 : v;
}
// the kinds of an instance table row {area_full, area_visible, y1, x1, y2, x2, sum_y, sum_x}; its count column is 1
__device__ __forceinline__ int kg_table_col_kind(int c) { return c == 2 || c == 3 ? KG_COL_MIN : c == 4 || c == 5 ? KG_COL_MAX : KG_COL_SUM; }

// ---- row-segment run walk ---------------------------------------------------------------------------------------------------------------
// A wave owns segment s of one map: the 64 pixels from x0 = 64 (s mod spr) of row y = s / spr, spr = ceil(W / 64), lane l at x0 + l
// (one 256-byte load per wave); a live lane's value is v = map[p], p = y * W + x.  A lane is a run head when its value differs from the
// pixel to its left in the segment, or when it is the segment's first lane; the ballot of the heads gives every lane the end of its
// run (one past its last lane: the next head, or the end of the live lanes, which are lanes 0 .. nlive - 1).
struct KgSegRun { long p; int y, x, v, end, nlive; bool live, head; };
__device__ __forceinline__ KgSegRun kg_seg_run(long s, long spr, int W, const int* __restrict__ map) {
    const int lane = threadIdx.x & 63;
    KgSegRun r;
    r.y = (int)(s / spr); r.x = ((int)(s - (long)r.y * spr) << 6) + lane;
    r.p = (long)r.y * W + r.x;
    r.live = r.x < W;
    r.v = r.live ? map[r.p] : 0;
    const int left = __shfl_up(r.v, 1);
    r.head = r.live && (lane == 0 || r.v != left);
    const unsigned long long heads = __ballot(r.head);
    r.nlive = __popcll(__ballot(r.live));
    const unsigned long long later = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
    r.end = later ? __builtin_ctzll(later) : r.nlive;
    return r;
}

// ---- per-image ranges, passed by value in the kernel arguments ------------------------------------------------------------------------------
#define KG_MAX_IMAGES 256           // images per launch
struct KgRanges { int start[KG_MAX_IMAGES + 1]; };
// the ranges of images [i0, i0 + cnt) (absolute rows), the rest empty; returns the largest row count among them
static inline int kg_ranges(const int* start, int i0, int cnt, KgRanges* rg) {
    int most = 0;
    for (int i = 0; i <= cnt; ++i) rg->start[i] = start[i0 + i];
    for (int i = cnt + 1; i <= KG_MAX_IMAGES; ++i) rg->start[i] = start[i0 + cnt];
    for (int i = 0; i < cnt; ++i) most = rg->start[i + 1] - rg->start[i] > most ? rg->start[i + 1] - rg->start[i] : most;
    return most;
}

// ---- host argument checks: nothing is launched unless they hold.  fn = the entry's name ---------------------------------------------------
#define KG_TRY(call)                            \
    do {                                        \
        const int rc_ = (call);                 \
        if (rc_ != KG_OK) return rc_;           \
    } while (0)

// a HOST start table `what` [nimg + 1] (nimg > 0, not null): first entry 0, non-decreasing, last entry == total (named total_name)
static inline int kg_check_start(const char* fn, const char* what, const int* start, int nimg, int total, const char* total_name) {
    KG_CHECK_ARG(start[0] == 0, "%s: %s[0] is %d, not 0", fn, what, start[0]);
    for (int i = 0; i < nimg; ++i)
        KG_CHECK_ARG(start[i + 1] >= start[i], "%s: %s decreases at image %d", fn, what, i);
    KG_CHECK_ARG(start[nimg] == total, "%s: %s[nimg] is %d, not %s = %d", fn, what, start[nimg], total_name, total);
    return KG_OK;
}
// every pixel index fits int32 (H, W, nimg > 0): of one map, and of a stack of nimg maps.  The division cannot overflow.
static inline int kg_check_map_size(const char* fn, int H, int W) {
    KG_CHECK_ARG((long)H * W <= 0x7fffffffL, "%s: H * W exceeds 2^31 - 1", fn);
    return KG_OK;
}
static inline int kg_check_stack_size(const char* fn, int nimg, int H, int W) {
    KG_CHECK_ARG((long)H * W <= 0x7fffffffL / nimg, "%s: nimg * H * W exceeds 2^31 - 1", fn);
    return KG_OK;
}
static inline bool kg_aligned(const void* p, unsigned mask) { return ((unsigned long long)(size_t)p & mask) == 0; }
// the byte ranges [a, a + abytes) and [b, b + bbytes) do not overlap; an absent or empty range overlaps nothing
static inline bool kg_apart(const void* a, long abytes, const void* b, long bbytes) {
    const char* pa = (const char*)a; const char* pb = (const char*)b;
    return !a || !b || abytes == 0 || bbytes == 0 || pa + abytes <= pb || pb + bbytes <= pa;
}
// The side bound of every per-job entry: H, W <= 2^15, so a box holds at most 2^30 pixels.  Each file says what it relies on.
#define KG_LABEL_MAX_SIDE 32768
// what opens a job entry: a stack of nimg int32 maps [H][W] within the side bound and 2^31 - 1 pixels, and a job table of m rows
// (NULL only when m == 0), both 4-byte aligned.  An extra size (R, V), the outputs and their aliasing stay with the entry.
static inline int kg_check_job_stack(const char* fn, const int* labels, int nimg, int H, int W, const int* jobs, int m) {
    KG_CHECK_ARG(nimg > 0 && H > 0 && W > 0 && m >= 0, "%s: bad size (nimg %d, H %d, W %d, m %d)", fn, nimg, H, W, m);
    KG_CHECK_ARG(H <= KG_LABEL_MAX_SIDE && W <= KG_LABEL_MAX_SIDE, "%s: H %d, W %d exceed %d", fn, H, W, KG_LABEL_MAX_SIDE);
    KG_TRY(kg_check_stack_size(fn, nimg, H, W));
    KG_CHECK_ARG(labels, "%s: null pointer (labels)", fn);
    KG_CHECK_ARG(jobs || m == 0, "%s: null pointer (jobs)", fn);
    KG_CHECK_ARG(kg_aligned(labels, 3) && kg_aligned(jobs, 3), "%s: misaligned pointer", fn);
    return KG_OK;
}
// the image of an entry that reads pixel values: [nimg][H][W][channels] of 1- or 2-byte elements, aligned to its element
static inline int kg_check_image(const char* fn, const void* image, int channels, int elem_bytes) {
    KG_CHECK_ARG(channels >= 1 && channels <= 4, "%s: channels %d (1 .. 4)", fn, channels);
    KG_CHECK_ARG(elem_bytes == 1 || elem_bytes == 2, "%s: elem_bytes %d (1 or 2)", fn, elem_bytes);
    KG_CHECK_ARG(image, "%s: null pointer (image)", fn);
    KG_CHECK_ARG(kg_aligned(image, elem_bytes == 2 ? 1 : 0), "%s: misaligned pointer (image)", fn);
    return KG_OK;
}
// grid cap of the kernels that stride over what is left
#define KG_LABEL_MAX_BLOCKS (1 << 20)
static inline unsigned kg_grid_cap(long blocks) { return (unsigned)(blocks < KG_LABEL_MAX_BLOCKS ? blocks : KG_LABEL_MAX_BLOCKS); }

// leading dimension of a bit-packed H x W mask (include/kgnet_hip.h "bit-mask layout"): H * ceil(W / 64) words, rounded up to even
__host__ __device__ static inline long kg_bits_ld(int H, int W) {
    const long nw = (long)H * ((W + 63) / 64);
    return (nw + 1) & ~1L;
}
static inline bool kg_bits_ld_ok(int H, int W, long ld_words) { return ld_words >= kg_bits_ld(H, W) && ld_words % 2 == 0 && ld_words <= 0x7fffffffL; }
static inline int kg_check_bits_ld(const char* fn, int H, int W, long ld_words) {
    KG_CHECK_ARG(kg_bits_ld_ok(H, W, ld_words), "%s: ld_words %ld too small or odd (need %ld)", fn, ld_words, kg_bits_ld(H, W));
    return KG_OK;
}
