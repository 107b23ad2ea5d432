// instances.hip -- from bit-packed instance masks to what the users of this network read: one instance label map per image, a table of
// exact per-instance integers, and the reference's mask overlay (test.py:29-37 apply_mask, looped as test.py:171-185) on gfx950.
// Input = the masks of one or more images of one size in the bit-mask layout of include/kgnet_hip.h, all rows concatenated; image i owns
// rows [row_start[i], row_start[i + 1]).  Row order is priority order (predict's rows are sorted by descending confidence).
//
// The index rule of label_common.h holds without exception here: every output has a size the host knows, and addresses come from the
// grid indices, the loop counters and the host-validated row ranges (passed by value) alone.  Values read from words / ids / colors only
// ever become predicates or stored values.
//
// Skeleton of the label and overlay kernels (paste_bits_kernel's): a wave owns one 64-pixel word position of one image, lane b owns pixel
// 64 k + b.  The wave walks the image's rows in chunks of 64: lane j loads that word of row c + j (one gather per chunk), the set bits of
// __ballot(word != 0) name the few rows that touch the position (masks are sparse: 2-4 at 512 x 512 with 150 instances), and each of
// them is broadcast with v_readlane for every lane to test its own bit.  The label kernel leaves a position once every live lane is
// resolved; the overlay visits every covering row, in ascending order, because the blend compounds.
// Compiled with -ffp-contract=off: the overlay's float64 expression must round product by product, as NumPy evaluates it.
#include "label_common.h"

#define KG_INST_WPW 8               // consecutive words a wave walks (one 64-byte line of every row it gathers from)

// lane j's value for every lane; j is wave-uniform (it comes from a ballot)
__device__ __forceinline__ unsigned inst_lane_u32(unsigned v, int j) { return (unsigned)__builtin_amdgcn_readlane((int)v, j); }
__device__ __forceinline__ unsigned long long inst_lane_u64(unsigned long long v, int j) {
    const unsigned lo = inst_lane_u32((unsigned)v, j), hi = inst_lane_u32((unsigned)(v >> 32), j);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ double inst_lane_f64(double v, int j) { return __longlong_as_double((long long)inst_lane_u64((unsigned long long)__double_as_longlong(v), j)); }

// labels[img][y][x] = id of the first row of the image, in row order, whose bit is set; 0 if none.  id = ids[row] (a value, never an
// index) or row - row_start[img] + 1.
__global__ __launch_bounds__(256) void instance_labels_kernel(const unsigned long long* __restrict__ words, long ld_words, const KgRanges rg, int H,
                                                              int W, const int* __restrict__ ids, int* __restrict__ labels) {
    const int lane = threadIdx.x & 63, wpr = (W + 63) >> 6, img = blockIdx.y;
    const long nw = (long)H * wpr;
    const int rs = rg.start[img], re = rg.start[img + 1];
    const long r0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * KG_INST_WPW;
    int* dst = labels + (long)img * H * W;
    for (long r = r0; r < r0 + KG_INST_WPW && r < nw; ++r) {         // r < nw: the padding word is never read
        const int y = (int)(r / wpr), x = ((int)(r - (long)y * wpr) << 6) + lane;
        const bool live = x < W;
        bool open = live;
        int label = 0;
        for (int c = rs; c < re; c += 64) {
            const int row = c + lane;
            const unsigned long long wd = row < re ? words[(long)row * ld_words + r] : 0ull;
            unsigned long long m = __ballot(wd != 0);
            if (m) {
                const int idv = row < re ? (ids ? ids[row] : row - rs + 1) : 0;
                do {
                    const int j = __builtin_ctzll(m);
                    m &= m - 1;
                    const unsigned long long wj = inst_lane_u64(wd, j);
                    const int idj = (int)inst_lane_u32((unsigned)idv, j);
                    if (open && ((wj >> lane) & 1ull)) {
                        label = idj;
                        open = false;
                    }
                } while (m);
                if (__ballot(open) == 0) break;
            }
        }
        if (live) dst[(long)y * W + x] = label;
    }
}

// sum of the positions of the set bits of w
__device__ __forceinline__ int inst_bitpos_sum(unsigned long long w) {
    return __builtin_popcountll(w & 0xAAAAAAAAAAAAAAAAull) + (__builtin_popcountll(w & 0xCCCCCCCCCCCCCCCCull) << 1) +
           (__builtin_popcountll(w & 0xF0F0F0F0F0F0F0F0ull) << 2) + (__builtin_popcountll(w & 0xFF00FF00FF00FF00ull) << 3) +
           (__builtin_popcountll(w & 0xFFFF0000FFFF0000ull) << 4) + (__builtin_popcountll(w & 0xFFFFFFFF00000000ull) << 5);
}

// table[row] = {area_full, area_visible, y1, x1, y2, x2, sum_y, sum_x}.  One block per row; lane l of a wave owns word k0 + l of the row
// (coalesced), and the pixels the row wins are its own bits minus those of the earlier rows of its image at the same word -- the label
// map's rule, recomputed from the words, so that ids need not be distinct.  A lane whose word has nothing left loads nothing more, and a
// wave leaves the earlier rows once no lane has anything left.  Integers only: no atomics, no initialisation, any order gives the same table.
__global__ __launch_bounds__(256) void instance_table_kernel(const unsigned long long* __restrict__ words, long ld_words, const KgRanges rg, int H,
                                                             int W, long long* __restrict__ table) {
    __shared__ long long part[4][8];
    const int img = blockIdx.y, rs = rg.start[img], re = rg.start[img + 1];
    const int row = rs + (int)blockIdx.x;
    if (row >= re) return;                                            // uniform over the block
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpr = (W + 63) >> 6;
    const long nw = (long)H * wpr;
    const unsigned long long tail = (W & 63) ? (1ull << (W & 63)) - 1 : ~0ull;      // pixels x < W of a row's last word
    const unsigned long long* mine = words + (long)row * ld_words;
    long long area_full = 0, area = 0, sum_y = 0, sum_x = 0;
    int y1 = INT_MAX, x1 = INT_MAX, y2 = 0, x2 = 0;
    for (long k0 = wave * 64L; k0 < nw; k0 += 256) {
        const long k = k0 + lane;
        const bool in = k < nw;
        const int y = in ? (int)(k / wpr) : 0, kw = in ? (int)(k - (long)y * wpr) : 0;
        unsigned long long left = in ? mine[k] : 0ull;
        if (kw == wpr - 1) left &= tail;
        area_full += __builtin_popcountll(left);
        for (int e = rs; e < row; e += 8) {
            if (__ballot(left != 0) == 0) break;
            if (left) {
                unsigned long long cover = 0;
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (e + u < row) cover |= words[(long)(e + u) * ld_words + k];
                left &= ~cover;
            }
        }
        if (left) {
            const int cnt = __builtin_popcountll(left), xa = kw << 6;
            area += cnt;
            sum_y += (long long)y * cnt;
            sum_x += (long long)xa * cnt + inst_bitpos_sum(left);
            y1 = y < y1 ? y : y1;
            y2 = y + 1 > y2 ? y + 1 : y2;
            const int xl = xa + __builtin_ctzll(left), xr = xa + 64 - __builtin_clzll(left);
            x1 = xl < x1 ? xl : x1;
            x2 = xr > x2 ? xr : x2;
        }
    }
    area_full = kg_wave_sum(area_full); area = kg_wave_sum(area); sum_y = kg_wave_sum(sum_y); sum_x = kg_wave_sum(sum_x);
    y1 = kg_wave_min(y1); x1 = kg_wave_min(x1); y2 = kg_wave_max(y2); x2 = kg_wave_max(x2);
    if (lane == 0) {
        long long* p = part[wave];
        p[0] = area_full; p[1] = area; p[2] = y1; p[3] = x1; p[4] = y2; p[5] = x2; p[6] = sum_y; p[7] = sum_x;
    }
    __syncthreads();
    // kg_block_combine (label_common.h), kept as this kernel's own copy: with the shared function the label-map-and-table leg at
    // 512^2, N = 8 measured above the parent's maximum twice (profiles/labelcommon_ab.json)
    if (threadIdx.x < 8) {
        const int c = threadIdx.x;
        long long v = part[0][c];
        for (int w = 1; w < 4; ++w) {
            const long long t = part[w][c];
            if (c == 2 || c == 3) v = t < v ? t : v;
            else if (c == 4 || c == 5) v = t > v ? t : v;
            else v += t;
        }
        const long long visible = part[0][1] + part[1][1] + part[2][1] + part[3][1];
        if (visible == 0 && c >= 2 && c <= 5) v = 0;
        table[(long)row * 8 + c] = v;
    }
}

// out[img][y][x][c] = apply_mask (test.py:29-37) for every row of the image that covers (y, x), in ascending row order:
// v = (uint8)(v * (1 - alpha) + alpha * color[c] * 255), float64, products and sums in exactly that order, truncated as NumPy's assignment
// into a uint8 image does (float64 -> integer -> low byte).  image and out may be the same buffer: a lane reads and writes its own pixel only.
__global__ __launch_bounds__(256) void instance_overlay_kernel(const unsigned char* image, const unsigned long long* __restrict__ words, long ld_words,
                                                               const KgRanges rg, int H, int W, const double* __restrict__ colors, double alpha,
                                                               unsigned char* out) {
    const int lane = threadIdx.x & 63, wpr = (W + 63) >> 6, img = blockIdx.y;
    const long nw = (long)H * wpr;
    const int rs = rg.start[img], re = rg.start[img + 1];
    const long r0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * KG_INST_WPW;
    const double keep = 1 - alpha;
    for (long r = r0; r < r0 + KG_INST_WPW && r < nw; ++r) {
        const int y = (int)(r / wpr), x = ((int)(r - (long)y * wpr) << 6) + lane;
        const bool live = x < W;
        const long px = (((long)img * H + y) * W + x) * 3;
        unsigned char v0 = 0, v1 = 0, v2 = 0;
        if (live) { v0 = image[px]; v1 = image[px + 1]; v2 = image[px + 2]; }
        for (int c = rs; c < re; c += 64) {
            const int row = c + lane;
            const unsigned long long wd = row < re ? words[(long)row * ld_words + r] : 0ull;
            unsigned long long m = __ballot(wd != 0);
            if (m) {
                double a0 = 0, a1 = 0, a2 = 0;                        // alpha * color[c] * 255 of this lane's row
                if (row < re) {
                    const double* col = colors + (long)row * 3;
                    a0 = alpha * col[0] * 255; a1 = alpha * col[1] * 255; a2 = alpha * col[2] * 255;
                }
                do {
                    const int j = __builtin_ctzll(m);
                    m &= m - 1;
                    const unsigned long long wj = inst_lane_u64(wd, j);
                    const double b0 = inst_lane_f64(a0, j), b1 = inst_lane_f64(a1, j), b2 = inst_lane_f64(a2, j);
                    if (live && ((wj >> lane) & 1ull)) {
                        v0 = (unsigned char)(long long)((double)v0 * keep + b0);
                        v1 = (unsigned char)(long long)((double)v1 * keep + b1);
                        v2 = (unsigned char)(long long)((double)v2 * keep + b2);
                    }
                } while (m);
            }
        }
        if (live) { out[px] = v0; out[px + 1] = v1; out[px + 2] = v2; }
    }
}

// host-side validation shared by both entries: nothing is launched unless all of it holds
static int inst_check(const char* fn, const void* words, long ld_words, int n, const int* row_start, int nimg, int H, int W) {
    KG_CHECK_ARG(row_start, "%s: null pointer (row_start)", fn);
    KG_CHECK_ARG(H > 0 && W > 0 && n >= 0 && nimg > 0, "%s: bad size (H %d, W %d, n %d, nimg %d)", fn, H, W, n, nimg);
    KG_TRY(kg_check_bits_ld(fn, H, W, ld_words));
    KG_CHECK_ARG(words || n == 0, "%s: null pointer (words)", fn);
    KG_CHECK_ARG(kg_aligned(words, 15), "%s: words must be 16-byte aligned", fn);
    KG_TRY(kg_check_start(fn, "row_start", row_start, nimg, n, "n"));
    KG_TRY(kg_check_stack_size(fn, nimg, H, W));
    KG_CHECK_ARG((long)n <= LONG_MAX / 8 / ld_words, "%s: n * ld_words too large", fn);
    return KG_OK;
}
static inline dim3 inst_grid(int H, int W, int nimg) {
    const long nw = (long)H * ((W + 63) / 64);
    return dim3((unsigned)((nw + 4 * KG_INST_WPW - 1) / (4 * KG_INST_WPW)), (unsigned)nimg);
}

// words: device [n][ld_words]; row_start: HOST int [nimg + 1]; ids: device int [n] or NULL; labels: device int [nimg][H][W];
// table: device int64 [n][8] or NULL.  One launch for the label map and one for the table per 256 images; no host synchronisation.
extern "C" int kg_instance_labels(const void* words, long ld_words, int n, const int* row_start, int nimg, int H, int W, const int* ids, int* labels,
                                  long long* table, void* stream) {
    KG_TRY(inst_check("kg_instance_labels", words, ld_words, n, row_start, nimg, H, W));
    KG_CHECK_ARG(labels, "kg_instance_labels: null pointer (labels)");
    for (int i0 = 0; i0 < nimg; i0 += KG_MAX_IMAGES) {
        const int cnt = nimg - i0 < KG_MAX_IMAGES ? nimg - i0 : KG_MAX_IMAGES;
        KgRanges rg;
        const int most = kg_ranges(row_start, i0, cnt, &rg);
        hipLaunchKernelGGL(instance_labels_kernel, inst_grid(H, W, cnt), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)words, ld_words,
                           rg, H, W, ids, labels + (long)i0 * H * W);
        KG_CHECK_LAUNCH("instance_labels");
        if (table && most > 0) {
            hipLaunchKernelGGL(instance_table_kernel, dim3((unsigned)most, (unsigned)cnt), dim3(256), 0, (hipStream_t)stream,
                               (const unsigned long long*)words, ld_words, rg, H, W, table);
            KG_CHECK_LAUNCH("instance_table");
        }
    }
    return KG_OK;
}

// image / out: device bytes [nimg][H][W][3] (out may equal image); colors: device float64 [n][3]; one launch per 256 images
extern "C" int kg_instance_overlay(const void* image, const void* words, long ld_words, int n, const int* row_start, int nimg, int H, int W,
                                   const double* colors, double alpha, void* out, void* stream) {
    KG_TRY(inst_check("kg_instance_overlay", words, ld_words, n, row_start, nimg, H, W));
    KG_CHECK_ARG(image && out && (colors || n == 0), "kg_instance_overlay: null pointer");
    KG_CHECK_ARG(alpha >= 0 && alpha <= 1, "kg_instance_overlay: alpha %g outside [0, 1]", alpha);
    for (int i0 = 0; i0 < nimg; i0 += KG_MAX_IMAGES) {
        const int cnt = nimg - i0 < KG_MAX_IMAGES ? nimg - i0 : KG_MAX_IMAGES;
        KgRanges rg;
        kg_ranges(row_start, i0, cnt, &rg);
        const long off = (long)i0 * H * W * 3;
        hipLaunchKernelGGL(instance_overlay_kernel, inst_grid(H, W, cnt), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)image + off,
                           (const unsigned long long*)words, ld_words, rg, H, W, colors, alpha, (unsigned char*)out + off);
        KG_CHECK_LAUNCH("instance_overlay");
    }
    return KG_OK;
}
