// distance.hip -- nearest-other-label distance maps of instance label maps on gfx950 (distance.py): for every pixel the squared Euclidean
// distance to the nearest pixel of the same image that carries another value, and that value.  Exact in integers, no atomics.
//   kg_label_distance   d2 and nearest of every pixel
//   kg_label_regrow     the same tile computation, written out as one result map: expand, ring, shrink (d2 / nearest never reach memory)
//   kg_label_inscribed  per job {img, id, box}: the largest d2 over the pixels of the box with labels == id, the first pixel that attains
//                       it, and the pixel count -- the inscribed circle of an instance
//
// THE DEFINITION.  labels = int32 [nimg][H][W], ANY int32 values, compared only.  max_d2 in 1 .. 4096, R = floor(sqrt(max_d2)) <= 64.  For a
// pixel p with value v: C(p) = the pixels q of the SAME image with labels[q] != v and |p - q|^2 <= max_d2.  d2[p] = the smallest |p - q|^2
// over C(p), nearest[p] = the smallest value (signed compare) among the q of C(p) at that distance; with C(p) empty d2[p] = max_d2 + 1
// ("saturated") and nearest[p] = v.  With frame != 0 the four sides of the image count as "another value" for d2 only: f = min(y + 1,
// x + 1, H - y, W - x), and where f^2 <= max_d2, d2[p] = min(d2[p], f^2); nearest is not affected.  The result depends on no order of
// execution, and a stacked image never sees its neighbours in the stack.
//
// THE SEPARABLE FORM the kernel computes.  (1) Per pixel, down its own column: g = the vertical distance to the nearest pixel of the column
// whose value differs from the pixel's own -- it lies just past either end of the pixel's vertical run, and only ends within R count --
// and gv = its value, the smaller one when both ends are equally far.  (2) Per pixel (x, y) with value v, along its row for x' in
// [x - R, x + R]: where labels[y][x'] != v the candidate is ((x - x')^2, labels[y][x']); otherwise, where g[y][x'] exists, it is
// ((x - x')^2 + g^2, gv[y][x']).  The lexicographic minimum over the candidates with first component <= max_d2 is (d2, nearest).  It is
// exact: for a fixed column x' the nearest pixel with another value is (x', y) itself or the first pixel past an end of v's run through
// (x', y), and among globally nearest pixels each is nearest within its own column, so the smaller value per column and then the minimum
// over columns is the tie rule.
//
// SIZE RULE.  max_d2 <= 4096, so a candidate is at most 2 * 4096, d2 <= 4097 and g <= 64 fits a byte; nimg * H * W <= 2^31 - 1, so every
// pixel index fits int32.  One workgroup owns a KG_DT_TH x KG_DT_TW tile; its LDS holds the tile's row band widened by R on both sides:
// labels and gv as int32, g as bytes, 9 * KG_DT_TH * (KG_DT_TW + 2 R) bytes = 54 KiB at R = 64, below the 64 KiB a launch gets without
// an attribute.
//
// INDEX RULE (label_common.h).  Every entry validates on the host before any HIP call and never synchronises; every output element is
// written.  Labels and d2 values are predicates and stored values only; a row or column outside the image is decided by a predicate on its
// coordinates before any address is formed; every loop is bounded by a kernel argument or a constant (the row scan may stop EARLIER on
// what it found, never later).  The job table of kg_label_inscribed is the one device-read table, bounded exactly as in
// kg_label_measure: its box is clamped to the map first and its image index is used only inside (unsigned)img < (unsigned)nimg.
// Plain C++ and vector memory operations only.
#include "label_common.h"

#define KG_DT_TH 32                     // tile rows    (distance.TILE_H)
#define KG_DT_TW 64                     // tile columns (distance.TILE_W): one wave per tile row in phase 2
#define KG_DT_MAX_D2 4096
#define KG_DT_MAX_R 64
#define KG_DT_NONE 255                  // g: no end of the run within R
#define KG_DT_OUTSIDE 254               // g: the column lies outside the image
static_assert(KG_DT_TW + 2 * KG_DT_MAX_R <= 256, "phase 1 has one thread per widened column");
static_assert(9 * KG_DT_TH * (KG_DT_TW + 2 * KG_DT_MAX_R) <= 64 * 1024, "the row band fits the LDS a launch gets without an attribute");

enum { KG_DT_EXPAND = 0, KG_DT_RING = 1, KG_DT_SHRINK = 2 };
struct KgRegrow { int op, lo2, hi2; };

// One block per tile (the grid strides when there are more tiles than KG_LABEL_MAX_BLOCKS), blockIdx.y = the image.
//   phase 1  thread c < WW = TW + 2 R owns column x0 - R + c.  It walks down from row y0 - R to the tile's last row (the end of the run
//            above every tile row), then up from row y0 + TH - 1 + R to the tile's first row (the end below), the tile's own rows from
//            LDS the second time.  Adjacent lanes read adjacent columns.  It leaves labels, g and gv of the tile's rows in LDS.
//   phase 2  wave w owns the tile rows w, w + 4, ...; lane l the pixel of column x0 + l.  It scans its row outwards, k = 1 .. R on both
//            sides, and stops once k^2 exceeds the best distance so far.  Consecutive lanes read consecutive dwords (labels, gv) and
//            four lanes share a dword of g: no bank conflict.
// A tile whose widened window holds one value only (and, with frame, lies farther than R from every side) skips the scan: saturated.
// REGROW: the result map of `rg` is written to d2o instead, and pixels whose result does not depend on the distance skip the scan.
template <bool REGROW>
__global__ __launch_bounds__(256) void label_distance_kernel(const int* __restrict__ labels, int H, int W, int tiles_x, long tiles, int R, int max_d2,
                                                             int frame, KgRegrow rg, int* __restrict__ d2o, int* __restrict__ nearo) {
    extern __shared__ int dt_lds[];
    __shared__ int mixed;
    const int WW = KG_DT_TW + 2 * R;
    int* lab = dt_lds;                                                 // [TH][WW]
    int* gv = dt_lds + KG_DT_TH * WW;                                  // [TH][WW]
    unsigned char* g = (unsigned char*)(dt_lds + 2 * KG_DT_TH * WW);   // [TH][WW]
    const long base = (long)blockIdx.y * H * W;                        // blockIdx.y < nimg: base + H * W <= 2^31 - 1
    const int c = threadIdx.x;
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int ty = (int)(t / tiles_x), y0 = ty * KG_DT_TH, x0 = (int)(t - (long)ty * tiles_x) * KG_DT_TW;   // (y0, x0) lies in the image
        if (c == 0) mixed = 0;
        __syncthreads();
        // ---- phase 1 ----
        if (c < WW) {
            const int X = x0 - R + c;
            const int rows = H - y0 < KG_DT_TH ? H - y0 : KG_DT_TH;    // the tile's rows inside the image
            if (X < 0 || X >= W) {
                for (int r = 0; r < rows; ++r) g[r * WW + c] = KG_DT_OUTSIDE;
            } else {
                const int ref = labels[base + (long)y0 * W + x0];
                const int* col = labels + base + X;
                int differs = 0;
                // down: up_d = the distance from the row to the pixel just above its run, up_v = that pixel's value
                const int ys = y0 - R > 0 ? y0 - R : 0;
                int cur = 0, up_d = KG_DT_NONE, up_v = 0;
                for (int y = ys; y < y0 + rows; ++y) {
                    const int val = col[(long)y * W];
                    differs |= val != ref;
                    if (y == ys) cur = val;
                    else if (val != cur) { up_v = cur; up_d = 1; cur = val; }
                    else if (up_d < KG_DT_NONE) ++up_d;
                    if (y >= y0) {
                        const int q = (y - y0) * WW + c;
                        lab[q] = val; gv[q] = up_v; g[q] = (unsigned char)(up_d <= R ? up_d : KG_DT_NONE);
                    }
                }
                // up: the same from below, combined with what the walk down left: the nearer end, the smaller value when equally far
                const int ye = y0 + KG_DT_TH + R < H ? y0 + KG_DT_TH + R : H;
                int dn_d = KG_DT_NONE, dn_v = 0;
                for (int y = ye - 1; y >= y0; --y) {
                    const int q = (y - y0) * WW + c;
                    const bool own = y < y0 + rows;                    // (rows < TH only when the image ends here: then ye == y0 + rows)
                    const int val = own ? lab[q] : col[(long)y * W];
                    differs |= val != ref;
                    if (y == ye - 1) cur = val;
                    else if (val != cur) { dn_v = cur; dn_d = 1; cur = val; }
                    else if (dn_d < KG_DT_NONE) ++dn_d;
                    if (own && dn_d <= R) {
                        const int ud = g[q];
                        if (dn_d < ud || (dn_d == ud && dn_v < gv[q])) { g[q] = (unsigned char)dn_d; gv[q] = dn_v; }
                    }
                }
                if (differs) mixed = 1;
            }
        }
        __syncthreads();
        const bool near_frame = frame && (y0 < R || x0 < R || y0 + KG_DT_TH + R > H || x0 + KG_DT_TW + R > W);
        const bool scan = mixed || near_frame;
        // ---- phase 2 ----
        const int lane = threadIdx.x & 63, X = x0 + lane, cc = R + lane;
        for (int r = threadIdx.x >> 6; r < KG_DT_TH; r += 4) {
            const int Y = y0 + r;
            if (Y >= H || X >= W) continue;
            const int* lrow = lab + r * WW;
            const int* vrow = gv + r * WW;
            const unsigned char* grow = g + r * WW;
            const int v = lrow[cc];
            int best = max_d2 + 1, bv = v;
            bool need = scan;
            if (REGROW) need = need && (rg.op == KG_DT_SHRINK ? v != 0 : v == 0);
            if (need) {
                const int g0 = grow[cc];
                if (g0 <= R && g0 * g0 <= max_d2) { best = g0 * g0; bv = vrow[cc]; }
                for (int k = 1; k <= R; ++k) {
                    const int kk = k * k;
                    if (kk > best) break;                              // every later candidate is farther than the best
#pragma unroll
                    for (int side = 0; side < 2; ++side) {
                        const int q = side ? cc + k : cc - k;
                        const int gg = grow[q];
                        if (gg == KG_DT_OUTSIDE) continue;
                        const int l = lrow[q];
                        int d, val;
                        if (l != v) { d = kk; val = l; }
                        else if (gg <= R) { d = kk + gg * gg; val = vrow[q]; }
                        else continue;
                        if (d <= max_d2 && (d < best || (d == best && val < bv))) { best = d; bv = val; }
                    }
                }
                if (frame) {
                    int f = Y + 1 < X + 1 ? Y + 1 : X + 1;
                    f = H - Y < f ? H - Y : f;
                    f = W - X < f ? W - X : f;
                    if (f <= R && f * f <= max_d2 && f * f < best) best = f * f;
                }
            }
            const long p = base + (long)Y * W + X;
            if (REGROW) {
                int o;
                if (rg.op == KG_DT_EXPAND) o = v == 0 && best <= rg.hi2 ? bv : v;
                else if (rg.op == KG_DT_RING) o = v == 0 && best > rg.lo2 && best <= rg.hi2 ? bv : 0;
                else o = v != 0 && best > rg.hi2 ? v : 0;
                d2o[p] = o;
            } else {
                if (d2o) d2o[p] = best;
                if (nearo) nearo[p] = bv;
            }
        }
        __syncthreads();                                               // the LDS band is written again by the block's next tile
    }
}

// One block per job (the grid strides when there are more jobs than KG_LABEL_MAX_BLOCKS).  key = d2 in the high half, 2^31 - 1 - (y * W + x)
// in the low half: the largest key is the largest d2 at the smallest index.  Reduced by shuffles and 4 * 2 * 8 bytes of LDS.
__device__ __forceinline__ long long kg_dt_wave_max(long long v) {
    for (int o = 32; o; o >>= 1) { const long long t = __shfl_xor(v, o); v = t > v ? t : v; }
    return v;
}
__global__ __launch_bounds__(256) void label_inscribed_kernel(const int* __restrict__ labels, const int* __restrict__ d2, int nimg, int H, int W,
                                                              const int* __restrict__ jobs, int m, int* __restrict__ out) {
    __shared__ long long part[4][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long j = blockIdx.x; j < m; j += gridDim.x) {
        const int* jb = jobs + j * 6;
        const int img = jb[0], id = jb[1];
        KgBox box = kg_job_box(jb + 2, H, W);
        if (!((unsigned)img < (unsigned)nimg)) box.h = box.w = 0;      // the only use of img before it scales an address
        const long base = (long)img * H * W;                           // used only with a non-empty box: img < nimg
        long long key = LLONG_MIN;
        int count = 0;
        kg_box_walk(box, [&](int Y, int X) {
            const int idx = Y * W + X;                                 // < H * W <= 2^31 - 1
            if (labels[base + idx] == id) {
                const long long k = (long long)(((unsigned long long)(unsigned)d2[base + idx] << 32) | (unsigned)(0x7fffffff - idx));
                key = k > key ? k : key;
                ++count;
            }
        });
        key = kg_dt_wave_max(key);
        count = kg_wave_sum(count);
        if (lane == 0) { part[wave][0] = key; part[wave][1] = count; }
        __syncthreads();
        if (threadIdx.x == 0) {
            const long long best = kg_block_combine<2>(part, 0, KG_COL_MAX, 1), total = kg_block_combine<2>(part, 1, KG_COL_SUM, 1);
            int* o = out + j * 4;
            if (total == 0) { o[0] = 0; o[1] = -1; o[2] = -1; o[3] = 0; }
            else {
                const int idx = 0x7fffffff - (int)(best & 0xffffffffLL);
                o[0] = (int)(best >> 32); o[1] = idx / W; o[2] = idx - (idx / W) * W; o[3] = (int)total;
            }
        }
        __syncthreads();                                               // part is written again by the block's next job
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
static int dt_radius(int max_d2) {
    int r = 0;
    while ((r + 1) * (r + 1) <= max_d2) ++r;
    return r;
}

static int dt_check_maps(const char* fn, const int* labels, int nimg, int H, int W, int max_d2) {
    KG_CHECK_ARG(nimg > 0 && H > 0 && W > 0, "%s: bad size (nimg %d, H %d, W %d)", fn, nimg, H, W);
    KG_TRY(kg_check_stack_size(fn, nimg, H, W));
    KG_CHECK_ARG(max_d2 >= 1 && max_d2 <= KG_DT_MAX_D2, "%s: max_d2 %d (1 .. %d)", fn, max_d2, KG_DT_MAX_D2);
    KG_CHECK_ARG(labels, "%s: null pointer (labels)", fn);
    return KG_OK;
}

template <bool REGROW>
static int dt_launch(const char* fn, const int* labels, int nimg, int H, int W, int max_d2, int frame, KgRegrow rg, int* a, int* b, hipStream_t s) {
    const int R = dt_radius(max_d2), tiles_x = (W + KG_DT_TW - 1) / KG_DT_TW;
    const long tiles = (long)tiles_x * ((H + KG_DT_TH - 1) / KG_DT_TH);
    const size_t lds = (size_t)9 * KG_DT_TH * (KG_DT_TW + 2 * R);
    const long per = (long)H * W;
    for (int i0 = 0; i0 < nimg; i0 += 65535) {                         // the image index is a grid dimension
        const int cnt = nimg - i0 < 65535 ? nimg - i0 : 65535;
        hipLaunchKernelGGL((label_distance_kernel<REGROW>), dim3(kg_grid_cap(tiles), cnt), dim3(256), lds, s, labels + i0 * per, H, W, tiles_x, tiles, R,
                           max_d2, frame != 0, rg, a ? a + i0 * per : nullptr, b ? b + i0 * per : nullptr);
    }
    KG_CHECK_LAUNCH(fn);
    return KG_OK;
}

extern "C" int kg_label_distance(const int* labels, int nimg, int H, int W, int max_d2, int frame, int* d2, int* nearest, void* stream) {
    KG_TRY(dt_check_maps("kg_label_distance", labels, nimg, H, W, max_d2));
    KG_CHECK_ARG(d2 || nearest, "kg_label_distance: d2 and nearest are both NULL");
    KG_CHECK_ARG(kg_aligned(labels, 3) && kg_aligned(d2, 3) && kg_aligned(nearest, 3), "kg_label_distance: misaligned pointer");
    KG_CHECK_ARG(d2 != labels && nearest != labels && d2 != nearest, "kg_label_distance: d2 / nearest alias labels or each other");
    return dt_launch<false>("label_distance", labels, nimg, H, W, max_d2, frame, KgRegrow{0, 0, 0}, d2, nearest, (hipStream_t)stream);
}

extern "C" int kg_label_regrow(const int* labels, int nimg, int H, int W, int max_d2, int frame, int op, int lo2, int hi2, int* out, void* stream) {
    KG_TRY(dt_check_maps("kg_label_regrow", labels, nimg, H, W, max_d2));
    KG_CHECK_ARG(op >= KG_DT_EXPAND && op <= KG_DT_SHRINK, "kg_label_regrow: op %d (0 expand, 1 ring, 2 shrink)", op);
    KG_CHECK_ARG(0 <= lo2 && lo2 <= hi2 && hi2 <= max_d2, "kg_label_regrow: need 0 <= lo2 <= hi2 <= max_d2 (lo2 %d, hi2 %d, max_d2 %d)", lo2, hi2, max_d2);
    KG_CHECK_ARG(op == KG_DT_RING || lo2 == 0, "kg_label_regrow: lo2 %d must be 0 for op %d", lo2, op);
    KG_CHECK_ARG(op == KG_DT_SHRINK || frame == 0, "kg_label_regrow: frame must be 0 for op %d (expand and ring do not see the frame)", op);
    KG_CHECK_ARG(out, "kg_label_regrow: null pointer (out)");
    KG_CHECK_ARG(kg_aligned(labels, 3) && kg_aligned(out, 3), "kg_label_regrow: misaligned pointer");
    KG_CHECK_ARG(out != labels, "kg_label_regrow: out aliases labels");
    return dt_launch<true>("label_regrow", labels, nimg, H, W, max_d2, frame, KgRegrow{op, lo2, hi2}, out, nullptr, (hipStream_t)stream);
}

// labels, d2: device int32 [nimg][H][W]; jobs: device int32 [m][6] = (img, id, y1, x1, y2, x2), written by the caller; out: device int32 [m][4]
extern "C" int kg_label_inscribed(const int* labels, const int* d2, int nimg, int H, int W, const int* jobs, int m, int* out, void* stream) {
    KG_CHECK_ARG(nimg > 0 && H > 0 && W > 0 && m >= 0, "kg_label_inscribed: bad size (nimg %d, H %d, W %d, m %d)", nimg, H, W, m);
    KG_TRY(kg_check_stack_size("kg_label_inscribed", nimg, H, W));
    KG_CHECK_ARG(labels && d2, "kg_label_inscribed: null pointer (labels / d2)");
    KG_CHECK_ARG((jobs && out) || m == 0, "kg_label_inscribed: null pointer (jobs / out)");
    KG_CHECK_ARG(kg_aligned(labels, 3) && kg_aligned(d2, 3) && kg_aligned(jobs, 3) && kg_aligned(out, 3), "kg_label_inscribed: misaligned pointer");
    KG_CHECK_ARG(!out || (out != labels && out != d2 && out != jobs), "kg_label_inscribed: out aliases an input");
    if (m == 0) return KG_OK;
    hipLaunchKernelGGL(label_inscribed_kernel, dim3(kg_grid_cap(m)), dim3(256), 0, (hipStream_t)stream, labels, d2, nimg, H, W, jobs, m, out);
    KG_CHECK_LAUNCH("label_inscribed");
    return KG_OK;
}
