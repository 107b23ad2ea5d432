// tiling.hip -- tiled whole-image inference on gfx950: what sits on either side of the per-tile predict calls (tiling.py).
//   kg_tile_cut      uint8 image [H][W][3] -> the network input of every tile of a grid, float32 [ny * nx][3][th][tw]
//   kg_bitmask_clip  clears the bits of bit-packed masks outside a valid window (a tile that reaches past the image)
//   kg_tile_stitch   per-tile label maps [ny * nx][th][tw] -> ONE label map [H][W]: per pixel the smallest non-zero value over the tiles
//                    that cover it
//   kg_label_table   per-instance integers read back from the stitched map inside each instance's box
//
// The index rule of label_common.h holds here.  The only addresses that depend on a table are those of the grid origins (a HOST array,
// validated, passed by value in the kernel arguments) and of the job boxes of kg_label_table (kg_job_box).
// Compiled with -ffp-contract=off: the tile input is float32(u8) / 255 - 0.5 as two float32 operations.
#include "label_common.h"

#define KG_TILE_MAX_AXIS 256        // tiles per axis: their origins travel by value in the kernel arguments (2 KB)
struct TileGrid { int ys[KG_TILE_MAX_AXIS]; int xs[KG_TILE_MAX_AXIS]; };

// ---- cut ------------------------------------------------------------------------------------------------------------------------------
// One lane: 4 adjacent pixels of one tile row (sp_image_kernel's shape): 12 source bytes, one float4 store per channel plane.  A pixel
// outside the image reads nothing and takes the value of pixel 0 (0 / 255 - 0.5 == -0.5); the test is per pixel, so an in-image width
// that is no multiple of 4 is exact.  Grid: x = pixel groups of a tile, y = grid column, z = grid row (both uniform: the origins are
// scalar loads).
__global__ __launch_bounds__(256) void tile_cut_kernel(const unsigned char* __restrict__ image, int H, int W, const TileGrid g, int th, int tw,
                                                       float* __restrict__ out) {
    const int q = blockIdx.x * 256 + threadIdx.x, qpr = tw >> 2;
    if (q >= th * qpr) return;
    const int y = q / qpr, x = (q - y * qpr) << 2;
    const int c = blockIdx.y, r = blockIdx.z, nx = gridDim.y;
    const int gy = g.ys[r] + y, gx = g.xs[c] + x;
    const bool rowin = gy < H;
    const unsigned char* src = image + ((long)gy * W + gx) * 3;
    float v[3][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const bool in = rowin && gx + e < W;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float f = in ? (float)src[e * 3 + ch] : 0.f;
            const float d = f / 255.f;
            v[ch][e] = d - 0.5f;
        }
    }
    float* dst = out + (((long)(r * nx + c) * 3) * th + y) * tw + x;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
        *reinterpret_cast<float4*>(dst + (long)ch * th * tw) = make_float4(v[ch][0], v[ch][1], v[ch][2], v[ch][3]);
}

// ---- clip -----------------------------------------------------------------------------------------------------------------------------
// One lane per word position (consecutive lanes, consecutive words: coalesced), walking the masks.  What a position keeps is the same
// for every mask: a position wholly inside the window returns at once, one wholly outside is stored as zero without being read, and
// only the words the window's right edge cuts are read, masked and stored.  The padding word and rows >= n are never touched.
__global__ __launch_bounds__(256) void bitmask_clip_kernel(unsigned long long* __restrict__ words, long ld_words, int n, int H, int W, int vh,
                                                           int vw) {
    const int wpr = (W + 63) >> 6;
    const long nw = (long)H * wpr, r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= nw) return;
    const int y = (int)(r / wpr), x0 = (int)(r - (long)y * wpr) << 6;
    unsigned long long keep = 0;
    if (y < vh && x0 < vw) {
        if (x0 + 64 <= vw) return;
        keep = (1ull << (vw - x0)) - 1;                               // 1 <= vw - x0 <= 63
    }
    for (int k = blockIdx.y; k < n; k += gridDim.y) {
        unsigned long long* p = words + (long)k * ld_words + r;
        *p = keep ? (*p & keep) : 0ull;
    }
}

// ---- stitch ---------------------------------------------------------------------------------------------------------------------------
// One lane per output pixel, one block per 256 pixels of one image row: a gather over the grid rows that cover y (uniform) and the grid
// columns that reach the block's 256 pixels (uniform), each lane testing its own x.  Every pixel is written exactly once, by one lane,
// from reads of tile_labels alone: no atomics, no read of labels, any launch order gives the same map.
__global__ __launch_bounds__(256) void tile_stitch_kernel(const int* __restrict__ tile_labels, const TileGrid g, int ny, int nx, int th, int tw,
                                                          int H, int W, int* __restrict__ labels) {
    const int y = blockIdx.x, bx0 = blockIdx.y * 256, x = bx0 + (int)threadIdx.x;
    const bool live = x < W;
    int best = 0;
    for (int r = 0; r < ny; ++r) {
        const int ty = y - g.ys[r];
        if (ty < 0) break;                                            // origins ascend (validated): no later row covers y either
        if (ty >= th) continue;
        for (int c = 0; c < nx; ++c) {
            const int x0 = g.xs[c];
            if (x0 > bx0 + 255) break;
            if (x0 + tw <= bx0) continue;
            const int tx = x - x0;
            if (live && tx >= 0 && tx < tw) {
                const int v = tile_labels[(((long)r * nx + c) * th + ty) * tw + tx];
                if (v != 0 && (best == 0 || v < best)) best = v;
            }
        }
    }
    if (live) labels[(long)y * W + x] = best;
}

// ---- table ----------------------------------------------------------------------------------------------------------------------------
// table[j] = {area_full[j] (0 without area_full), then over the pixels of the box of job j whose label equals its id: count, y1, x1, y2,
// x2 (half-open; zeros if none), sum_y, sum_x}.  One block per job, walking its clamped box (kg_box_walk).  Integers only, reduced by
// shuffles and 256 bytes of LDS.
__global__ __launch_bounds__(256) void label_table_kernel(const int* __restrict__ labels, int H, int W, const int* __restrict__ jobs,
                                                          const long long* __restrict__ area_full, long long* __restrict__ table) {
    __shared__ long long part[4][8];
    const long j = blockIdx.x;
    const int* jb = jobs + j * 5;
    const int id = jb[0];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long area = 0, sum_y = 0, sum_x = 0;
    int y1 = INT_MAX, x1 = INT_MAX, y2 = 0, x2 = 0;
    kg_box_walk(kg_job_box(jb + 1, H, W), [&](int Y, int X) {
        if (labels[(long)Y * W + X] == id) {
            ++area; sum_y += Y; sum_x += X;
            y1 = Y < y1 ? Y : y1; y2 = Y + 1 > y2 ? Y + 1 : y2;
            x1 = X < x1 ? X : x1; x2 = X + 1 > x2 ? X + 1 : x2;
        }
    });
    area = kg_wave_sum(area); sum_y = kg_wave_sum(sum_y); sum_x = kg_wave_sum(sum_x);
    y1 = kg_wave_min(y1); x1 = kg_wave_min(x1); y2 = kg_wave_max(y2); x2 = kg_wave_max(x2);
    if (lane == 0) {
        long long* p = part[wave];
        p[0] = 0; p[1] = area; p[2] = y1; p[3] = x1; p[4] = y2; p[5] = x2; p[6] = sum_y; p[7] = sum_x;
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        const int c = threadIdx.x;
        const long long v = kg_block_combine<8>(part, c, kg_table_col_kind(c), 1);
        table[j * 8 + c] = c == 0 ? (area_full ? area_full[j] : 0) : v;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
static int tile_axis_check(const char* fn, const char* axis, const int* o, int n, int L) {
    KG_CHECK_ARG(o, "%s: null pointer (%s origins)", fn, axis);
    KG_CHECK_ARG(n >= 1 && n <= KG_TILE_MAX_AXIS, "%s: %d tiles along %s (1 .. %d)", fn, n, axis, KG_TILE_MAX_AXIS);
    KG_CHECK_ARG(o[0] >= 0, "%s: %s origin %d is negative", fn, axis, o[0]);
    for (int i = 1; i < n; ++i) KG_CHECK_ARG(o[i] > o[i - 1], "%s: %s origins do not ascend at tile %d", fn, axis, i);
    KG_CHECK_ARG(o[n - 1] < L, "%s: %s origin %d starts outside the image (%d)", fn, axis, o[n - 1], L);
    return KG_OK;
}
// the grid of kg_tile_cut / kg_tile_stitch: nothing is launched unless all of it holds
static int tile_grid_check(const char* fn, const int* ys, int ny, const int* xs, int nx, int th, int tw, int H, int W, TileGrid* g) {
    KG_CHECK_ARG(H > 0 && W > 0 && th > 0 && tw > 0, "%s: bad size (H %d, W %d, th %d, tw %d)", fn, H, W, th, tw);
    KG_TRY(kg_check_map_size(fn, H, W));
    KG_TRY(tile_axis_check(fn, "y", ys, ny, H));
    KG_TRY(tile_axis_check(fn, "x", xs, nx, W));
    KG_CHECK_ARG((long)ny * nx * th <= 0x7fffffffL / tw, "%s: ny * nx * th * tw exceeds 2^31 - 1", fn);
    memset(g, 0, sizeof(*g));
    for (int i = 0; i < ny; ++i) g->ys[i] = ys[i];
    for (int i = 0; i < nx; ++i) g->xs[i] = xs[i];
    return KG_OK;
}

// image: device bytes [H][W][3]; ys / xs: HOST int [ny] / [nx]; out: device float32 [ny * nx][3][th][tw], 16-byte aligned, tw % 4 == 0
extern "C" int kg_tile_cut(const void* image, int H, int W, const int* ys, int ny, const int* xs, int nx, int th, int tw, float* out, void* stream) {
    KG_CHECK_ARG(image && out, "kg_tile_cut: null pointer");
    TileGrid g;
    KG_TRY(tile_grid_check("kg_tile_cut", ys, ny, xs, nx, th, tw, H, W, &g));
    KG_CHECK_ARG(tw % 4 == 0, "kg_tile_cut: tw %d is not a multiple of 4", tw);
    KG_CHECK_ARG(kg_aligned(out, 15), "kg_tile_cut: out must be 16-byte aligned");
    hipLaunchKernelGGL(tile_cut_kernel, dim3((unsigned)kg_cdiv((long)th * (tw >> 2), 256), (unsigned)nx, (unsigned)ny), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)image, H, W, g, th, tw, out);
    KG_CHECK_LAUNCH("tile_cut");
    return KG_OK;
}

// words: device [n][ld_words] of H x W masks, changed in place: every bit at y >= vh or x >= vw is cleared
extern "C" int kg_bitmask_clip(void* words, long ld_words, int n, int H, int W, int vh, int vw, void* stream) {
    KG_CHECK_ARG(H > 0 && W > 0 && n >= 0, "kg_bitmask_clip: bad size (H %d, W %d, n %d)", H, W, n);
    KG_CHECK_ARG(vh >= 0 && vh <= H && vw >= 0 && vw <= W, "kg_bitmask_clip: window %d x %d outside the %d x %d masks", vh, vw, H, W);
    const long nw = (long)H * ((W + 63) / 64);
    KG_TRY(kg_check_bits_ld("kg_bitmask_clip", H, W, ld_words));
    KG_CHECK_ARG(words || n == 0, "kg_bitmask_clip: null pointer (words)");
    KG_CHECK_ARG(kg_aligned(words, 15), "kg_bitmask_clip: words must be 16-byte aligned");
    KG_CHECK_ARG((long)n <= LONG_MAX / 8 / ld_words, "kg_bitmask_clip: n * ld_words too large");
    if (n == 0 || (vh == H && vw == W)) return KG_OK;
    hipLaunchKernelGGL(bitmask_clip_kernel, dim3((unsigned)kg_cdiv(nw, 256), (unsigned)(n < 65535 ? n : 65535)), dim3(256), 0, (hipStream_t)stream,
                       (unsigned long long*)words, ld_words, n, H, W, vh, vw);
    KG_CHECK_LAUNCH("bitmask_clip");
    return KG_OK;
}

// tile_labels: device int32 [ny * nx][th][tw], values >= 0; ys / xs: HOST int [ny] / [nx]; labels: device int32 [H][W]
extern "C" int kg_tile_stitch(const int* tile_labels, const int* ys, int ny, const int* xs, int nx, int th, int tw, int H, int W, int* labels,
                              void* stream) {
    KG_CHECK_ARG(tile_labels && labels, "kg_tile_stitch: null pointer");
    TileGrid g;
    KG_TRY(tile_grid_check("kg_tile_stitch", ys, ny, xs, nx, th, tw, H, W, &g));
    KG_CHECK_ARG(kg_cdiv(W, 256) <= 65535, "kg_tile_stitch: W %d too large", W);
    hipLaunchKernelGGL(tile_stitch_kernel, dim3((unsigned)H, (unsigned)kg_cdiv(W, 256)), dim3(256), 0, (hipStream_t)stream, tile_labels, g, ny, nx, th,
                       tw, H, W, labels);
    KG_CHECK_LAUNCH("tile_stitch");
    return KG_OK;
}

// labels: device int32 [H][W]; jobs: device int32 [n][5] = (id, y1, x1, y2, x2), written and validated by the caller; area_full: device
// int64 [n] or NULL; table: device int64 [n][8]
extern "C" int kg_label_table(const int* labels, int H, int W, const int* jobs, int n, const long long* area_full, long long* table, void* stream) {
    KG_CHECK_ARG(H > 0 && W > 0 && n >= 0, "kg_label_table: bad size (H %d, W %d, n %d)", H, W, n);
    KG_TRY(kg_check_map_size("kg_label_table", H, W));
    KG_CHECK_ARG(labels, "kg_label_table: null pointer (labels)");
    KG_CHECK_ARG((jobs && table) || n == 0, "kg_label_table: null pointer (jobs / table)");
    KG_CHECK_ARG(kg_aligned(labels, 3) && kg_aligned(jobs, 3) && kg_aligned(area_full, 7) && kg_aligned(table, 7), "kg_label_table: misaligned pointer");
    if (n == 0) return KG_OK;
    hipLaunchKernelGGL(label_table_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, labels, H, W, jobs, area_full, table);
    KG_CHECK_LAUNCH("label_table");
    return KG_OK;
}
