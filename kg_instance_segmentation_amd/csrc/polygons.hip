// polygons.hip -- polygon annotations to a label map on gfx950: the exact tiled polygon fill (polygons.py).
//   kg_polygons_fill     an edge table, per-tile item lists -> out[nimg][H][W] (the value of the first covering item, else background) and,
//                        when asked for, cover[nimg][H][W] (the number of distinct rows that cover the pixel)
//
// Semantics (include/kgnet_hip.h is the normative text).  Fixed point F = 256: a vertex is q = rint(256 v), the centre of pixel (y, x) is
// (cx, cy) = (256 x + 128, 256 y + 128).  An edge row is (x0, y0, x1, y1) with y0 < y1 (ordered upward, horizontal edges dropped by the
// host); it COUNTS for a centre iff
//     y0 <= cy < y1  and  (x1 - x0) * (cy - y0) > (cx - x0) * (y1 - y0)          (32 x 32 -> 64 bit products)
// i.e. its intersection with the scanline lies strictly right of the centre.  An item {value, edge_first, edge_count, row} is one part:
// it covers a pixel iff the number of its counting edges is odd.  out = the value of the first item of the tile's list that covers the
// pixel; cover += 1 for a covering item whose row differs from the row of the last item the pixel counted.
//
// A gather with no atomics: one block of 256 threads per KG_POLY_TILE_H x KG_POLY_TILE_W tile (the grid strides when there are more tiles
// than KG_LABEL_MAX_BLOCKS), wave w on rows 8 w .. 8 w + 7 of the tile, lane l on column l: a wave's store is 64 consecutive pixels of a
// row, and every pixel of the map is written once by one lane whatever order the blocks run in.
//   WALK    the items tile_ptr[t] .. tile_ptr[t + 1] in list order, the same in every thread of the block.
//   STAGE   the item's edges in chunks of KG_POLY_EDGE_CHUNK, one edge (16 bytes) per thread.  A thread keeps its edge when [y0, y1)
//           meets the tile's centre rows and max(x0, x1) lies right of the tile's first centre column -- no other edge can count here --
//           and the kept edges of a wave go, compacted by ballot and popcount, to the wave's 64 slots of LDS.  The slots are
//           double-buffered by the parity of the chunk: one barrier per chunk.
//   TEST    every lane runs the crossing test of its 8 pixels against the staged edges.  All lanes read the same LDS address (a
//           broadcast, no bank conflict); cx is one per lane, so the right side is one product per edge and the left side advances by
//           256 (x1 - x0) per row.  The parities are 8 bits of a register.
//
// The index rule of label_common.h holds here, with ONE new exception, two levels of caller-written tables:
//   - tile_ptr[t], tile_ptr[t + 1] are each clamped to [0, n_items] before use, and a decreasing pair is an empty range;
//   - an item's edge_first, edge_count are used only inside the 64-bit unsigned predicates first <= E and count <= E - first; a failing
//     predicate empties the item.
// No address depends on an edge coordinate, a value or a row, so a wrong table can produce wrong pixels but cannot reach outside edges,
// items, out or cover.  Coordinate differences of a wrong edge table wrap (unsigned arithmetic) instead of overflowing.
#include "label_common.h"

#define KG_POLY_TILE_H 32
#define KG_POLY_TILE_W 64
#define KG_POLY_EDGE_CHUNK 256          // edges staged per barrier: one per thread
#define KG_POLY_ROWS (KG_POLY_TILE_H / 4)

static_assert(KG_POLY_TILE_W == 64 && KG_POLY_TILE_H % 4 == 0 && KG_POLY_ROWS <= 32 && KG_POLY_EDGE_CHUNK == 256,
              "a wave owns 64 consecutive pixels of a row, a block of 256 threads stages one edge per thread");

__device__ __forceinline__ int kg_poly_sub(int a, int b) { return (int)((unsigned)a - (unsigned)b); }   // wraps, never overflows

template <bool COVER>
__global__ __launch_bounds__(256) void polygons_fill_kernel(const int4* __restrict__ edges, unsigned long long E, const int4* __restrict__ items,
                                                            int n_items, const int* __restrict__ tile_ptr, long ntiles, int tiles_y, int tiles_x,
                                                            int H, int W, int background, int* __restrict__ out, int* __restrict__ cover) {
    __shared__ int4 staged[2][4][64];
    __shared__ int kept[2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const long per_img = (long)tiles_y * tiles_x;
    unsigned walk = 0;                                                 // the chunk counter: the same in every thread
    for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long img = t / per_img;
        const int rest = (int)(t - img * per_img), ty = rest / tiles_x, tx = rest - ty * tiles_x;
        const int y_first = ty * KG_POLY_TILE_H, x_first = tx * KG_POLY_TILE_W;
        const int y_end = y_first + KG_POLY_TILE_H < H ? y_first + KG_POLY_TILE_H : H;      // > y_first: the tile meets the map
        const int cy_first = 256 * y_first + 128, cy_last = 256 * (y_end - 1) + 128, cx_first = 256 * x_first + 128;
        const int cx = 256 * (x_first + lane) + 128, cy0 = 256 * (y_first + wave * KG_POLY_ROWS) + 128;
        int lo = tile_ptr[t], hi = tile_ptr[t + 1];
        lo = lo < 0 ? 0 : lo > n_items ? n_items : lo;                 // the clamped range of the first table level
        hi = hi < 0 ? 0 : hi > n_items ? n_items : hi;
        int val[KG_POLY_ROWS], cnt[KG_POLY_ROWS], last[KG_POLY_ROWS];
        unsigned has = 0;                                              // bit k: pixel k has its value, or lies outside the map
#pragma unroll
        for (int k = 0; k < KG_POLY_ROWS; ++k) {
            val[k] = background; cnt[k] = 0; last[k] = 0;
            has |= (unsigned)(x_first + lane >= W || y_first + wave * KG_POLY_ROWS + k >= H) << k;
        }
        for (int i = lo; i < hi; ++i) {
            const int4 it = items[i];                                  // {value, edge_first, edge_count, row}
            const unsigned long long first = (unsigned long long)(long long)it.y, count = (unsigned long long)(long long)it.z;
            const bool ok = first <= E && count <= E - first;          // the second table level: a failing predicate empties the item
            const unsigned n = ok ? (unsigned)count : 0u;              // <= E <= INT_MAX
            unsigned odd = 0;
            for (unsigned c0 = 0; c0 < n; c0 += KG_POLY_EDGE_CHUNK) {
                const int b = walk++ & 1;
                bool keep = false;
                int4 e = {0, 0, 0, 0};
                if (c0 + threadIdx.x < n) {
                    e = edges[first + c0 + threadIdx.x];               // first + c0 + threadIdx.x < first + count <= E
                    const int xm = e.x > e.z ? e.x : e.z;
                    keep = e.y <= cy_last && e.w > cy_first && xm > cx_first;
                }
                const unsigned long long bk = __ballot(keep);
                if (keep) staged[b][wave][__popcll(bk & below)] = e;
                if (lane == 0) kept[b][wave] = __popcll(bk);
                __syncthreads();
                for (int w = 0; w < 4; ++w) {
                    const int m = kept[b][w];
                    for (int j = 0; j < m; ++j) {
                        const int4 g = staged[b][w][j];
                        const int dx = kg_poly_sub(g.z, g.x), dy = kg_poly_sub(g.w, g.y);
                        const long long rhs = (long long)kg_poly_sub(cx, g.x) * dy, step = (long long)dx * 256;
                        long long lhs = (long long)dx * kg_poly_sub(cy0, g.y);
                        int cy = cy0;
#pragma unroll
                        for (int k = 0; k < KG_POLY_ROWS; ++k) {
                            odd ^= (unsigned)(g.y <= cy && cy < g.w && lhs > rhs) << k;
                            lhs += step; cy += 256;
                        }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < KG_POLY_ROWS; ++k) {
                if ((odd >> k) & 1u) {
                    if (!((has >> k) & 1u)) val[k] = it.x;
                    if constexpr (COVER) {
                        if (cnt[k] == 0 || last[k] != it.w) { ++cnt[k]; last[k] = it.w; }
                    }
                }
            }
            has |= odd;
            if constexpr (!COVER) {                                    // every pixel of the tile has its value: the rest cannot change one
                if (__syncthreads_and(has == (1u << KG_POLY_ROWS) - 1u)) break;
            }
        }
        const int x = x_first + lane;
        if (x < W) {
#pragma unroll
            for (int k = 0; k < KG_POLY_ROWS; ++k) {
                const int y = y_first + wave * KG_POLY_ROWS + k;
                if (y < H) {
                    const long p = (img * H + y) * W + x;              // img < nimg, y < H, x < W: inside the stack
                    out[p] = val[k];
                    if constexpr (COVER) cover[p] = cnt[k];
                }
            }
        }
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// edges: device int32 [E][4] = (x0, y0, x1, y1); items: device int32 [n_items][4] = {value, edge_first, edge_count, row}; tile_ptr: device
// int32 [nimg * tiles + 1], tiles = ceil(H / KG_POLY_TILE_H) * ceil(W / KG_POLY_TILE_W); out, cover: device int32 [nimg][H][W]
extern "C" int kg_polygons_fill(const int* edges, int E, const int* items, int n_items, const int* tile_ptr, int nimg, int H, int W, int background,
                                int* out, int* cover, void* stream) {
    const char* fn = "kg_polygons_fill";
    KG_CHECK_ARG(nimg > 0 && H > 0 && W > 0, "%s: bad size (nimg %d, H %d, W %d)", fn, nimg, H, W);
    KG_CHECK_ARG(E >= 0 && n_items >= 0, "%s: E %d, n_items %d", fn, E, n_items);
    // H, W <= 2^15: a centre coordinate stays below 2^23 + 2^7
    KG_CHECK_ARG(H <= KG_LABEL_MAX_SIDE && W <= KG_LABEL_MAX_SIDE, "%s: H %d, W %d exceed %d", fn, H, W, KG_LABEL_MAX_SIDE);
    KG_TRY(kg_check_stack_size(fn, nimg, H, W));
    KG_CHECK_ARG(out, "%s: null pointer (out)", fn);
    KG_CHECK_ARG(tile_ptr, "%s: null pointer (tile_ptr)", fn);
    KG_CHECK_ARG(edges || E == 0, "%s: null pointer (edges)", fn);
    KG_CHECK_ARG(items || n_items == 0, "%s: null pointer (items)", fn);
    KG_CHECK_ARG(kg_aligned(edges, 15) && kg_aligned(items, 15), "%s: misaligned pointer (edges and items: 16 bytes)", fn);
    KG_CHECK_ARG(kg_aligned(tile_ptr, 3) && kg_aligned(out, 3) && kg_aligned(cover, 3), "%s: misaligned pointer", fn);
    const int tiles_y = (H + KG_POLY_TILE_H - 1) / KG_POLY_TILE_H, tiles_x = (W + KG_POLY_TILE_W - 1) / KG_POLY_TILE_W;
    const long ntiles = (long)nimg * tiles_y * tiles_x;                // <= nimg * H * W <= 2^31 - 1
    const long mbytes = 4L * nimg * H * W, ebytes = 16L * E, ibytes = 16L * n_items, pbytes = 4L * (ntiles + 1);
    KG_CHECK_ARG(kg_apart(out, mbytes, cover, mbytes), "%s: out aliases cover", fn);
    KG_CHECK_ARG(kg_apart(out, mbytes, edges, ebytes) && kg_apart(out, mbytes, items, ibytes) && kg_apart(out, mbytes, tile_ptr, pbytes),
                 "%s: out aliases a table", fn);
    KG_CHECK_ARG(kg_apart(cover, mbytes, edges, ebytes) && kg_apart(cover, mbytes, items, ibytes) &&
                     kg_apart(cover, mbytes, tile_ptr, pbytes), "%s: cover aliases a table", fn);
    const dim3 grid(kg_grid_cap(ntiles));
    if (cover)
        hipLaunchKernelGGL(polygons_fill_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const int4*)edges, (unsigned long long)E,
                           (const int4*)items, n_items, tile_ptr, ntiles, tiles_y, tiles_x, H, W, background, out, cover);
    else
        hipLaunchKernelGGL(polygons_fill_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const int4*)edges, (unsigned long long)E,
                           (const int4*)items, n_items, tile_ptr, ntiles, tiles_y, tiles_x, H, W, background, out, (int*)nullptr);
    KG_CHECK_LAUNCH("polygons_fill");
    return KG_OK;
}
