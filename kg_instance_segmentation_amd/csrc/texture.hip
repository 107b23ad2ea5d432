// texture.hip -- per-instance grey-level co-occurrence matrices of instance label maps on gfx950 (texture.py): what an instance looks like
// inside.  A co-occurrence count is a function of PAIRS of pixels: no function of measure.hip's sums or of intensity.hip's bins.
//   kg_label_glcm   per job {img, id, box, channel, distance, lo, span}: the four L x L matrices G[k][i][j] = the number of pixels p of the
//                   job (inside the clamped box, labels == id) whose partner p + o_k lies inside the MAP, carries the id too, and whose
//                   levels are lev(p) = i, lev(p + o_k) = j; o_k = (0, d), (d, d), (d, 0), (d, -d)
//
// The matrices live in LDS (int [4][1024], 16 KiB) and are filled with LDS integer atomics: the counts are integers, so the order in which
// the atomics land changes nothing.  No atomics on global memory; every output element is written with a plain vector store.
//
// Two routes, chosen per workgroup from the clamped box and d alone, giving the same rows:
//   staged   (h + d) * (w + 2 d) <= 16384: the rectangle of rows y1 .. y2 - 1 + d and columns x1 - d .. x2 - 1 + d is staged into LDS, one
//            byte per pixel -- the level where the pixel lies inside the map and carries the id, 0xFF otherwise -- so that every pixel is
//            loaded from global memory and divided ONCE; the pair pass reads LDS only.
//   direct   a larger box: the same pair pass straight from global memory (map and image are cache-resident at these sizes).
//
// The index rule of label_common.h holds with the exception it lists for intensity.hip and this file: an LDS BIN INDEX FORMED FROM A PIXEL
// VALUE.  Both levels are bounded where the index is made -- min(., L - 1) immediately before use, so i * L + j <= L * L - 1 <= 1023 inside
// int [4][1024].  The staged byte's index is a box-local coordinate: (yy + dy) * sw + xx + dx with 0 <= yy + dy < h + d, 0 <= xx + dx <
// w + 2 d = sw, below (h + d) * sw <= 16384.  No GLOBAL address depends on a pixel or label value: the job table's box is clamped before
// any address is formed; img, channel, distance and span are used only inside the predicates that empty the box when they fail; lo is
// only subtracted and compared.
#include "label_common.h"

#define KG_TX_MAX_L 32
#define KG_TX_CELLS (KG_TX_MAX_L * KG_TX_MAX_L)
#define KG_TX_MAX_D 32
#define KG_TX_STAGE 16384               // staged bytes: with the matrices 32 KiB of static LDS
#define KG_TX_NONE 0xFF                 // a staged pixel outside the map or of another label

// lev = min(max(v - lo, 0) * L / span, L - 1), span > 0.  Exact for every lo and span: 0 <= v <= 65535, so v - lo >= 0 fits 32 unsigned
// bits, and the product is formed in 32 bits only where it fits.
__device__ __forceinline__ int tx_level(int v, int lo, int span, int L) {
    if (v <= lo) return 0;
    const unsigned u = (unsigned)v - (unsigned)lo;
    if (u >= (unsigned)span) return L - 1;
    const unsigned q = u <= 0x03ffffffu ? u * (unsigned)L / (unsigned)span : (unsigned)((unsigned long long)u * (unsigned)L / (unsigned)span);
    return (int)q < L - 1 ? (int)q : L - 1;                            // u < span: q < L already
}

// the partner of direction k at distance d, as (dy, dx)
__device__ __forceinline__ void tx_offset(int k, int d, int& dy, int& dx) {
    dy = k == 0 ? 0 : d;
    dx = k == 2 ? 0 : k == 3 ? -d : d;
}

// One block per job (the grid strides beyond KG_LABEL_MAX_BLOCKS jobs and reuses its LDS: the matrices are cleared per job).
template <typename T>
__global__ __launch_bounds__(256) void label_glcm_kernel(const int* __restrict__ labels, int nimg, int H, int W, const T* __restrict__ image, int C,
                                                         const int* __restrict__ jobs, int m, int L, int* __restrict__ out) {
    __shared__ int G[4][KG_TX_CELLS];
    __shared__ unsigned char stage[KG_TX_STAGE];
    const int t = threadIdx.x;
    const int LL = L * L;                                              // 2 <= L <= 32: checked on the host
    for (long j = blockIdx.x; j < m; j += gridDim.x) {
        const int* jb = jobs + j * 10;
        const int img = jb[0], id = jb[1], channel = jb[6], distance = jb[7], lo = jb[8], span = jb[9];
        const bool ok = (unsigned)img < (unsigned)nimg && (unsigned)channel < (unsigned)C && (unsigned)(distance - 1) < (unsigned)KG_TX_MAX_D
                        && span > 0;
        KgBox b = kg_job_box(jb + 2, H, W);
        if (!ok) b.h = b.w = 0;
        const long base = ok ? (long)img * H * W : 0;                  // img < nimg: base + H * W <= nimg * H * W <= 2^31 - 1
        const int ch = ok ? channel : 0, d = ok ? distance : 1, sp = ok ? span : 1;
        for (int e = t; e < LL; e += 256) G[0][e] = G[1][e] = G[2][e] = G[3][e] = 0;
        __syncthreads();
        if (b.h > 0 && b.w > 0) {
            const int sw = b.w + 2 * d, sh = b.h + d;                  // <= 32768 + 64
            if ((long)sh * sw <= KG_TX_STAGE) {                        // uniform: the job table and the map size only
                const KgBox s{b.y1, b.x1 - d, sh, sw};
                kg_box_walk(s, [&](int Y, int X) {
                    int lev = KG_TX_NONE;
                    if ((unsigned)Y < (unsigned)H && (unsigned)X < (unsigned)W) {
                        const long p = base + (long)Y * W + X;
                        if (labels[p] == id) lev = tx_level((int)image[p * C + ch], lo, sp, L);
                    }
                    stage[(Y - s.y1) * sw + (X - s.x1)] = (unsigned char)lev;   // box-local: < sh * sw <= 16384
                });
                __syncthreads();
                kg_box_walk(b, [&](int Y, int X) {
                    const int at = (Y - b.y1) * sw + (X - b.x1) + d;
                    const int c = stage[at];
                    if (c != KG_TX_NONE) {
                        const int i = (c < L - 1 ? c : L - 1) * L;
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            int dy, dx;
                            tx_offset(k, d, dy, dx);
                            const int q = stage[at + dy * sw + dx];    // row < h + d, column in [0, w + 2 d)
                            if (q != KG_TX_NONE) atomicAdd(&G[k][i + (q < L - 1 ? q : L - 1)], 1);
                        }
                    }
                });
            } else {
                kg_box_walk(b, [&](int Y, int X) {
                    const long p = base + (long)Y * W + X;
                    if (labels[p] == id) {
                        const int c = tx_level((int)image[p * C + ch], lo, sp, L);
                        const int i = (c < L - 1 ? c : L - 1) * L;
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            int dy, dx;
                            tx_offset(k, d, dy, dx);
                            const int y = Y + dy, x = X + dx;
                            if (y < H && (unsigned)x < (unsigned)W) {  // y >= Y >= 0
                                const long pq = base + (long)y * W + x;
                                if (labels[pq] == id) {
                                    const int q = tx_level((int)image[pq * C + ch], lo, sp, L);
                                    atomicAdd(&G[k][i + (q < L - 1 ? q : L - 1)], 1);
                                }
                            }
                        }
                    }
                });
            }
        }
        __syncthreads();
        int* row = out + j * 4 * LL;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            for (int e = t; e < LL; e += 256) row[k * LL + e] = G[k][e];
        __syncthreads();                                               // G and stage are written again by the block's next job
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// labels: device int32 [nimg][H][W]; image: device [nimg][H][W][channels] of elem_bytes-byte unsigned elements; jobs: device int32 [m][10] =
// (img, id, y1, x1, y2, x2, channel, distance, lo, span); out: device int32 [m][4][levels][levels]
extern "C" int kg_label_glcm(const int* labels, int nimg, int H, int W, const void* image, int channels, int elem_bytes, const int* jobs, int m,
                             int levels, int* out, void* stream) {
    const char* fn = "kg_label_glcm";
    KG_TRY(kg_check_job_stack(fn, labels, nimg, H, W, jobs, m));       // H, W <= KG_LABEL_MAX_SIDE: every count of a box fits int32
    KG_TRY(kg_check_image(fn, image, channels, elem_bytes));
    KG_CHECK_ARG(levels >= 2 && levels <= KG_TX_MAX_L, "%s: levels %d (2 .. %d)", fn, levels, KG_TX_MAX_L);
    KG_CHECK_ARG(out || m == 0, "%s: null pointer (out)", fn);
    KG_CHECK_ARG(kg_aligned(out, 3), "%s: misaligned pointer", fn);
    if (m == 0) return KG_OK;
    hipStream_t s = (hipStream_t)stream;
    if (elem_bytes == 2)
        hipLaunchKernelGGL((label_glcm_kernel<unsigned short>), dim3(kg_grid_cap(m)), dim3(256), 0, s, labels, nimg, H, W,
                           (const unsigned short*)image, channels, jobs, m, levels, out);
    else
        hipLaunchKernelGGL((label_glcm_kernel<unsigned char>), dim3(kg_grid_cap(m)), dim3(256), 0, s, labels, nimg, H, W,
                           (const unsigned char*)image, channels, jobs, m, levels, out);
    KG_CHECK_LAUNCH("label_glcm");
    return KG_OK;
}
