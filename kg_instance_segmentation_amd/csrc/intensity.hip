// intensity.hip -- per-instance intensity order statistics and histograms of instance label maps on gfx950 (intensity.py): what the sums
// of measure.hip cannot give, because an order statistic does not add.
//   kg_label_quantiles   per job {img, id, box} and image channel: the pixel count n and, for each of Q rationals num / den, the two order
//                        statistics v[k_lo], v[k_hi] around the rank num (n - 1) / den of the sorted values of the job's pixels
//   kg_label_histograms  per job {img, id, box, channel, shift, prefix}: the 256-bin histogram of (value >> shift) over the job's pixels
//
// Both count into an LDS histogram of 256 bins with LDS integer atomics: the sums are integers, so the order in which the atomics land
// changes nothing.  No atomics on global memory; every output element is written with a plain vector store.
//
// The index rule of label_common.h holds with the one exception it lists for this file: an LDS BIN INDEX FORMED FROM A PIXEL VALUE.  It
// is bounded where it is made -- `& 255` (min(., 255) first where the last bin collects) immediately before use, inside int [256] -- and
// so is the low-byte histogram a rank selected (an LDS row index read back from LDS, used only inside (unsigned)s < (unsigned)KEEP).
// No GLOBAL address depends on a pixel or label value: the job table's box is clamped before any address is formed, its image index,
// channel and shift are used only inside unsigned range predicates that empty the box when they fail, and the quantile table is read
// at fixed positions and only compared and multiplied (a row with den <= 0, num < 0 or num > den is not divided by: lo = hi = 0).
#include "label_common.h"

#define KG_IQ_MAX_Q 8                   // quantiles per call: 16 ranks per channel
#define KG_IQ_RANKS (2 * KG_IQ_MAX_Q)
#define KG_IQ_DEN_MAX 1000000           // num (n - 1) < 2^20 2^30: the 64-bit product cannot overflow
#define KG_IQ_KEEP 4                    // low-byte histograms a 16-bit channel keeps per walk (LDS budget)

// In-place inclusive scan of NH histograms: thread t owns bin t of each.  A shuffle scan per wave, the four wave totals through LDS.
// The caller has synchronised after the last atomic; on return hist[i][t] = the count of the bins 0 .. t, visible to every thread.
template <int NH>
__device__ __forceinline__ void iq_scan(int (*hist)[256], int (*wtot)[4]) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int v[NH];
#pragma unroll
    for (int i = 0; i < NH; ++i) {
        int x = hist[i][t];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(x, o);
            if (lane >= o) x += u;
        }
        v[i] = x;
        if (lane == 63) wtot[i][wave] = x;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NH; ++i) {
        int off = 0;
#pragma unroll
        for (int w = 0; w < 3; ++w) off += w < wave ? wtot[i][w] : 0;
        hist[i][t] = v[i] + off;
    }
    __syncthreads();
}

// One block per job (the grid strides beyond KG_LABEL_MAX_BLOCKS jobs and reuses its LDS: everything is cleared per job).
//   walk 1   every channel's histogram of the value (8-bit) or of its high byte (16-bit): C histograms
//   select   scan; threads 0 .. 2Q - 1 turn the table into ranks (the only divisions); the thread whose bin holds rank k
//            (excl <= k < incl) owns it: the answer for 8-bit, the high byte and the residual rank k - excl for 16-bit
//   walk 2+  16-bit only: per channel the DISTINCT selected high bytes are compacted (several ranks in one bin is the usual case) and
//            KEEP of them per walk get a low-byte histogram; the residual ranks are selected the same way.  ceil(distinct / KEEP) walks.
template <int C, typename T>
__global__ __launch_bounds__(256) void label_quantiles_kernel(const int* __restrict__ labels, int nimg, int H, int W, const T* __restrict__ image,
                                                              const int* __restrict__ jobs, int m, const int* __restrict__ qtab, int Q,
                                                              int* __restrict__ out) {
    constexpr bool WIDE = sizeof(T) == 2;
    constexpr int K = WIDE ? KG_IQ_KEEP : 1;
    constexpr int NH = C * K;
    __shared__ int hist[NH][256];
    __shared__ int wtot[NH][4];
    __shared__ int rank[KG_IQ_RANKS];                                  // the rank k of column r; -1: none (n == 0 or a bad table row)
    __shared__ int res[C][KG_IQ_RANKS];
    __shared__ int selhi[C][KG_IQ_RANKS], resid[C][KG_IQ_RANKS], slot[C][KG_IQ_RANKS], dist[C][KG_IQ_RANKS], ndist[C];
    const int t = threadIdx.x;
    const int R = 2 * Q, ncol = 1 + R;                                 // 1 <= Q <= 8: checked on the host
    for (long j = blockIdx.x; j < m; j += gridDim.x) {
        const int* jb = jobs + j * 6;
        const int img = jb[0], id = jb[1];
        const bool ok = (unsigned)img < (unsigned)nimg;                // the only use of img before it scales an address
        KgBox b = kg_job_box(jb + 2, H, W);
        if (!ok) b.h = b.w = 0;
        const long base = ok ? (long)img * H * W : 0;                  // img < nimg: base + H * W <= nimg * H * W <= 2^31 - 1
#pragma unroll
        for (int c = 0; c < C; ++c) hist[c][t] = 0;
        if (t < C * KG_IQ_RANKS) { (&res[0][0])[t] = 0; (&selhi[0][0])[t] = -1; }
        __syncthreads();
        kg_box_walk(b, [&](int Y, int X) {
            const long p = base + (long)Y * W + X;
            if (labels[p] == id) {
                const T* px = image + p * C;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const int v = (int)px[c];
                    atomicAdd(&hist[c][(WIDE ? v >> 8 : v) & 255], 1);
                }
            }
        });
        __syncthreads();
        iq_scan<C>(hist, wtot);
        const int n = hist[0][255];                                    // every channel counts the same pixels
        if (t < R) {
            const int num = qtab[2 * (t >> 1)], den = qtab[2 * (t >> 1) + 1];
            int k = -1;
            if (n > 0 && den > 0 && num >= 0 && num <= den) {
                const long long tt = (long long)num * (n - 1);
                const long long lo = tt / den;
                k = (int)(lo + ((t & 1) && tt - lo * den != 0));       // <= n - 1, since num <= den
            }
            rank[t] = k;
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int incl = hist[c][t], excl = t ? hist[c][t - 1] : 0;
            if (incl > excl)
                for (int r = 0; r < R; ++r) {
                    const int k = rank[r];
                    if (k >= excl && k < incl) {
                        if constexpr (WIDE) { selhi[c][r] = t; resid[c][r] = k - excl; }
                        else res[c][r] = t;
                    }
                }
        }
        __syncthreads();
        if constexpr (WIDE) {
            if (t < C) {                                               // the distinct selected high bytes of channel t, in rank order
                int nd = 0;
                for (int r = 0; r < R; ++r) {
                    const int hb = selhi[t][r];
                    int s = -1;
                    if (hb >= 0) {
                        for (int u = 0; u < nd; ++u) s = dist[t][u] == hb ? u : s;
                        if (s < 0) { s = nd; dist[t][nd++] = hb; }
                    }
                    slot[t][r] = s;
                }
                ndist[t] = nd;
            }
            __syncthreads();
            int most = 0;
#pragma unroll
            for (int c = 0; c < C; ++c) most = ndist[c] > most ? ndist[c] : most;
            for (int p0 = 0; p0 < most; p0 += K) {                     // uniform: most comes from LDS after a barrier
                int sel[C][K];
#pragma unroll
                for (int c = 0; c < C; ++c)
#pragma unroll
                    for (int s = 0; s < K; ++s) {
                        hist[c * K + s][t] = 0;
                        sel[c][s] = p0 + s < ndist[c] ? dist[c][p0 + s] : -1;
                    }
                __syncthreads();
                kg_box_walk(b, [&](int Y, int X) {
                    const long p = base + (long)Y * W + X;
                    if (labels[p] == id) {
                        const T* px = image + p * C;
#pragma unroll
                        for (int c = 0; c < C; ++c) {
                            const int v = (int)px[c], hb = v >> 8;
                            int s = -1;
#pragma unroll
                            for (int u = 0; u < K; ++u) s = hb == sel[c][u] ? u : s;
                            if (s >= 0) atomicAdd(&hist[c * K + s][v & 255], 1);
                        }
                    }
                });
                __syncthreads();
                iq_scan<NH>(hist, wtot);
#pragma unroll
                for (int c = 0; c < C; ++c)
                    for (int r = 0; r < R; ++r) {
                        const int s = slot[c][r] - p0;
                        if ((unsigned)s < (unsigned)K) {               // the rank's high byte is one of this walk's
                            const int kk = resid[c][r];
                            const int incl = hist[c * K + s][t], excl = t ? hist[c * K + s][t - 1] : 0;
                            if (kk >= excl && kk < incl) res[c][r] = (selhi[c][r] << 8) | t;
                        }
                    }
                __syncthreads();                                       // hist is cleared again by the next walk
            }
        }
        if (t < C * ncol) {
            const int c = t / ncol, i = t - c * ncol;
            out[(j * C + c) * ncol + i] = i == 0 ? n : res[c][i - 1];
        }
        __syncthreads();                                               // res, rank and hist are written again by the block's next job
    }
}

// One block per histogram job: the same walk, one LDS histogram of the one named channel, 256 plain stores.
template <typename T>
__global__ __launch_bounds__(256) void label_histograms_kernel(const int* __restrict__ labels, int nimg, int H, int W, const T* __restrict__ image,
                                                               int C, const int* __restrict__ jobs, int m, int* __restrict__ out) {
    __shared__ int hist[256];
    const int t = threadIdx.x;
    for (long j = blockIdx.x; j < m; j += gridDim.x) {
        const int* jb = jobs + j * 9;
        const int img = jb[0], id = jb[1], channel = jb[6], shift = jb[7], prefix = jb[8];
        const bool ok = (unsigned)img < (unsigned)nimg && (unsigned)channel < (unsigned)C && (unsigned)shift <= 8u;
        KgBox b = kg_job_box(jb + 2, H, W);
        if (!ok) b.h = b.w = 0;
        const long base = ok ? (long)img * H * W : 0;
        const int ch = ok ? channel : 0, sh = ok ? shift : 0;
        hist[t] = 0;
        __syncthreads();
        kg_box_walk(b, [&](int Y, int X) {
            const long p = base + (long)Y * W + X;
            if (labels[p] == id) {
                const int w = (int)image[p * C + ch] >> sh;
                if (prefix < 0) atomicAdd(&hist[(w < 255 ? w : 255) & 255], 1);
                else if ((w >> 8) == prefix) atomicAdd(&hist[w & 255], 1);
            }
        });
        __syncthreads();
        out[j * 256 + t] = hist[t];
        __syncthreads();                                               // hist is cleared again by the block's next job
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
template <int C, typename T>
static void iq_launch(const int* labels, int nimg, int H, int W, const void* image, const int* jobs, int m, const int* qtab, int Q, int* out,
                      hipStream_t stream) {
    hipLaunchKernelGGL((label_quantiles_kernel<C, T>), dim3(kg_grid_cap(m)), dim3(256), 0, stream, labels, nimg, H, W, (const T*)image, jobs, m,
                       qtab, Q, out);
}

// the checks both entries share; fn = the entry's name
static int iq_check(const char* fn, const int* labels, int nimg, int H, int W, const void* image, int channels, int elem_bytes, const int* jobs,
                    int m, const int* out) {
    KG_TRY(kg_check_job_stack(fn, labels, nimg, H, W, jobs, m));       // H, W <= KG_LABEL_MAX_SIDE: every count and rank of a box fits int32
    KG_TRY(kg_check_image(fn, image, channels, elem_bytes));
    KG_CHECK_ARG(out || m == 0, "%s: null pointer (out)", fn);
    KG_CHECK_ARG(kg_aligned(out, 3), "%s: misaligned pointer", fn);
    return KG_OK;
}

// labels: device int32 [nimg][H][W]; image: device [nimg][H][W][channels] of elem_bytes-byte unsigned elements; jobs: device int32 [m][6] =
// (img, id, y1, x1, y2, x2); qtab: device int32 [Q][2] = (num, den); out: device int32 [m][channels][1 + 2 Q]
extern "C" int kg_label_quantiles(const int* labels, int nimg, int H, int W, const void* image, int channels, int elem_bytes, const int* jobs, int m,
                                  const int* qtab, int Q, int* out, void* stream) {
    KG_TRY(iq_check("kg_label_quantiles", labels, nimg, H, W, image, channels, elem_bytes, jobs, m, out));
    KG_CHECK_ARG(Q >= 1 && Q <= KG_IQ_MAX_Q, "kg_label_quantiles: Q %d (1 .. %d)", Q, KG_IQ_MAX_Q);
    KG_CHECK_ARG(qtab, "kg_label_quantiles: null pointer (qtab)");
    KG_CHECK_ARG(kg_aligned(qtab, 3), "kg_label_quantiles: misaligned pointer");
    if (m == 0) return KG_OK;
    hipStream_t s = (hipStream_t)stream;
    switch (channels * 2 + (elem_bytes == 2)) {
        case 2: iq_launch<1, unsigned char>(labels, nimg, H, W, image, jobs, m, qtab, Q, out, s); break;
        case 3: iq_launch<1, unsigned short>(labels, nimg, H, W, image, jobs, m, qtab, Q, out, s); break;
        case 4: iq_launch<2, unsigned char>(labels, nimg, H, W, image, jobs, m, qtab, Q, out, s); break;
        case 5: iq_launch<2, unsigned short>(labels, nimg, H, W, image, jobs, m, qtab, Q, out, s); break;
        case 6: iq_launch<3, unsigned char>(labels, nimg, H, W, image, jobs, m, qtab, Q, out, s); break;
        case 7: iq_launch<3, unsigned short>(labels, nimg, H, W, image, jobs, m, qtab, Q, out, s); break;
        case 8: iq_launch<4, unsigned char>(labels, nimg, H, W, image, jobs, m, qtab, Q, out, s); break;
        default: iq_launch<4, unsigned short>(labels, nimg, H, W, image, jobs, m, qtab, Q, out, s); break;
    }
    KG_CHECK_LAUNCH("label_quantiles");
    return KG_OK;
}

// jobs: device int32 [m][9] = (img, id, y1, x1, y2, x2, channel, shift, prefix); out: device int32 [m][256]
extern "C" int kg_label_histograms(const int* labels, int nimg, int H, int W, const void* image, int channels, int elem_bytes, const int* jobs,
                                   int m, int* out, void* stream) {
    KG_TRY(iq_check("kg_label_histograms", labels, nimg, H, W, image, channels, elem_bytes, jobs, m, out));
    if (m == 0) return KG_OK;
    hipStream_t s = (hipStream_t)stream;
    if (elem_bytes == 2)
        hipLaunchKernelGGL((label_histograms_kernel<unsigned short>), dim3(kg_grid_cap(m)), dim3(256), 0, s, labels, nimg, H, W,
                           (const unsigned short*)image, channels, jobs, m, out);
    else
        hipLaunchKernelGGL((label_histograms_kernel<unsigned char>), dim3(kg_grid_cap(m)), dim3(256), 0, s, labels, nimg, H, W,
                           (const unsigned char*)image, channels, jobs, m, out);
    KG_CHECK_LAUNCH("label_histograms");
    return KG_OK;
}
