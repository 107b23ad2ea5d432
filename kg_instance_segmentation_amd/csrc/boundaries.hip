// boundaries.hip -- boundary distances between two label maps on gfx950 (boundaries.py): for every source pixel of one instance the exact
// squared distance to the nearest outline pixel of another instance in another map.  Hausdorff, HD95, ASSD and the surface Dice are host
// float64 over these integers.
//   kg_label_border_counts  per job {img, dir, id_s, source box, id_t, target box, first}: {n_sources, n_targets, status}
//   kg_label_border_d2      per job: d2 of its k-th source into d2[first + k]
//
// BORDER pixel of id v in a map: a pixel that holds v and has one of its four side-neighbours outside the map or holding another value.
// The neighbours are read from the MAP, never from a box, and "outside the map" is decided by a predicate on the coordinates before the
// address exists; so the borders of pieces that tile a box are the border pixels of the box, piece by piece.
//
// The index rule of label_common.h holds here.  The job table is the one device-read table: both boxes are clamped to the map before any
// address is formed, img is used only inside (unsigned)img < (unsigned)nimg, dir and mode are predicates.  Label values are compared
// only.  LDS is indexed by compaction counts (prefix counts of predicates, bounded by the pixels of the target box <= 8192 and by the
// 512-slot queue, whose index is masked with 511 where it is made) and holds box-local and map coordinates, never a label.  The store of
// kg_label_border_d2 is of the kg_label_runs kind: first of the job table plus a prefix count of predicates, inside the 64-bit unsigned
// predicate first + k < D.  No atomics, no global scratch.
#include "label_common.h"

#define KG_BORDER_MAX_TARGET_PIXELS 8192   // the clamped target box of a job: every target fits one 32 KiB list
#define KG_BORDER_QUEUE 512                // source queue: fewer than 256 left over plus one chunk of at most 256

struct KgBorderMap { const int* map; int H, W; };
// the pixel (Y, X) of the map, inside it, holds v and is a border pixel of v
__device__ __forceinline__ bool kg_is_border(const KgBorderMap& g, int Y, int X, int v) {
    const int* p = g.map + (long)Y * g.W + X;
    return (Y == 0 || p[-g.W] != v) || (Y == g.H - 1 || p[g.W] != v) || (X == 0 || p[-1] != v) || (X == g.W - 1 || p[1] != v);
}

// The minimum of (ly - y)^2 + (lx - x)^2 over a list of 4 * nt4 words (y << 16 | x), y, x < 8192, read 16 bytes at a time: every lane of
// a wave passes the same address, so the read is a broadcast.  -1 for an empty list.
__device__ __forceinline__ int kg_nearest_d2(const int* tgt, int nt4, int ly, int lx) {
    if (nt4 == 0) return -1;
    const int4* t4 = (const int4*)tgt;
    int best = INT_MAX;
#pragma unroll 4
    for (int i = 0; i < nt4; ++i) {
        const int4 v = t4[i];
        int dy = ly - (v.x >> 16), dx = lx - (v.x & 0xffff), d = dy * dy + dx * dx;
        best = d < best ? d : best;
        dy = ly - (v.y >> 16); dx = lx - (v.y & 0xffff); d = dy * dy + dx * dx;
        best = d < best ? d : best;
        dy = ly - (v.z >> 16); dx = lx - (v.z & 0xffff); d = dy * dy + dx * dx;
        best = d < best ? d : best;
        dy = ly - (v.w >> 16); dx = lx - (v.w & 0xffff); d = dy * dy + dx * dx;
        best = d < best ? d : best;
    }
    return best;
}

// One block of 256 per job; the grid strides when there are more jobs than KG_LABEL_MAX_BLOCKS.  Both boxes are walked as flat row-major
// lists in chunks of 256 positions (consecutive lanes, consecutive x, as kg_box_walk does; all lanes stay in the loop for the ballots).
// TARGETS: the border pixels of id_t are compacted into tgt as box-local (y << 16 | x) words, in raster order: ballot, popcount below the
// lane, the wave totals through part, a carry across chunks.  The list is padded to a multiple of four with copies of its last word,
// which cannot change a minimum.  SOURCES: compacted the same way into a ring queue of map coordinates; whenever 256 are queued, or the
// walk ends, lane t takes the t-th of them and scans the whole list with 16-byte reads -- every lane reads the same address, a
// broadcast -- keeping the minimum in a register, and stores it at first + (sources flushed before) + t.  The count kernel is the same
// two walks without the list, the queue and the scan.
//
// part is double-buffered by the parity of the chunk (runlengths.hip says why one barrier per chunk is enough).  The queue needs one more
// barrier per flush, between its writes and its reads; a slot is rewritten only in a later chunk, behind that chunk's part barrier, which
// a thread reaches after its reads of the flush before.  tgt of the job before is rewritten behind the first part barrier of this job.
template <bool WRITE>
__global__ __launch_bounds__(256) void label_border_kernel(const int* __restrict__ a, const int* __restrict__ b, int nimg, int H, int W,
                                                           const int* __restrict__ jobs, int m, int mode, int* __restrict__ out, long long D) {
    __shared__ __attribute__((aligned(16))) int tgt[WRITE ? KG_BORDER_MAX_TARGET_PIXELS : 4];
    __shared__ int queue[WRITE ? KG_BORDER_QUEUE : 1];
    __shared__ int part[2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned walk = 0;
    for (long j = blockIdx.x; j < m; j += gridDim.x) {
        const int* jb = jobs + j * 13;
        const int img = jb[0], id_s = jb[2], id_t = jb[7];
        const bool swap = jb[1] != 0;
        KgBox sb = kg_job_box(jb + 3, H, W), tb = kg_job_box(jb + 8, H, W);
        const bool bad = !((unsigned)img < (unsigned)nimg) || sb.h == 0 || sb.w == 0 || tb.h == 0 || tb.w == 0;
        const bool big = !bad && (long)tb.h * tb.w > KG_BORDER_MAX_TARGET_PIXELS;
        int ns = 0, nt = 0;                                            // the carries: the same in every thread
        if (!bad && !big) {
            const long base = (long)img * H * W;                       // img < nimg here
            const KgBorderMap src{(swap ? b : a) + base, H, W}, dst{(swap ? a : b) + base, H, W};
            {   // ---- targets
                const int n = tb.h * tb.w, sy = 256 / tb.w, sx = 256 - sy * tb.w;
                int yy = (int)threadIdx.x / tb.w, xx = (int)threadIdx.x - yy * tb.w;
                for (int e0 = 0; e0 < n; e0 += 256) {
                    bool is = false;
                    if (yy < tb.h) {
                        const int Y = tb.y1 + yy, X = tb.x1 + xx;
                        is = dst.map[(long)Y * W + X] == id_t && kg_is_border(dst, Y, X, id_t);
                    }
                    const unsigned long long bt = __ballot(is);
                    int k = __popcll(bt & below);
                    int* q = part[walk++ & 1];
                    if (lane == 0) q[wave] = __popcll(bt);
                    __syncthreads();
                    int tot = 0;
                    for (int w = 0; w < 4; ++w) { if (w < wave) k += q[w]; tot += q[w]; }
                    if constexpr (WRITE) {
                        if (is) tgt[nt + k] = (yy << 16) | xx;         // nt + k < the pixels of the box <= 8192; yy, xx < 8192
                    }
                    nt += tot;
                    xx += sx; yy += sy;
                    if (xx >= tb.w) { xx -= tb.w; ++yy; }
                }
            }
            int nt4 = 0;
            if constexpr (WRITE) {
                __syncthreads();
                nt4 = (nt + 3) >> 2;                                   // <= 2048
                if (nt > 0 && threadIdx.x < 3 && nt + (int)threadIdx.x < 4 * nt4) tgt[nt + threadIdx.x] = tgt[nt - 1];
                // (read by the scan only behind the barrier that follows the first queue write)
            }
            {   // ---- sources
                const long long first = WRITE ? (long long)jb[12] : 0;
                const bool all = mode & 1, region = mode & 2;
                const long n = (long)sb.h * sb.w;
                const int sy = 256 / sb.w, sx = 256 - sy * sb.w;
                int yy = (int)threadIdx.x / sb.w, xx = (int)threadIdx.x - yy * sb.w;
                int head = 0, queued = 0;
                for (long e0 = 0; e0 < n; e0 += 256) {
                    bool is = false;
                    const int Y = sb.y1 + yy, X = sb.x1 + xx;
                    if (yy < sb.h) is = src.map[(long)Y * W + X] == id_s && (all || kg_is_border(src, Y, X, id_s));
                    const unsigned long long bs = __ballot(is);
                    int k = __popcll(bs & below);
                    int* q = part[walk++ & 1];
                    if (lane == 0) q[wave] = __popcll(bs);
                    __syncthreads();
                    int tot = 0;
                    for (int w = 0; w < 4; ++w) { if (w < wave) k += q[w]; tot += q[w]; }
                    if constexpr (WRITE) {
                        if (is) queue[(head + queued + k) & (KG_BORDER_QUEUE - 1)] = (Y << 16) | X;     // Y, X < 32768
                        queued += tot;                                 // < 256 + 256
                        const bool last = e0 + 256 >= n;
                        if (queued >= 256 || (last && queued > 0)) {
                            __syncthreads();
                            do {                                       // twice only at the end of the walk, with more than 256 queued
                                const int take = queued < 256 ? queued : 256;
                                if ((int)threadIdx.x < take) {
                                    const int s = queue[(head + (int)threadIdx.x) & (KG_BORDER_QUEUE - 1)];
                                    const int SY = s >> 16, SX = s & 0xffff;
                                    const int ly = SY - tb.y1, lx = SX - tb.x1;       // the source in the target box's frame
                                    int best;
                                    if (region && (unsigned)ly < (unsigned)tb.h && (unsigned)lx < (unsigned)tb.w && dst.map[(long)SY * W + SX] == id_t)
                                        best = 0;
                                    else
                                        best = kg_nearest_d2(tgt, nt4, ly, lx);
                                    const unsigned long long slot = (unsigned long long)(first + ns + (int)threadIdx.x);
                                    if (slot < (unsigned long long)D) out[slot] = best;
                                }
                                head = (head + take) & (KG_BORDER_QUEUE - 1);
                                queued -= take; ns += take;
                            } while (last && queued > 0);
                        }
                    } else {
                        ns += tot;
                    }
                    xx += sx; yy += sy;
                    if (xx >= sb.w) { xx -= sb.w; ++yy; }
                }
            }
        }
        if constexpr (!WRITE) {
            if (threadIdx.x == 0) { out[3 * j] = ns; out[3 * j + 1] = nt; out[3 * j + 2] = big ? 1 : 0; }
        }
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// (H, W <= KG_LABEL_MAX_SIDE: a source box holds <= 2^30 pixels, so the counts fit int32, and d2 <= 2 * 32767^2 < 2^31)
static int kg_check_border(const char* fn, const int* a, const int* b, int nimg, int H, int W, const int* jobs, int m, int mode, const int* out,
                           long out_bytes, bool need_out) {
    KG_TRY(kg_check_job_stack(fn, a, nimg, H, W, jobs, m));
    KG_TRY(kg_check_job_stack(fn, b, nimg, H, W, jobs, m));
    KG_CHECK_ARG(mode >= 0 && mode <= 3, "%s: mode %d (0 .. 3: bit 0 = all sources, bit 1 = region targets)", fn, mode);
    KG_CHECK_ARG(out || !need_out, "%s: null pointer (output)", fn);
    KG_CHECK_ARG(kg_aligned(out, 3), "%s: misaligned pointer (output)", fn);
    const long map_bytes = 4L * nimg * H * W;
    KG_CHECK_ARG(kg_apart(out, out_bytes, a, map_bytes) && kg_apart(out, out_bytes, b, map_bytes), "%s: the output aliases a label map", fn);
    KG_CHECK_ARG(kg_apart(out, out_bytes, jobs, 52L * m), "%s: the output aliases jobs", fn);
    return KG_OK;
}

// a, b: device int32 [nimg][H][W]; jobs: device int32 [m][13], written by the caller; counts: device int32 [m][3]
extern "C" int kg_label_border_counts(const int* a, const int* b, int nimg, int H, int W, const int* jobs, int m, int mode, int* counts,
                                      void* stream) {
    KG_TRY(kg_check_border("kg_label_border_counts", a, b, nimg, H, W, jobs, m, mode, counts, 12L * (m > 0 ? m : 0), m > 0));
    if (m == 0) return KG_OK;
    hipLaunchKernelGGL(label_border_kernel<false>, dim3(kg_grid_cap(m)), dim3(256), 0, (hipStream_t)stream, a, b, nimg, H, W, jobs, m, mode, counts,
                       0LL);
    KG_CHECK_LAUNCH("label_border_counts");
    return KG_OK;
}

// d2: device int32 [D]
extern "C" int kg_label_border_d2(const int* a, const int* b, int nimg, int H, int W, const int* jobs, int m, int mode, int* d2, int D,
                                  void* stream) {
    KG_CHECK_ARG(D >= 0, "kg_label_border_d2: D %d", D);
    KG_TRY(kg_check_border("kg_label_border_d2", a, b, nimg, H, W, jobs, m, mode, d2, 4L * D, D > 0));
    if (m == 0 || D == 0) return KG_OK;                                // no slot passes the predicate: nothing to store
    hipLaunchKernelGGL(label_border_kernel<true>, dim3(kg_grid_cap(m)), dim3(256), 0, (hipStream_t)stream, a, b, nimg, H, W, jobs, m, mode, d2,
                       (long long)D);
    KG_CHECK_LAUNCH("label_border_d2");
    return KG_OK;
}
