// contours.hip -- the outline of every instance of a label map as polygon rings on gfx950 (contours.py).
//   kg_label_contour_counts  per job {img, id, box}: {rings, vertices, perimeter, status}
//   kg_label_contours        per job {img, id, box, ring_at, vert_at}: the k-th ring of the job into rings[ring_at + k] as
//                            {first, count, perimeter, area2}, its vertices into verts[first .. first + count) as (y, x)
//
// Semantics (include/kgnet_hip.h is the normative text).  P = the pixels of the clamped box with labels == id; vertices are the lattice
// points (Y, X), pixel (y, x) is the square between (y, x) and (y + 1, x + 1).  A directed crack leaves a vertex E (x + 1), S (y + 1),
// W (x - 1) or N (y - 1) with P on its right and non-P on its left:
//     E at (Y, X): m(Y, X) && !m(Y - 1, X)            S: m(Y, X - 1) && !m(Y, X)
//     W at (Y, X): m(Y - 1, X - 1) && !m(Y, X - 1)    N: m(Y - 1, X) && !m(Y - 1, X - 1)
// The successor of a crack that arrives at V in direction d is the first existing crack leaving V among right turn (d + 1) & 3, straight
// d, left turn (d + 3) & 3 (right first: P is 4-connected).  The cracks fall into rings; the vertices of a ring are where the direction
// changes.  A CANDIDATE is an E crack at (Y, X) with no E crack at (Y, X - 1); the start of a ring is its candidate with the smallest
// (Y, X) in raster order, and the rings of a job are ordered by their starts.
//
// One block per job (the grid strides when there are more jobs than KG_LABEL_MAX_BLOCKS), 256 threads:
//   FILL   the (h + 2) x pitch membership bits of the box with a zero halo on each side, read as one flat row-major list (consecutive
//          lanes, consecutive x); a wave's ballot is one aligned 64-bit piece of the bitmap, as label_runs_kernel stores it.  The halo and
//          the padding of a row are 0 by a predicate on the coordinates before an address exists.  The pitch is an odd number of dwords
//          for the reason given at kg_run_tile (runlengths.hip).
//   SCAN   the (h + 1)(w + 1) vertex positions in raster order, 256 per chunk.  A lane whose position is a candidate traces its ring in
//          LDS: it stops as NOT the owner on arriving at a candidate with a smaller (Y, X), as the OWNER on returning to its own, and
//          counts vertices and cracks and sums area2 on the way.  The step count is capped at 4 (h + 1)(w + 1).
//   SLOTS  an exclusive scan of (owner, owner ? count : 0) -- ballot and popcount for the rings, a shuffle scan for the vertices, the wave
//          totals through LDS, a carry across chunks -- gives every owner its ring slot and its vertex offset in start order.  The write
//          kernel's owner traces once more and stores; the count kernel stores the four totals of the job.
//
// The index rule of label_common.h holds here, with ONE new exception: the tracer's position is an LDS bit index that depends on bits
// derived from labels.  It is bounded by construction (a crack touches a P pixel of the box, so its ends lie in [0, h] x [0, w]) and by
// an explicit clamp to that range after every step.  No GLOBAL address depends on a label: the loads depend on the job table (box
// clamped before any address is formed, image index only inside (unsigned)img < (unsigned)nimg), and the stores on the job table plus
// prefix counts, each inside a 64-bit unsigned range predicate (slot < R, first + k < V).  No atomics.
#include "label_common.h"

#define KG_CT_BITS (1 << 18)            // membership bits of one job, halo included: 32 KB of LDS

// pitch in bits of a box of w columns: w + 2 rounded up to an odd number of dwords
__host__ __device__ static inline int kg_ct_pitch(int w) { return (((w + 2 + 31) >> 5) | 1) << 5; }
__host__ __device__ static inline bool kg_ct_fits(int h, int w) { return (long)(h + 2) * kg_ct_pitch(w) <= KG_CT_BITS; }

struct KgCtRing { int count, perimeter; long long area2; bool owner; };

// The ring of the candidate at (Y0, X0), box-local.  bits: the bitmap, m(y, x) at bit (y + 1) * pitch + x + 1.  STORE: the vertices go to
// verts[first + k], each inside (first + k) < V.  Every position is clamped to [0, h] x [0, w], so the four bits around it are rows
// Y, Y + 1 and columns X, X + 1 of the (h + 2) x pitch bitmap.
template <bool STORE>
__device__ __forceinline__ KgCtRing kg_ct_trace(const unsigned* bits, int pitch, int h, int w, int y1, int x1, int Y0, int X0, int cap,
                                                int* __restrict__ verts, unsigned long long first, unsigned long long V) {
    KgCtRing r{1, 0, 0, false};
    int Y = Y0, X = X0, d = 0;
    if constexpr (STORE) {
        if (first < V) { verts[2 * first] = y1 + Y; verts[2 * first + 1] = x1 + X; }
    }
    for (int s = 0; s < cap; ++s) {
        r.area2 += d == 0 ? -(long long)(y1 + Y) : d == 1 ? (long long)(x1 + X) : d == 2 ? (long long)(y1 + Y) : -(long long)(x1 + X);
        Y += (d == 1) - (d == 3); X += (d == 0) - (d == 2);
        Y = Y < 0 ? 0 : Y > h ? h : Y; X = X < 0 ? 0 : X > w ? w : X;  // the explicit clamp of the LDS exception
        ++r.perimeter;
        const int up = Y * pitch + X, dn = up + pitch;                 // m(Y - 1, X - 1) and m(Y, X - 1)
        const bool a = (bits[up >> 5] >> (up & 31)) & 1u, b = (bits[(up + 1) >> 5] >> ((up + 1) & 31)) & 1u;
        const bool c = (bits[dn >> 5] >> (dn & 31)) & 1u, e = (bits[(dn + 1) >> 5] >> ((dn + 1) & 31)) & 1u;
        const unsigned ex = (unsigned)(e && !b) | (unsigned)(c && !e) << 1 | (unsigned)(a && !c) << 2 | (unsigned)(b && !a) << 3;
        const int rt = (d + 1) & 3, lt = (d + 3) & 3;
        int nd;
        if ((ex >> rt) & 1u) nd = rt;
        else if ((ex >> d) & 1u) nd = d;
        else if ((ex >> lt) & 1u) nd = lt;
        else break;                                                    // a bitmap that cannot occur
        if (nd == 0 && !(c && !a)) {                                   // the next crack is a candidate
            if (Y == Y0 && X == X0) { r.owner = true; break; }
            if (Y < Y0 || (Y == Y0 && X < X0)) break;
        }
        if (nd != d) {
            if constexpr (STORE) {
                const unsigned long long at = first + (unsigned long long)r.count;
                if (at < V) { verts[2 * at] = y1 + Y; verts[2 * at + 1] = x1 + X; }
            }
            ++r.count;
        }
        d = nd;
    }
    return r;
}

// part is double-buffered by the parity of the chunk, as in label_runs_kernel: one barrier per chunk, two per job around the fill.
template <bool WRITE>
__global__ __launch_bounds__(256) void label_contours_kernel(const int* __restrict__ labels, int nimg, int H, int W, const int* __restrict__ jobs,
                                                             int m, long long* __restrict__ out, long long R, int* __restrict__ verts,
                                                             long long V) {
    __shared__ unsigned bits[KG_CT_BITS / 32];
    __shared__ int part[2][4][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned walk = 0;
    for (long j = blockIdx.x; j < m; j += gridDim.x) {
        const int* jb = jobs + j * (WRITE ? 8 : 6);
        const int img = jb[0], id = jb[1];
        KgBox box = kg_job_box(jb + 2, H, W);
        if (!((unsigned)img < (unsigned)nimg)) box.h = box.w = 0;      // the only use of img before it scales an address
        const long base = (long)img * H * W;                           // used only with a non-empty box: img < nimg
        long long ring_at = 0, vert_at = 0;
        if constexpr (WRITE) { ring_at = jb[6]; vert_at = jb[7]; }
        const bool live = box.h > 0 && box.w > 0, fits = live && kg_ct_fits(box.h, box.w);
        int rings = 0, nverts = 0, perim = 0;                          // the carries: the same in every thread
        if (fits) {
            const int h = box.h, w = box.w, pitch = kg_ct_pitch(w), total = (h + 2) * pitch;   // <= KG_CT_BITS, a multiple of 32
            __syncthreads();                                           // the bits of the job before have been read
            {
                const int sr = 256 / pitch, sc = 256 - sr * pitch;
                int rr = (int)threadIdx.x / pitch, c = (int)threadIdx.x - rr * pitch;
                for (int e0 = 0; e0 < total; e0 += 256) {
                    bool in = false;
                    if (rr >= 1 && rr <= h && c >= 1 && c <= w)        // inside the box, hence inside the map
                        in = labels[base + (long)(box.y1 + rr - 1) * W + (box.x1 + c - 1)] == id;
                    const unsigned long long b = __ballot(in);
                    const int word = (e0 + (wave << 6)) >> 5;          // e0 + 64 wave + 63 < total rounded up to 256 <= KG_CT_BITS
                    if (lane == 0) bits[word] = (unsigned)b;
                    if (lane == 32) bits[word + 1] = (unsigned)(b >> 32);
                    c += sc; rr += sr;
                    if (c >= pitch) { c -= pitch; ++rr; }
                }
            }
            __syncthreads();
            const int nv = (h + 1) * (w + 1), cap = 4 * nv;            // nv < 2^18
            for (int q0 = 0; q0 < nv; q0 += 256) {
                const int q = q0 + (int)threadIdx.x;
                int Y = 0, X = 0;
                bool cand = false;
                if (q < nv) {
                    Y = q / (w + 1); X = q - Y * (w + 1);
                    const int up = Y * pitch + X, dn = up + pitch;
                    const bool a = (bits[up >> 5] >> (up & 31)) & 1u, b = (bits[(up + 1) >> 5] >> ((up + 1) & 31)) & 1u;
                    const bool c = (bits[dn >> 5] >> (dn & 31)) & 1u, e = (bits[(dn + 1) >> 5] >> ((dn + 1) & 31)) & 1u;
                    cand = (e && !b) && !(c && !a);
                }
                KgCtRing r{0, 0, 0, false};
                if (cand) r = kg_ct_trace<false>(bits, pitch, h, w, box.y1, box.x1, Y, X, cap, nullptr, 0ull, 0ull);
                const int mine = r.owner ? r.count : 0;
                const unsigned long long bo = __ballot(r.owner);
                int kr = __popcll(bo & below);
                int inc = mine;                                        // inclusive shuffle scan of the vertex counts of the wave
                for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o); if (lane >= o) inc += t; }
                int kv = inc - mine;
                const int wp = kg_wave_sum(r.owner ? r.perimeter : 0);
                int (*p)[3] = part[walk++ & 1];
                if (lane == 63) { p[wave][0] = __popcll(bo); p[wave][1] = inc; p[wave][2] = wp; }
                __syncthreads();
                int tr = 0, tv = 0, tp = 0;
                for (int k = 0; k < 4; ++k) {
                    if (k < wave) { kr += p[k][0]; kv += p[k][1]; }
                    tr += p[k][0]; tv += p[k][1]; tp += p[k][2];
                }
                if constexpr (WRITE) {
                    if (r.owner) {
                        const long long first = vert_at + nverts + kv;
                        const unsigned long long slot = (unsigned long long)(ring_at + rings + kr);
                        if (slot < (unsigned long long)R) {
                            out[4 * slot] = first; out[4 * slot + 1] = r.count; out[4 * slot + 2] = r.perimeter; out[4 * slot + 3] = r.area2;
                        }
                        kg_ct_trace<true>(bits, pitch, h, w, box.y1, box.x1, Y, X, cap, verts, (unsigned long long)first, (unsigned long long)V);
                    }
                }
                rings += tr; nverts += tv; perim += tp;
            }
        }
        if constexpr (!WRITE) {
            if (threadIdx.x == 0) { out[4 * j] = rings; out[4 * j + 1] = nverts; out[4 * j + 2] = perim; out[4 * j + 3] = live && !fits; }
        }
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// labels: device int32 [nimg][H][W]; jobs: device int32 [m][6] = (img, id, y1, x1, y2, x2), written by the caller;
// out: device int64 [m][4] = {rings, vertices, perimeter, status}
extern "C" int kg_label_contour_counts(const int* labels, int nimg, int H, int W, const int* jobs, int m, long long* out, void* stream) {
    KG_TRY(kg_check_job_stack("kg_label_contour_counts", labels, nimg, H, W, jobs, m));
    KG_CHECK_ARG(out || m == 0, "kg_label_contour_counts: null pointer (out)");
    KG_CHECK_ARG(kg_aligned(out, 7), "kg_label_contour_counts: misaligned pointer");
    KG_CHECK_ARG(!out || kg_apart(out, 32L * m, labels, 4L * nimg * H * W), "kg_label_contour_counts: out aliases labels");
    if (m == 0) return KG_OK;
    hipLaunchKernelGGL(label_contours_kernel<false>, dim3(kg_grid_cap(m)), dim3(256), 0, (hipStream_t)stream, labels, nimg, H, W, jobs, m, out,
                       0LL, (int*)nullptr, 0LL);
    KG_CHECK_LAUNCH("label_contour_counts");
    return KG_OK;
}

// jobs: device int32 [m][8] = (img, id, y1, x1, y2, x2, ring_at, vert_at); rings: device int64 [R][4] = {first, count, perimeter, area2};
// verts: device int32 [V][2] = (y, x)
extern "C" int kg_label_contours(const int* labels, int nimg, int H, int W, const int* jobs, int m, long long* rings, int R, int* verts, int V,
                                 void* stream) {
    const char* fn = "kg_label_contours";
    KG_TRY(kg_check_job_stack(fn, labels, nimg, H, W, jobs, m));
    KG_CHECK_ARG(R >= 0 && V >= 0, "%s: R %d, V %d", fn, R, V);
    KG_CHECK_ARG(rings || R == 0, "%s: null pointer (rings)", fn);
    KG_CHECK_ARG(verts || V == 0, "%s: null pointer (verts)", fn);
    KG_CHECK_ARG(kg_aligned(rings, 7) && kg_aligned(verts, 3), "%s: misaligned pointer", fn);
    const long lbytes = 4L * nimg * H * W;
    KG_CHECK_ARG(!rings || kg_apart(rings, 32L * R, labels, lbytes), "%s: rings aliases labels", fn);
    KG_CHECK_ARG(!verts || kg_apart(verts, 8L * V, labels, lbytes), "%s: verts aliases labels", fn);
    KG_CHECK_ARG(!rings || !verts || kg_apart(rings, 32L * R, verts, 8L * V), "%s: rings aliases verts", fn);
    if (m == 0 || (R == 0 && V == 0)) return KG_OK;                    // no slot passes a predicate: nothing to store
    hipLaunchKernelGGL(label_contours_kernel<true>, dim3(kg_grid_cap(m)), dim3(256), 0, (hipStream_t)stream, labels, nimg, H, W, jobs, m, rings,
                       (long long)R, verts, (long long)V);
    KG_CHECK_LAUNCH("label_contours");
    return KG_OK;
}
