// runlengths.hip -- run-length lists of instance label maps on gfx950 (runlengths.py): the Kaggle rows and COCO counts of every
// instance, and the way back from run-length rows to a label map.
//   kg_label_run_counts  per job {img, id, box}: the number of run heads and of run tails among the box's pixels with labels == id
//   kg_label_runs        per job {img, id, box, head_at, tail_at}: the position of the k-th head into out[head_at + k][0], of the k-th
//                        tail into out[tail_at + k][1]
//   kg_runs_paint        sorted, disjoint rows {first, last, value} -> a label map
//
// Pixel order: p = x * H + y, down the columns first, 0-based.  A pixel of the box with labels == id is a HEAD when p == 0 or the map's
// pixel at p - 1 does not hold id, a TAIL when p == H * W - 1 or the pixel at p + 1 does not; p - 1 is (y - 1, x), or (H - 1, x - 1) when
// y == 0, and p + 1 mirrors that, so a run continues from the bottom of one column into the top of the next.
//
// The index rule of label_common.h holds here.  The job table is the one device-read table: its box is clamped to the map before any
// address is formed and its image index is used only inside (unsigned)img < (unsigned)nimg.  The pixels at p - 1 and p + 1 are read from
// the MAP, never from the box, and a position outside the map is decided by a predicate on its coordinates before its address exists.
// Label values are compared only.  The one NEW exception is the store of kg_label_runs: its slot is head_at + k (tail_at + k), where k is
// a prefix count of predicates, not a label value, and the store happens only inside the 64-bit unsigned predicate slot < R -- a negative
// or oversized offset from a wrong table cannot leave the buffer.  kg_runs_paint indexes its rows by a binary-search position in [0, R).
// No atomics anywhere.
#include "label_common.h"

#define KG_RL_BITS (1 << 17)            // membership bits of one tile of a box: 16 KB of LDS

// A box of h rows is walked in tiles of cw columns; a tile keeps one membership bit per pixel of its h rows plus the row of the pixels
// at p - 1 of its top row and the row of the pixels at p + 1 of its bottom row: (h + 2) rows of `pitch` bits, flat.  h <= 32768 leaves
// at least 3 bits per row.  The scan reads the bits down the columns: consecutive lanes are `pitch` bits apart, so a pitch above one
// dword is an ODD number of dwords -- the 32 lanes of a ds_read_b32 group then fall on 32 different banks -- and a pitch of at most one
// dword puts neighbouring lanes into the same or the next dword (a broadcast).  A band of 65536 pixels (runlengths.py) is one tile.
struct KgRunTile { int cw, pitch; };
__device__ __forceinline__ KgRunTile kg_run_tile(int h, int w) {
    const int budget = KG_RL_BITS / (h + 2);
    KgRunTile t;
    if (budget >= 96) {
        const int pmax = (((budget - 32) >> 6) << 6) + 32;           // the largest odd number of dwords that fits
        t.cw = w < pmax ? w : pmax;
        t.pitch = t.cw <= 32 ? t.cw : ((((t.cw + 31) >> 5) | 1) << 5);
    } else {
        const int cap = budget < 32 ? budget : 32;
        t.cw = w < cap ? w : cap;
        t.pitch = t.cw;
    }
    return t;
}

// One block per job (the grid strides when there are more jobs than KG_LABEL_MAX_BLOCKS).  Per tile: FILL -- the 256 threads read the
// (h + 2) x pitch elements as one flat row-major list (consecutive lanes, consecutive x, as kg_box_walk does), a wave's ballot is one
// aligned 64-bit piece of the bitmap, no atomics; SCAN -- the tile's pixels in column-major order, 256 positions per chunk: the ballots of
// heads and tails, the popcount below the lane, the wave totals through LDS and a carry that runs across chunks, tiles and (in
// runlengths.py) bands.  The count and the write kernel are this one walk.
//
// part is double-buffered by the parity of the chunk: a thread that writes part[q] for chunk k + 2 has passed the barrier of chunk
// k + 1, which every thread reaches only after it has read part[q] of chunk k.  One barrier per chunk, two per tile around the fill.
template <bool WRITE>
__global__ __launch_bounds__(256) void label_runs_kernel(const int* __restrict__ labels, int nimg, int H, int W, const int* __restrict__ jobs,
                                                         int m, int* __restrict__ out, long long R) {
    __shared__ unsigned bits[KG_RL_BITS / 32];
    __shared__ int part[2][4][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned walk = 0;
    for (long j = blockIdx.x; j < m; j += gridDim.x) {
        const int* jb = jobs + j * (WRITE ? 8 : 6);
        const int img = jb[0], id = jb[1];
        KgBox box = kg_job_box(jb + 2, H, W);
        if (!((unsigned)img < (unsigned)nimg)) box.h = box.w = 0;      // the only use of img before it scales an address
        const long base = (long)img * H * W;                           // used only with a non-empty box: img < nimg
        long long head_at = 0, tail_at = 0;
        if constexpr (WRITE) { head_at = jb[6]; tail_at = jb[7]; }
        int heads = 0, tails = 0;                                      // the carries: the same in every thread
        if (box.h > 0 && box.w > 0) {
            const KgRunTile tile = kg_run_tile(box.h, box.w);
            const int pitch = tile.pitch, total = (box.h + 2) * pitch; // <= KG_RL_BITS
            for (int c0 = 0; c0 < box.w; c0 += tile.cw) {
                const int cwt = box.w - c0 < tile.cw ? box.w - c0 : tile.cw;
                __syncthreads();                                       // the bits of the tile (or job) before have been read
                {
                    const int sr = 256 / pitch, sc = 256 - sr * pitch;
                    int rr = (int)threadIdx.x / pitch, c = (int)threadIdx.x - rr * pitch;
                    for (int e0 = 0; e0 < total; e0 += 256) {
                        bool in = false;
                        if (rr < box.h + 2 && c < cwt) {
                            // tile row rr is map row y1 + rr - 1; above row 0 lies the bottom of the column before, below row H - 1 the
                            // top of the column after: the coordinates decide "outside the map" before the address exists
                            int Y = box.y1 + rr - 1, X = box.x1 + c0 + c;
                            if (Y < 0) { Y = H - 1; --X; }
                            else if (Y >= H) { Y = 0; ++X; }
                            if (X >= 0 && X < W) in = labels[base + (long)Y * W + X] == id;
                        }
                        const unsigned long long b = __ballot(in);
                        const int word = (e0 + (wave << 6)) >> 5;      // e0 + 64 wave + 63 < total rounded up to 256 <= KG_RL_BITS
                        if (lane == 0) bits[word] = (unsigned)b;
                        if (lane == 32) bits[word + 1] = (unsigned)(b >> 32);
                        c += sc; rr += sr;
                        if (c >= pitch) { c -= pitch; ++rr; }
                    }
                }
                __syncthreads();
                const int n = box.h * cwt;
                const int sc = 256 / box.h, sr = 256 - sc * box.h;
                int c = (int)threadIdx.x / box.h, r = (int)threadIdx.x - c * box.h;
                for (int q0 = 0; q0 < n; q0 += 256) {
                    bool hd = false, tl = false;
                    if (c < cwt) {
                        const int at = r * pitch + c;                  // the pixel is tile row r + 1: at + 2 pitch < total
                        const bool prev = (bits[at >> 5] >> (at & 31)) & 1u;
                        const bool me = (bits[(at + pitch) >> 5] >> ((at + pitch) & 31)) & 1u;
                        const bool next = (bits[(at + 2 * pitch) >> 5] >> ((at + 2 * pitch) & 31)) & 1u;
                        hd = me && !prev; tl = me && !next;
                    }
                    const unsigned long long bh = __ballot(hd), bt = __ballot(tl);
                    int kh = __popcll(bh & below), kt = __popcll(bt & below);
                    int (*q)[2] = part[walk++ & 1];
                    if (lane == 0) { q[wave][0] = __popcll(bh); q[wave][1] = __popcll(bt); }
                    __syncthreads();
                    int th = 0, tt = 0;
                    for (int k = 0; k < 4; ++k) {
                        if (k < wave) { kh += q[k][0]; kt += q[k][1]; }
                        th += q[k][0]; tt += q[k][1];
                    }
                    if constexpr (WRITE) {
                        if (hd || tl) {
                            const int p = (box.x1 + c0 + c) * H + box.y1 + r;
                            const unsigned long long sh = (unsigned long long)(head_at + heads + kh);
                            const unsigned long long st = (unsigned long long)(tail_at + tails + kt);
                            if (hd && sh < (unsigned long long)R) out[2 * sh] = p;
                            if (tl && st < (unsigned long long)R) out[2 * st + 1] = p;
                        }
                    }
                    heads += th; tails += tt;
                    r += sr; c += sc;
                    if (r >= box.h) { r -= box.h; ++c; }
                }
            }
        }
        if constexpr (!WRITE) {
            if (threadIdx.x == 0) { out[2 * j] = heads; out[2 * j + 1] = tails; }
        }
    }
}

// One lane per output pixel in row-major order (coalesced stores).  pos = the number of rows with first <= p, found by a binary search
// whose steps are the powers of two from `top` (the largest one <= R, a kernel argument) down: a row is read only inside pos + s <= R,
// so the index is a search position in [0, R), and with R == 0 (top == 0) nothing is read.
__global__ __launch_bounds__(256) void runs_paint_kernel(const int* __restrict__ runs, long R, long top, int H, int W, int background,
                                                         int* __restrict__ out) {
    const long n = (long)H * W;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < n; e += gridDim.x * 256L) {
        const int y = (int)(e / W), x = (int)(e - (long)y * W);
        const int p = x * H + y;
        long pos = 0;
        for (long s = top; s; s >>= 1)
            if (pos + s <= R && runs[3 * (pos + s - 1)] <= p) pos += s;
        int v = background;
        if (pos > 0 && p <= runs[3 * (pos - 1) + 1]) v = runs[3 * (pos - 1) + 2];
        out[e] = v;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// (H, W <= KG_LABEL_MAX_SIDE: a box holds <= 2^30 pixels, hence <= 2^30 runs)
// labels: device int32 [nimg][H][W]; jobs: device int32 [m][6] = (img, id, y1, x1, y2, x2), written by the caller;
// out: device int32 [m][2] = {heads, tails}
extern "C" int kg_label_run_counts(const int* labels, int nimg, int H, int W, const int* jobs, int m, int* out, void* stream) {
    KG_TRY(kg_check_job_stack("kg_label_run_counts", labels, nimg, H, W, jobs, m));
    KG_CHECK_ARG(out || m == 0, "kg_label_run_counts: null pointer (out)");
    KG_CHECK_ARG(kg_aligned(out, 3), "kg_label_run_counts: misaligned pointer");
    KG_CHECK_ARG(!out || kg_apart(out, 8L * m, labels, 4L * nimg * H * W), "kg_label_run_counts: out aliases labels");
    if (m == 0) return KG_OK;
    hipLaunchKernelGGL(label_runs_kernel<false>, dim3(kg_grid_cap(m)), dim3(256), 0, (hipStream_t)stream, labels, nimg, H, W, jobs, m, out, 0LL);
    KG_CHECK_LAUNCH("label_run_counts");
    return KG_OK;
}

// jobs: device int32 [m][8] = (img, id, y1, x1, y2, x2, head_at, tail_at); out: device int32 [R][2] = {first, last}
extern "C" int kg_label_runs(const int* labels, int nimg, int H, int W, const int* jobs, int m, int* out, int R, void* stream) {
    KG_TRY(kg_check_job_stack("kg_label_runs", labels, nimg, H, W, jobs, m));
    KG_CHECK_ARG(R >= 0, "kg_label_runs: R %d", R);
    KG_CHECK_ARG(out || R == 0, "kg_label_runs: null pointer (out)");
    KG_CHECK_ARG(kg_aligned(out, 3), "kg_label_runs: misaligned pointer");
    KG_CHECK_ARG(!out || kg_apart(out, 8L * R, labels, 4L * nimg * H * W), "kg_label_runs: out aliases labels");
    if (m == 0 || R == 0) return KG_OK;                                // no slot passes the predicate: nothing to store
    hipLaunchKernelGGL(label_runs_kernel<true>, dim3(kg_grid_cap(m)), dim3(256), 0, (hipStream_t)stream, labels, nimg, H, W, jobs, m, out,
                       (long long)R);
    KG_CHECK_LAUNCH("label_runs");
    return KG_OK;
}

// runs: device int32 [R][3] = {first, last, value}, sorted by first and disjoint (the caller's promise); out: device int32 [H][W]
extern "C" int kg_runs_paint(const int* runs, int R, int H, int W, int background, int* out, void* stream) {
    KG_CHECK_ARG(H > 0 && W > 0 && R >= 0, "kg_runs_paint: bad size (R %d, H %d, W %d)", R, H, W);
    KG_CHECK_ARG(H <= KG_LABEL_MAX_SIDE && W <= KG_LABEL_MAX_SIDE, "kg_runs_paint: H %d, W %d exceed %d", H, W, KG_LABEL_MAX_SIDE);
    KG_TRY(kg_check_map_size("kg_runs_paint", H, W));
    KG_CHECK_ARG(out, "kg_runs_paint: null pointer (out)");
    KG_CHECK_ARG(runs || R == 0, "kg_runs_paint: null pointer (runs)");
    KG_CHECK_ARG(kg_aligned(runs, 3) && kg_aligned(out, 3), "kg_runs_paint: misaligned pointer");
    KG_CHECK_ARG(!runs || kg_apart(out, 4L * H * W, runs, 12L * R), "kg_runs_paint: out aliases runs");
    long top = 0;
    if (R > 0) for (top = 1; top * 2 <= (long)R; top *= 2) {}
    hipLaunchKernelGGL(runs_paint_kernel, dim3(kg_grid_cap(((long)H * W + 255) / 256)), dim3(256), 0, (hipStream_t)stream, runs, (long)R, top, H, W,
                       background, out);
    KG_CHECK_LAUNCH("runs_paint");
    return KG_OK;
}
