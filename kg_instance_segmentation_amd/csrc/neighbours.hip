// neighbours.hip -- the touching-neighbour graph of instance label maps on gfx950 (neighbours.py): which other values the pixels of an
// instance touch, and along how many pixel sides and corners.
//   kg_label_neighbours  per job {img, id, box, resume, after}: the non-zero values != id that sit next to a pixel of the box with
//                        labels == id, in ascending signed order, each with its side and corner count, `slots` of them per row
//
// The index rule of label_common.h holds here.  The job table is the one device-read table: its box is clamped to the map before any
// address is formed, its image index is used only inside the predicate (unsigned)img < (unsigned)nimg (a job that fails it writes a row of
// zeros and reads nothing else), and resume / after are compared with label values, nothing else.  A neighbour outside the map is decided
// by a predicate on its coordinates before its address exists.  Label values are compared and stored only: there is no table a value
// could index, hence no hash and no atomics, and the row is the same from run to run.
#include "label_common.h"

#define KG_NB_MAX_SLOTS 64
#define KG_NB_NONE LLONG_MAX            // "no value": every key is an int32 widened to 64 bits, so INT_MIN and INT_MAX need no sentinel

__device__ __forceinline__ long long kg_nb_wave_min(long long v) {
    for (int o = 32; o; o >>= 1) { const long long t = __shfl_xor(v, o); v = t < v ? t : v; }
    return v;
}

// One block per job (the grid strides when there are more jobs than KG_LABEL_MAX_BLOCKS).  The values are EXTRACTED IN ORDER: the block
// holds a uniform threshold thr (below every int32 at first, `after` when the job resumes) and walks the box; a walk takes the block
// minimum N of the qualifying neighbour values above thr and, once a current value exists, counts the sides and corners of that value
// (== thr) on the same pass.  Then the current value is written to its slot and N becomes the current value.  k distinct values cost
// min(k, slots) + 1 walks; the map stays in L2 between them (a nucleus box is a few hundred pixels).
//
// 32-bit partials, with their bound: a box holds at most 2^30 pixels, so a thread visits at most 2^22 of them and a wave 2^28; sides and
// corners add at most 4 per visited pixel each, so a thread's count stays below 2^24 and a wave's sum at or below 2^30.
//
// part is double-buffered by the parity of the walk: a thread that writes part[q] for walk k + 2 has passed the barrier of walk k + 1,
// which every thread reaches only after it has read part[q] of walk k.  One barrier per walk.
template <bool DIAG>
__global__ __launch_bounds__(256) void label_neighbours_kernel(const int* __restrict__ labels, int nimg, int H, int W, const int* __restrict__ jobs,
                                                               int m, int slots, long long* __restrict__ out) {
    __shared__ long long part[2][4][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ncol = 2 + 3 * slots;
    unsigned walk = 0;
    for (long j = blockIdx.x; j < m; j += gridDim.x) {
        const int* jb = jobs + j * 8;
        const int img = jb[0], id = jb[1];
        KgBox box = kg_job_box(jb + 2, H, W);
        if (!((unsigned)img < (unsigned)nimg)) box.h = box.w = 0;      // the only use of img before it scales an address
        const long base = (long)img * H * W;                           // used only with a non-empty box: img < nimg
        long long thr = jb[6] != 0 ? (long long)jb[7] : (long long)INT_MIN - 1;
        bool counting = false;                                         // thr is a value of the map whose sides and corners are wanted
        int count = 0, more = 0;
        long long* row = out + j * ncol;
        for (int w = 0; w <= slots; ++w) {                             // (it leaves through a break: at w == slots, count == slots)
            const int cur = (int)thr;
            long long nxt = KG_NB_NONE;
            int sides = 0, corners = 0;
            auto see = [&](int v, int& tally) {
                if (v != id && v != 0) {
                    tally += counting && v == cur;
                    if ((long long)v > thr && (long long)v < nxt) nxt = v;
                }
            };
            kg_box_walk(box, [&](int Y, int X) {
                const long p = base + (long)Y * W + X;
                if (labels[p] == id) {
                    // the coordinate decides "outside the map" before the neighbour's address exists
                    const bool up = Y > 0, dn = Y < H - 1, lf = X > 0, rt = X < W - 1;
                    if (up) see(labels[p - W], sides);
                    if (dn) see(labels[p + W], sides);
                    if (lf) see(labels[p - 1], sides);
                    if (rt) see(labels[p + 1], sides);
                    if constexpr (DIAG) {
                        if (up && lf) see(labels[p - W - 1], corners);
                        if (up && rt) see(labels[p - W + 1], corners);
                        if (dn && lf) see(labels[p + W - 1], corners);
                        if (dn && rt) see(labels[p + W + 1], corners);
                    }
                }
            });
            nxt = kg_nb_wave_min(nxt); sides = kg_wave_sum(sides); corners = kg_wave_sum(corners);
            long long (*q)[3] = part[walk++ & 1];
            if (lane == 0) { q[wave][0] = nxt; q[wave][1] = sides; q[wave][2] = corners; }
            __syncthreads();
            long long N = q[0][0], S = q[0][1], C = q[0][2];           // every thread forms the same three numbers: the loop stays uniform
            for (int k = 1; k < 4; ++k) { N = q[k][0] < N ? q[k][0] : N; S += q[k][1]; C += q[k][2]; }
            if (counting) {
                if (threadIdx.x == 0) { row[2 + 3 * count] = cur; row[3 + 3 * count] = S; row[4 + 3 * count] = C; }
                ++count;
            }
            if (N == KG_NB_NONE) break;
            if (count == slots) { more = 1; break; }
            thr = N; counting = true;
        }
        if (threadIdx.x == 0) { row[0] = count; row[1] = more; }
        for (int c = 2 + 3 * count + (int)threadIdx.x; c < ncol; c += 256) row[c] = 0;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// labels: device int32 [nimg][H][W]; jobs: device int32 [m][8] = (img, id, y1, x1, y2, x2, resume, after), written by the caller;
// out: device int64 [m][2 + 3 * slots] = {count, more, (value, sides, corners) x slots}
extern "C" int kg_label_neighbours(const int* labels, int nimg, int H, int W, int connectivity, const int* jobs, int m, int slots, long long* out,
                                   void* stream) {
    // H, W <= KG_LABEL_MAX_SIDE: a box holds <= 2^30 pixels, so a count of sides <= 2^32 fits int64
    KG_TRY(kg_check_job_stack("kg_label_neighbours", labels, nimg, H, W, jobs, m));
    KG_CHECK_ARG(connectivity == 4 || connectivity == 8, "kg_label_neighbours: connectivity %d (4 or 8)", connectivity);
    KG_CHECK_ARG(slots >= 1 && slots <= KG_NB_MAX_SLOTS, "kg_label_neighbours: slots %d (1 .. %d)", slots, KG_NB_MAX_SLOTS);
    KG_CHECK_ARG(out || m == 0, "kg_label_neighbours: null pointer (out)");
    KG_CHECK_ARG(kg_aligned(out, 7), "kg_label_neighbours: misaligned pointer");
    if (m == 0) return KG_OK;
    hipStream_t s = (hipStream_t)stream;
    if (connectivity == 8)
        hipLaunchKernelGGL(label_neighbours_kernel<true>, dim3(kg_grid_cap(m)), dim3(256), 0, s, labels, nimg, H, W, jobs, m, slots, out);
    else
        hipLaunchKernelGGL(label_neighbours_kernel<false>, dim3(kg_grid_cap(m)), dim3(256), 0, s, labels, nimg, H, W, jobs, m, slots, out);
    KG_CHECK_LAUNCH("label_neighbours");
    return KG_OK;
}
