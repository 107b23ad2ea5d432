// labelmetrics.hip -- the contingency of two instance label maps on gfx950 (labelmetrics.py): what every label-map metric is a function of.
//   kg_label_stats       label map [H][W] with ids 1 .. n -> per id {area, y1, x1, y2, x2} and the number of pixels outside [0, n]
//   kg_label_inter_jobs  per job {id_a, id_b, box}: the pixels of the box with a == id_a && b == id_b
//
// The index rule of label_common.h holds here.  kg_label_stats forms an address from a value read from device memory: the row of `stats`
// a pixel's label selects.  The rule that bounds it: the index v - 1 is formed only inside the predicate (unsigned)(v - 1) < (unsigned)n,
// evaluated in unsigned arithmetic so that no label (INT_MIN included) wraps into range; a pixel that fails it (and is not 0) adds one
// to `invalid` and touches nothing else.  kg_label_inter_jobs uses labels as predicates only; the one table it reads is the jobs
// (kg_job_box).
#include "label_common.h"

// ---- stats ----------------------------------------------------------------------------------------------------------------------------
// stats[i] = {0, INT_MAX, INT_MAX, 0, 0}: the neutral element of (add, min, min, max, max); invalid[0] = 0
__global__ __launch_bounds__(256) void label_stats_init_kernel(int* __restrict__ stats, int n, int* __restrict__ invalid) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) invalid[0] = 0;
    if (i < (long)n * 5) {
        const int c = (int)(i % 5);
        stats[i] = (c == 1 || c == 2) ? INT_MAX : 0;
    }
}

// One wave per 64-pixel segment of one row, four segments per block, the grid striding over the H * ceil(W / 64) segments; the runs of
// a segment come from kg_seg_run.  Only run heads with a valid id issue atomics, five per run: integer add / min / max, so the result
// does not depend on arrival order.  Invalid pixels are counted per wave by a ballot and added once per wave.
__global__ __launch_bounds__(256) void label_stats_kernel(const int* __restrict__ labels, int H, int W, int n, int* __restrict__ stats,
                                                          int* __restrict__ invalid) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long spr = (W + 63) >> 6, nseg = (long)H * spr;
    int bad = 0;                                                      // wave-uniform
    for (long s = (long)blockIdx.x * 4 + wave; s < nseg; s += (long)gridDim.x * 4) {
        const KgSegRun r = kg_seg_run(s, spr, W, labels);
        const bool valid = r.live && (unsigned)r.v - 1u < (unsigned)n;    // 1 <= v <= n: the only place v - 1 may become an index
        bad += __popcll(__ballot(r.live && r.v != 0 && !valid));
        if (r.head && valid) {
            const int len = r.end - lane;
            int* st = stats + (long)((unsigned)r.v - 1u) * 5;
            atomicAdd(st + 0, len);
            atomicMin(st + 1, r.y);
            atomicMin(st + 2, r.x);
            atomicMax(st + 3, r.y + 1);
            atomicMax(st + 4, r.x + len);
        }
    }
    if (lane == 0 && bad) atomicAdd(invalid, bad);
}

// an id with no pixel: its box becomes zeros
__global__ __launch_bounds__(256) void label_stats_finish_kernel(int* __restrict__ stats, int n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n && stats[i * 5] == 0) { stats[i * 5 + 1] = 0; stats[i * 5 + 2] = 0; }
}

// ---- intersections --------------------------------------------------------------------------------------------------------------------
// count[j] = the pixels of the box of job j with a == id_a && b == id_b.  One block per job (the grid strides when there are more jobs
// than KG_LABEL_MAX_BLOCKS), walking its clamped box (kg_box_walk); an empty or inverted box gives 0.  Reduced by shuffles and 32 bytes
// of LDS, no atomics.
__global__ __launch_bounds__(256) void label_inter_jobs_kernel(const int* __restrict__ a, const int* __restrict__ b, int H, int W,
                                                               const int* __restrict__ jobs, int m, long long* __restrict__ count) {
    __shared__ long long part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long j = blockIdx.x; j < m; j += gridDim.x) {
        const int* jb = jobs + j * 6;
        const int ia = jb[0], ib = jb[1];
        long long c = 0;
        kg_box_walk(kg_job_box(jb + 2, H, W), [&](int Y, int X) {
            const long p = (long)Y * W + X;
            c += (a[p] == ia) & (b[p] == ib);
        });
        c = kg_wave_sum(c);
        if (lane == 0) part[wave] = c;
        __syncthreads();
        if (threadIdx.x == 0) count[j] = part[0] + part[1] + part[2] + part[3];
        __syncthreads();                                              // part is written again by the block's next job
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// labels: device int32 [H][W]; stats: device int32 [n][5] (may be NULL when n == 0); invalid: device int32 [1]
extern "C" int kg_label_stats(const int* labels, int H, int W, int n, int* stats, int* invalid, void* stream) {
    KG_CHECK_ARG(H > 0 && W > 0 && n >= 0, "kg_label_stats: bad size (H %d, W %d, n %d)", H, W, n);
    KG_TRY(kg_check_map_size("kg_label_stats", H, W));
    KG_CHECK_ARG((long)n * 5 <= 0x7fffffffL, "kg_label_stats: n %d too large", n);
    KG_CHECK_ARG(labels && invalid, "kg_label_stats: null pointer (labels / invalid)");
    KG_CHECK_ARG(stats || n == 0, "kg_label_stats: null pointer (stats)");
    KG_CHECK_ARG(kg_aligned(labels, 3) && kg_aligned(stats, 3) && kg_aligned(invalid, 3), "kg_label_stats: misaligned pointer");
    const long nseg = (long)H * ((W + 63) / 64), cells = (long)n * 5, nb = (nseg + 3) / 4;
    hipLaunchKernelGGL(label_stats_init_kernel, dim3((unsigned)(cells ? kg_cdiv(cells, 256) : 1)), dim3(256), 0, (hipStream_t)stream, stats, n, invalid);
    KG_CHECK_LAUNCH("label_stats_init");
    hipLaunchKernelGGL(label_stats_kernel, dim3(kg_grid_cap(nb)), dim3(256), 0, (hipStream_t)stream, labels, H, W, n, stats, invalid);
    KG_CHECK_LAUNCH("label_stats");
    hipLaunchKernelGGL(label_stats_finish_kernel, dim3((unsigned)(n ? kg_cdiv(n, 256) : 1)), dim3(256), 0, (hipStream_t)stream, stats, n);
    KG_CHECK_LAUNCH("label_stats_finish");
    return KG_OK;
}

// a, b: device int32 [H][W]; jobs: device int32 [m][6] = (id_a, id_b, y1, x1, y2, x2), written by the caller; count: device int64 [m]
extern "C" int kg_label_inter_jobs(const int* a, const int* b, int H, int W, const int* jobs, int m, long long* count, void* stream) {
    KG_CHECK_ARG(H > 0 && W > 0 && m >= 0, "kg_label_inter_jobs: bad size (H %d, W %d, m %d)", H, W, m);
    KG_TRY(kg_check_map_size("kg_label_inter_jobs", H, W));
    KG_CHECK_ARG(a && b, "kg_label_inter_jobs: null pointer (a / b)");
    KG_CHECK_ARG((jobs && count) || m == 0, "kg_label_inter_jobs: null pointer (jobs / count)");
    KG_CHECK_ARG(kg_aligned(a, 3) && kg_aligned(b, 3) && kg_aligned(jobs, 3) && kg_aligned(count, 7), "kg_label_inter_jobs: misaligned pointer");
    if (m == 0) return KG_OK;
    hipLaunchKernelGGL(label_inter_jobs_kernel, dim3(kg_grid_cap(m)), dim3(256), 0, (hipStream_t)stream, a, b, H, W, jobs, m, count);
    KG_CHECK_LAUNCH("label_inter_jobs");
    return KG_OK;
}
