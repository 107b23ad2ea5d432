// measure.hip -- per-instance measurements of instance label maps on gfx950 (measure.py): the exact integers every shape, contact and
// intensity measurement of an instance is a function of.
//   kg_label_measure  per job {img, id, box}: over the pixels of the box with labels == id, the count, the first and second coordinate
//                     sums, the 4-neighbour edge counts (all, frame, contact, boundary pixels) and per image channel sum, sum of squares,
//                     min and max
//
// The index rule of label_common.h holds here.  The job table is the one device-read table: its box is clamped to the map before any
// address is formed, and its image index is used only inside the predicate (unsigned)img < (unsigned)nimg (a job that fails it writes a
// row of zeros and reads nothing else).  A neighbour outside the map is decided by a predicate on its coordinates before its address
// exists.  No atomics.
#include "label_common.h"

#define KG_MS_GEOM 10                   // geometry columns; 4 more per channel
#define KG_MS_MAX_COLS (KG_MS_GEOM + 4 * 4)

// One block per job (the grid strides when there are more jobs than KG_LABEL_MAX_BLOCKS), walking its clamped box.  A lane whose pixel
// holds the id reads its four neighbours FROM THE MAP (a box or band edge inside the map is not an object edge), each under a
// coordinate predicate, and the pixel's C channel values.  Partials are reduced by shuffles and 4 * (10 + 4 C) * 8 bytes of LDS.
//
// This kernel keeps ITS OWN COPY of the clamped box, of the walk (kg_job_box / kg_box_walk of label_common.h state the rule: the same
// clamp, the same flat row-major list, additions only) and of the four-wave combine: written with the shared functions its 3-channel
// leg measured 10-25 % slower than with this text, twice (profiles/labelcommon_ab.json).  A change to the walk or the clamp in
// label_common.h is made here too.
//
// 32-bit partials, with their bound: a box holds at most 2^30 pixels, so a thread visits at most 2^22 of them and a wave 2^28; the five
// counts (area, the three edge counts, boundary pixels) add at most 4 per visited pixel, so a thread's count stays below 2^24 and a
// wave's sum at or below 2^30.  Every other sum is 64-bit in the thread: a coordinate sum reaches 2^37 there, a uint16 sum of squares 2^54.
template <int C, typename T>
__global__ __launch_bounds__(256) void label_measure_kernel(const int* __restrict__ labels, int nimg, int H, int W, const T* __restrict__ image,
                                                            const int* __restrict__ jobs, int m, long long* __restrict__ out) {
    constexpr int NCOL = KG_MS_GEOM + 4 * C;
    __shared__ long long part[4][NCOL];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long j = blockIdx.x; j < m; j += gridDim.x) {
        const int* jb = jobs + j * 6;
        const int img = jb[0], id = jb[1];
        int by1 = jb[2], bx1 = jb[3], by2 = jb[4], bx2 = jb[5];
        by1 = by1 < 0 ? 0 : by1; bx1 = bx1 < 0 ? 0 : bx1;
        by2 = by2 > H ? H : by2; bx2 = bx2 > W ? W : bx2;
        const bool ok = (unsigned)img < (unsigned)nimg;                // the only use of img before it scales an address
        const int bh = ok && by2 > by1 ? by2 - by1 : 0, bw = ok && bx2 > bx1 ? bx2 - bx1 : 0;
        int area = 0, edges = 0, e_border = 0, e_contact = 0, bpix = 0;
        long long sy = 0, sx = 0, syy = 0, syx = 0, sxx = 0;
        long long vsum[C ? C : 1], vsq[C ? C : 1];
        int vmin[C ? C : 1], vmax[C ? C : 1];
#pragma unroll
        for (int c = 0; c < (C ? C : 1); ++c) { vsum[c] = 0; vsq[c] = 0; vmin[c] = INT_MAX; vmax[c] = 0; }
        if (bh > 0 && bw > 0) {
            const long base = (long)img * H * W;                       // img < nimg: base + H * W <= nimg * H * W <= 2^31 - 1
            const int stepy = 256 / bw, stepx = 256 - stepy * bw;
            int yy = (int)threadIdx.x / bw, xx = (int)threadIdx.x - yy * bw;
            while (yy < bh) {
                const int Y = by1 + yy, X = bx1 + xx;
                const long p = base + (long)Y * W + X;
                if (labels[p] == id) {
                    ++area; sy += Y; sx += X;
                    syy += (long long)Y * Y; syx += (long long)Y * X; sxx += (long long)X * X;
                    int e = 0, eb = 0, ec = 0;
                    // up, down, left, right: the coordinate decides "outside the map" before the neighbour's address exists
                    if (Y == 0) { ++e; ++eb; } else { const int v = labels[p - W]; e += v != id; ec += (v != id) & (v != 0); }
                    if (Y == H - 1) { ++e; ++eb; } else { const int v = labels[p + W]; e += v != id; ec += (v != id) & (v != 0); }
                    if (X == 0) { ++e; ++eb; } else { const int v = labels[p - 1]; e += v != id; ec += (v != id) & (v != 0); }
                    if (X == W - 1) { ++e; ++eb; } else { const int v = labels[p + 1]; e += v != id; ec += (v != id) & (v != 0); }
                    edges += e; e_border += eb; e_contact += ec; bpix += e != 0;
                    if constexpr (C > 0) {
                        const T* px = image + p * C;
#pragma unroll
                        for (int c = 0; c < C; ++c) {
                            const int v = (int)px[c];
                            vsum[c] += v; vsq[c] += (long long)v * v;
                            vmin[c] = v < vmin[c] ? v : vmin[c]; vmax[c] = v > vmax[c] ? v : vmax[c];
                        }
                    }
                }
                xx += stepx; yy += stepy;
                if (xx >= bw) { xx -= bw; ++yy; }
            }
        }
        area = kg_wave_sum(area); edges = kg_wave_sum(edges); e_border = kg_wave_sum(e_border); e_contact = kg_wave_sum(e_contact);
        bpix = kg_wave_sum(bpix);
        sy = kg_wave_sum(sy); sx = kg_wave_sum(sx); syy = kg_wave_sum(syy); syx = kg_wave_sum(syx); sxx = kg_wave_sum(sxx);
        if constexpr (C > 0) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                vsum[c] = kg_wave_sum(vsum[c]); vsq[c] = kg_wave_sum(vsq[c]); vmin[c] = kg_wave_min(vmin[c]); vmax[c] = kg_wave_max(vmax[c]);
            }
        }
        if (lane == 0) {
            long long* q = part[wave];
            q[0] = area; q[1] = sy; q[2] = sx; q[3] = syy; q[4] = syx; q[5] = sxx; q[6] = edges; q[7] = e_border; q[8] = e_contact; q[9] = bpix;
            if constexpr (C > 0) {
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    q[KG_MS_GEOM + 4 * c] = vsum[c]; q[KG_MS_GEOM + 4 * c + 1] = vsq[c];
                    q[KG_MS_GEOM + 4 * c + 2] = vmin[c]; q[KG_MS_GEOM + 4 * c + 3] = vmax[c];
                }
            }
        }
        __syncthreads();
        if (threadIdx.x < NCOL) {
            const int c = threadIdx.x;
            const int kind = c < KG_MS_GEOM ? 0 : (c - KG_MS_GEOM) & 3;   // 2: a minimum, 3: a maximum, else a sum
            long long v = part[0][c];
            for (int w = 1; w < 4; ++w) {
                const long long t = part[w][c];
                if (kind == 2) v = t < v ? t : v;
                else if (kind == 3) v = t > v ? t : v;
                else v += t;
            }
            const long long total = part[0][0] + part[1][0] + part[2][0] + part[3][0];
            if (total == 0 && kind == 2) v = 0;                        // no pixel: min (still INT_MAX) and max are 0
            out[j * NCOL + c] = v;
        }
        __syncthreads();                                               // part is written again by the block's next job
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
template <int C, typename T>
static void ms_launch(const int* labels, int nimg, int H, int W, const void* image, const int* jobs, int m, long long* out, hipStream_t stream) {
    hipLaunchKernelGGL((label_measure_kernel<C, T>), dim3(kg_grid_cap(m)), dim3(256), 0, stream, labels, nimg, H, W,
                       (const T*)image, jobs, m, out);
}

// labels: device int32 [nimg][H][W]; image: device [nimg][H][W][channels] of elem_bytes-byte unsigned elements, NULL exactly when channels
// == 0; jobs: device int32 [m][6] = (img, id, y1, x1, y2, x2), written by the caller; out: device int64 [m][10 + 4 * channels]
extern "C" int kg_label_measure(const int* labels, int nimg, int H, int W, const void* image, int channels, int elem_bytes, const int* jobs, int m,
                                long long* out, void* stream) {
    // H, W <= KG_LABEL_MAX_SIDE (2^15): area <= 2^30, a coordinate product < 2^30, a coordinate sum < 2^60, and a uint16 sum of squares
    // < 2^62 -- every column fits int64 and nothing else needs checking
    KG_TRY(kg_check_job_stack("kg_label_measure", labels, nimg, H, W, jobs, m));
    KG_CHECK_ARG(channels >= 0 && channels <= 4, "kg_label_measure: channels %d (0 .. 4)", channels);
    KG_CHECK_ARG(elem_bytes == 1 || elem_bytes == 2, "kg_label_measure: elem_bytes %d (1 or 2)", elem_bytes);
    KG_CHECK_ARG((image != nullptr) == (channels > 0), "kg_label_measure: image must be NULL exactly when channels == 0 (channels %d)", channels);
    KG_CHECK_ARG(out || m == 0, "kg_label_measure: null pointer (out)");
    KG_CHECK_ARG(kg_aligned(out, 7) && kg_aligned(image, elem_bytes == 2 ? 1 : 0), "kg_label_measure: misaligned pointer");
    if (m == 0) return KG_OK;
    hipStream_t s = (hipStream_t)stream;
    switch (channels * 2 + (elem_bytes == 2)) {
        case 0: case 1: ms_launch<0, unsigned char>(labels, nimg, H, W, image, jobs, m, out, s); break;
        case 2: ms_launch<1, unsigned char>(labels, nimg, H, W, image, jobs, m, out, s); break;
        case 3: ms_launch<1, unsigned short>(labels, nimg, H, W, image, jobs, m, out, s); break;
        case 4: ms_launch<2, unsigned char>(labels, nimg, H, W, image, jobs, m, out, s); break;
        case 5: ms_launch<2, unsigned short>(labels, nimg, H, W, image, jobs, m, out, s); break;
        case 6: ms_launch<3, unsigned char>(labels, nimg, H, W, image, jobs, m, out, s); break;
        case 7: ms_launch<3, unsigned short>(labels, nimg, H, W, image, jobs, m, out, s); break;
        case 8: ms_launch<4, unsigned char>(labels, nimg, H, W, image, jobs, m, out, s); break;
        default: ms_launch<4, unsigned short>(labels, nimg, H, W, image, jobs, m, out, s); break;
    }
    KG_CHECK_LAUNCH("label_measure");
    return KG_OK;
}
