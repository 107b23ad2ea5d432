// linking.hip -- which values of ANOTHER label map lie under the pixels of an instance, on gfx950 (linking.py): the overlap lists that
// link the frames of a time-lapse, stitch the planes of a stack and relate the objects of two segmentations.
//   kg_label_overlaps  per job {img_a, id, box, img_b, dy, dx, resume, after}: with P = the pixels of the box in a[img_a] that hold id,
//                      the partner of (y, x) is (y + dy, x + dx) in b[img_b]; the row holds |P|, the partners that hold 0, the partners
//                      outside the map, and the non-zero partner values in ascending signed order, each with its pixel count, `slots` of
//                      them per row
//
// The index rule of label_common.h holds here without a new exception.  The job table is the one device-read table: its box is clamped to
// the map before any address is formed (kg_job_box); img_a and img_b are used only inside (unsigned)img < (unsigned)nimg predicates that
// empty the box when they fail (such a job writes a row of zeros and reads nothing else); the partner coordinate is a 64-bit sum of a box
// coordinate and dy / dx, used only inside (unsigned long long)(Y + dy) < H and (unsigned long long)(X + dx) < W BEFORE its address
// exists, so dy / dx of INT_MIN / INT_MAX read nothing; resume / after are compared with label values, nothing else.  Label values of
// either map are compared, counted and stored only: there is no table a value could index, hence no hash and no atomics, and the row is
// the same from run to run.  a and b are read only and may be one buffer.
#include "label_common.h"

#define KG_OV_MAX_SLOTS 64
#define KG_OV_NONE LLONG_MAX            // "no value": every key is an int32 widened to 64 bits, so INT_MIN and INT_MAX need no sentinel

__device__ __forceinline__ long long kg_ov_wave_min(long long v) {
    for (int o = 32; o; o >>= 1) { const long long t = __shfl_xor(v, o); v = t < v ? t : v; }
    return v;
}

// One block per job (the grid strides when there are more jobs than KG_LABEL_MAX_BLOCKS).  The ordered extraction of
// label_neighbours_kernel: the block holds a uniform threshold thr (below every int32 at first, `after` when the job resumes) and walks
// the box; a walk takes the block minimum N of the non-zero partner values above thr and, once a current value exists, counts the
// partners that hold it (== thr) on the same pass.  Then the current value is written to its slot and N becomes the current value.  The
// first walk also takes the three header counts (area, zero, outside), which are over all of P whatever thr is.  k distinct values cost
// min(k, slots) + 1 walks; both maps stay in L2 between them (a nucleus box is a few hundred pixels).
//
// 32-bit partials, with their bound: a box holds at most 2^30 pixels (H, W <= KG_LABEL_MAX_SIDE), so a thread visits at most 2^22 of
// them and a wave 2^28; every count adds at most 1 per visited pixel, so a thread's count stays at or below 2^22 and a wave's sum at or
// below 2^28.  The block sums are formed in 64 bits.
//
// part is double-buffered by the parity of the walk: a thread that writes part[q] for walk k + 2 has passed the barrier of walk k + 1,
// which every thread reaches only after it has read part[q] of walk k.  One barrier per walk.
__global__ __launch_bounds__(256) void label_overlaps_kernel(const int* a, int nimg_a, const int* b, int nimg_b, int H, int W,
                                                             const int* __restrict__ jobs, int m, int slots, long long* __restrict__ out) {
    __shared__ long long part[2][4][5];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ncol = 5 + 2 * slots;
    unsigned walk = 0;
    for (long j = blockIdx.x; j < m; j += gridDim.x) {
        const int* jb = jobs + j * 11;
        const int img_a = jb[0], id = jb[1], img_b = jb[6];
        const long long dy = jb[7], dx = jb[8];
        KgBox box = kg_job_box(jb + 2, H, W);
        // the only uses of img_a and img_b before they scale an address
        if (!((unsigned)img_a < (unsigned)nimg_a) || !((unsigned)img_b < (unsigned)nimg_b)) box.h = box.w = 0;
        const long base_a = (long)img_a * H * W, base_b = (long)img_b * H * W;   // used only with a non-empty box: both predicates hold
        long long thr = jb[9] != 0 ? (long long)jb[10] : (long long)INT_MIN - 1;
        bool counting = false;                                         // thr is a partner value whose pixel count is wanted
        int count = 0, more = 0;
        long long area = 0, zero = 0, outside = 0;
        long long* row = out + j * ncol;
        for (int w = 0; w <= slots; ++w) {                             // (it leaves through a break: at w == slots, count == slots)
            const int cur = (int)thr;
            long long nxt = KG_OV_NONE;
            int pixels = 0, n_area = 0, n_zero = 0, n_outside = 0;
            kg_box_walk(box, [&](int Y, int X) {
                if (a[base_a + (long)Y * W + X] == id) {
                    ++n_area;
                    // the coordinates decide "outside the map" in 64 bits before the partner's address exists
                    const long long PY = (long long)Y + dy, PX = (long long)X + dx;
                    if ((unsigned long long)PY < (unsigned long long)H && (unsigned long long)PX < (unsigned long long)W) {
                        const int v = b[base_b + PY * W + PX];
                        if (v == 0) ++n_zero;
                        else {
                            pixels += counting && v == cur;
                            if ((long long)v > thr && (long long)v < nxt) nxt = v;
                        }
                    } else ++n_outside;
                }
            });
            nxt = kg_ov_wave_min(nxt); pixels = kg_wave_sum(pixels);
            long long (*q)[5] = part[walk++ & 1];
            if (w == 0) {                                              // uniform: the header counts travel with the first walk only
                n_area = kg_wave_sum(n_area); n_zero = kg_wave_sum(n_zero); n_outside = kg_wave_sum(n_outside);
                if (lane == 0) { q[wave][2] = n_area; q[wave][3] = n_zero; q[wave][4] = n_outside; }
            }
            if (lane == 0) { q[wave][0] = nxt; q[wave][1] = pixels; }
            __syncthreads();
            long long N = q[0][0], S = q[0][1];                        // every thread forms the same numbers: the loop stays uniform
            for (int k = 1; k < 4; ++k) { N = q[k][0] < N ? q[k][0] : N; S += q[k][1]; }
            if (w == 0) {
                area = q[0][2] + q[1][2] + q[2][2] + q[3][2];
                zero = q[0][3] + q[1][3] + q[2][3] + q[3][3];
                outside = q[0][4] + q[1][4] + q[2][4] + q[3][4];
            }
            if (counting) {
                if (threadIdx.x == 0) { row[5 + 2 * count] = cur; row[6 + 2 * count] = S; }
                ++count;
            }
            if (N == KG_OV_NONE) break;
            if (count == slots) { more = 1; break; }
            thr = N; counting = true;
        }
        if (threadIdx.x == 0) { row[0] = count; row[1] = more; row[2] = area; row[3] = zero; row[4] = outside; }
        for (int c = 5 + 2 * count + (int)threadIdx.x; c < ncol; c += 256) row[c] = 0;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// a: device int32 [nimg_a][H][W]; b: device int32 [nimg_b][H][W] (may be a); jobs: device int32 [m][11] = (img_a, id, y1, x1, y2, x2,
// img_b, dy, dx, resume, after), written by the caller; out: device int64 [m][5 + 2 * slots] = {count, more, area, zero, outside,
// (value, pixels) x slots}
extern "C" int kg_label_overlaps(const int* a, int nimg_a, const int* b, int nimg_b, int H, int W, const int* jobs, int m, int slots,
                                 long long* out, void* stream) {
    // H, W <= KG_LABEL_MAX_SIDE: a box holds <= 2^30 pixels, which is what the 32-bit partials of the kernel rely on
    KG_TRY(kg_check_job_stack("kg_label_overlaps", a, nimg_a, H, W, jobs, m));
    KG_TRY(kg_check_job_stack("kg_label_overlaps", b, nimg_b, H, W, jobs, m));
    KG_CHECK_ARG(slots >= 1 && slots <= KG_OV_MAX_SLOTS, "kg_label_overlaps: slots %d (1 .. %d)", slots, KG_OV_MAX_SLOTS);
    KG_CHECK_ARG(out || m == 0, "kg_label_overlaps: null pointer (out)");
    KG_CHECK_ARG(kg_aligned(out, 7), "kg_label_overlaps: misaligned pointer");
    const long out_bytes = (long)m * (5 + 2 * slots) * 8;
    KG_CHECK_ARG(kg_apart(out, out_bytes, a, (long)nimg_a * H * W * 4) && kg_apart(out, out_bytes, b, (long)nimg_b * H * W * 4)
                 && kg_apart(out, out_bytes, jobs, (long)m * 44), "kg_label_overlaps: out overlaps an input");
    if (m == 0) return KG_OK;
    hipLaunchKernelGGL(label_overlaps_kernel, dim3(kg_grid_cap(m)), dim3(256), 0, (hipStream_t)stream, a, nimg_a, b, nimg_b, H, W, jobs, m, slots, out);
    KG_CHECK_LAUNCH("label_overlaps");
    return KG_OK;
}
