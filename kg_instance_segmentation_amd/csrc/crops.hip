// crops.hip -- fixed-size patches and masks per instance of instance label maps on gfx950 (crops.py): the instance itself in the form the next
// model takes.  The first kernel of the family whose output is pixels and not integers about pixels: a gather with integer arithmetic.
//   kg_label_crops   per job {img, id, oy, ox, ay, by, cy, ax, bx, cx}: output pixel (i, j) of an OH x OW patch samples the source position
//                    Y = (oy << 16) + ay i + by j + cy, X = (ox << 16) + ax i + bx j + cx (int64, 1/65536 pixel, pixel centres at integers);
//                    patches [m][C][OH][OW] in the image's element type (bilinear or nearest, a tap outside the map is `fill`) and masks
//                    [m][OH][OW] uint8 (labels == id at the nearest pixel).  The kernel knows nothing of windows or angles: crops.affine_jobs
//                    builds the table on the host.
//
// A work item is (job, chunk of 1024 output positions in raster order); a thread owns 4 consecutive positions of its chunk, so the stores of
// a wave into one channel plane are 256 contiguous elements, and a thread's 4 uint8 (2 + 2 uint16) elements go out as 32-bit vector stores
// where the plane offset is 4-byte aligned and the 4 positions exist, as element stores elsewhere (OH * OW odd with 3 channels misaligns
// every second plane).  The positions' taps are formed once and serve every channel.  No atomics, no LDS, no synchronisation; taps are plain
// loads of the interleaved [H][W][C] image (tools/crops_bench.py measures it against a copy of the bytes it writes).
//
// The index rule of label_common.h holds with its first exception, the caller's job table: img is used inside (unsigned)img < (unsigned)nimg;
// every tap (y, x) is used inside the unsigned 64-bit predicates (unsigned long long)y < H and (unsigned long long)x < W, formed from the
// int64 Y, X BEFORE any narrowing, so extreme coefficients (INT_MIN, INT_MAX) and far origins give `fill` and cannot leave the buffers:
// |Y| <= 2^47 + 255 * 2^32 + 2^31 < 2^63.  No address depends on a label or a pixel value.
#include "label_common.h"

#define KG_CROPS_NEAREST 1              // flags bit 0: the tap at the nearest pixel (0: bilinear)
#define KG_CROPS_MASKED 2               // flags bit 1: a pixel whose mask is 0 becomes fill
#define KG_CROPS_MAX_SIDE 256
#define KG_CROPS_CHUNK 1024             // output positions per work item: 256 threads x 4 consecutive positions

// the pixel index of the tap (y, x) in the stack, or -1 outside the map (or for a bad job): base + y * W + x <= nimg * H * W - 1 <= 2^31 - 2
__device__ __forceinline__ int crops_tap(bool live, long long y, long long x, int base, int H, int W) {
    return live && (unsigned long long)y < (unsigned long long)H && (unsigned long long)x < (unsigned long long)W ? base + (int)y * W + (int)x : -1;
}

template <typename T>
__device__ __forceinline__ void crops_store4(T* __restrict__ dst, const unsigned (&v)[4], int n) {
    if (n == 4 && (((unsigned long long)(size_t)dst) & 3) == 0) {
        if (sizeof(T) == 1) {
            *(unsigned*)dst = v[0] | v[1] << 8 | v[2] << 16 | v[3] << 24;
        } else {
            ((unsigned*)dst)[0] = v[0] | v[1] << 16;
            ((unsigned*)dst)[1] = v[2] | v[3] << 16;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) dst[k] = (T)v[k];
    }
}

template <typename T, bool NEAREST>
__global__ __launch_bounds__(256) void label_crops_kernel(const int* __restrict__ labels, int nimg, int H, int W, const T* __restrict__ image, int C,
                                                          const int* __restrict__ jobs, long items, int nchunk, int OH, int OW, int masked,
                                                          unsigned fill, T* __restrict__ patches, unsigned char* __restrict__ masks) {
    const int OHW = OH * OW;                                           // <= 65536
    const bool want_label = masks != nullptr || masked;
    for (long item = blockIdx.x; item < items; item += gridDim.x) {
        const long job = item / nchunk;
        const int chunk = (int)(item - job * nchunk);
        const int* jb = jobs + job * 10;
        const int img = jb[0], id = jb[1];
        const bool live = (unsigned)img < (unsigned)nimg;
        const int base = live ? img * (H * W) : 0;                     // img < nimg: base + H * W <= nimg * H * W <= 2^31 - 1
        const long long oy = (long long)jb[2] * 65536, ox = (long long)jb[3] * 65536;
        const long long ay = jb[4], by = jb[5], cy = jb[6], ax = jb[7], bx = jb[8], cx = jb[9];
        const int p0 = chunk * KG_CROPS_CHUNK + (int)threadIdx.x * 4;  // < 65536 + 1024
        const int n = OHW - p0 < 4 ? OHW - p0 : 4;                     // the thread's positions that exist; <= 0: none
        if (n <= 0) continue;
        int t00[4], t01[4], t10[4], t11[4];                            // tap pixel indices, -1 = fill; NEAREST uses t00 only
        unsigned fy[4], fx[4], mk[4];
        int i = p0 / OW, j = p0 - i * OW;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool here = k < n;
            const long long Y = oy + ay * i + by * j + cy, X = ox + ax * i + bx * j + cx;
            const int pn = crops_tap(live && here, (Y + 32768) >> 16, (X + 32768) >> 16, base, H, W);
            mk[k] = want_label && pn >= 0 && labels[pn] == id ? 1u : 0u;
            if (NEAREST) {
                t00[k] = pn;
            } else {
                const long long y0 = Y >> 16, x0 = X >> 16;
                fy[k] = (unsigned)(Y & 65535); fx[k] = (unsigned)(X & 65535);
                t00[k] = crops_tap(live && here, y0, x0, base, H, W);
                t01[k] = crops_tap(live && here, y0, x0 + 1, base, H, W);
                t10[k] = crops_tap(live && here, y0 + 1, x0, base, H, W);
                t11[k] = crops_tap(live && here, y0 + 1, x0 + 1, base, H, W);
            }
            if (++j == OW) { j = 0; ++i; }
        }
        if (masks != nullptr) crops_store4(masks + job * OHW + p0, mk, n);     // job * OHW + p0 < m * OH * OW <= 2^31 - 1
        if (patches != nullptr) {
            for (int c = 0; c < C; ++c) {
                unsigned v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    unsigned r;
                    if (NEAREST) {
                        r = t00[k] >= 0 ? (unsigned)image[(long)t00[k] * C + c] : fill;
                    } else {
                        const unsigned long long v00 = t00[k] >= 0 ? (unsigned)image[(long)t00[k] * C + c] : fill;
                        const unsigned long long v01 = t01[k] >= 0 ? (unsigned)image[(long)t01[k] * C + c] : fill;
                        const unsigned long long v10 = t10[k] >= 0 ? (unsigned)image[(long)t10[k] * C + c] : fill;
                        const unsigned long long v11 = t11[k] >= 0 ? (unsigned)image[(long)t11[k] * C + c] : fill;
                        const unsigned long long gx = 65536u - fx[k], gy = 65536u - fy[k];
                        const unsigned long long acc = gy * (gx * v00 + fx[k] * v01) + fy[k] * (gx * v10 + fx[k] * v11);   // < 2^48
                        r = (unsigned)((acc + 0x80000000ull) >> 32);
                    }
                    v[k] = masked && !mk[k] ? fill : r;
                }
                crops_store4(patches + (job * C + c) * OHW + p0, v, n);        // < m * C * OH * OW <= 2^31 - 1
            }
        }
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// labels: device int32 [nimg][H][W]; image: device [nimg][H][W][channels] of elem_bytes-byte unsigned elements, or NULL (masks only);
// jobs: device int32 [m][10] = (img, id, oy, ox, ay, by, cy, ax, bx, cx); patches: device [m][channels][OH][OW] of the image's elements, or
// NULL; masks: device uint8 [m][OH][OW], or NULL (patches only)
extern "C" int kg_label_crops(const int* labels, int nimg, int H, int W, const void* image, int channels, int elem_bytes, const int* jobs, int m,
                              int OH, int OW, int flags, int fill, void* patches, unsigned char* masks, void* stream) {
    const char* fn = "kg_label_crops";
    KG_TRY(kg_check_job_stack(fn, labels, nimg, H, W, jobs, m));
    if (image || patches) KG_TRY(kg_check_image(fn, image, channels, elem_bytes));
    KG_CHECK_ARG(OH >= 1 && OH <= KG_CROPS_MAX_SIDE && OW >= 1 && OW <= KG_CROPS_MAX_SIDE, "%s: output size %d x %d (1 .. %d)", fn, OH, OW,
                 KG_CROPS_MAX_SIDE);
    KG_CHECK_ARG((flags & ~(KG_CROPS_NEAREST | KG_CROPS_MASKED)) == 0, "%s: flags %d (bit 0 nearest, bit 1 masked)", fn, flags);
    KG_CHECK_ARG(fill >= 0 && fill <= 65535, "%s: fill %d (0 .. 65535)", fn, fill);
    KG_CHECK_ARG(!patches || elem_bytes == 2 || fill <= 255, "%s: fill %d does not fit a 1-byte element", fn, fill);
    KG_CHECK_ARG(patches || masks || m == 0, "%s: null pointer (patches and masks: at least one output)", fn);
    const int C = patches ? channels : 1;
    KG_CHECK_ARG((long)m * C <= 0x7fffffffL / ((long)OH * OW), "%s: m * C * OH * OW exceeds 2^31 - 1", fn);
    KG_CHECK_ARG(kg_aligned(patches, elem_bytes == 2 ? 1 : 0), "%s: misaligned pointer (patches)", fn);
    const long map_bytes = (long)nimg * H * W * 4, img_bytes = image ? (long)nimg * H * W * channels * elem_bytes : 0;
    const long patch_bytes = patches ? (long)m * C * OH * OW * elem_bytes : 0, mask_bytes = masks ? (long)m * OH * OW : 0;
    KG_CHECK_ARG(kg_apart(patches, patch_bytes, labels, map_bytes) && kg_apart(patches, patch_bytes, image, img_bytes)
                 && kg_apart(patches, patch_bytes, jobs, (long)m * 40) && kg_apart(masks, mask_bytes, labels, map_bytes)
                 && kg_apart(masks, mask_bytes, image, img_bytes) && kg_apart(masks, mask_bytes, jobs, (long)m * 40)
                 && kg_apart(patches, patch_bytes, masks, mask_bytes), "%s: an output overlaps an input or the other output", fn);
    if (m == 0) return KG_OK;
    hipStream_t s = (hipStream_t)stream;
    const int nchunk = (OH * OW + KG_CROPS_CHUNK - 1) / KG_CROPS_CHUNK;
    const long items = (long)m * nchunk;
    const dim3 grid(kg_grid_cap(items)), block(256);
    const int masked = (flags & KG_CROPS_MASKED) != 0;
    const bool nearest = (flags & KG_CROPS_NEAREST) != 0 || !patches;  // without patches only the mask's nearest tap is formed
#define KG_CROPS_LAUNCH(T, NEAR)                                                                                                                \
    hipLaunchKernelGGL((label_crops_kernel<T, NEAR>), grid, block, 0, s, labels, nimg, H, W, (const T*)image, C, jobs, items, nchunk, OH, OW, masked, \
                       (unsigned)fill, (T*)patches, masks)
    if (patches && elem_bytes == 2) {
        if (nearest) KG_CROPS_LAUNCH(unsigned short, true); else KG_CROPS_LAUNCH(unsigned short, false);
    } else {
        if (nearest) KG_CROPS_LAUNCH(unsigned char, true); else KG_CROPS_LAUNCH(unsigned char, false);
    }
#undef KG_CROPS_LAUNCH
    KG_CHECK_LAUNCH("label_crops");
    return KG_OK;
}
