// sampleprep.hip -- a decoded training sample (uint8 image + instance masks) -> the network's inputs and targets, on gfx950.
// Reference: BaseDataset.__getitem__ (dataset_base.py:81-116) under train.py:77-85's pipelines:
//   ConvertImgFloat -> PhotometricDistort -> Expand(max_scale 2, mean 0) -> RandomMirror_w -> RandomMirror_h -> Resize   (train)
//   ConvertImgFloat -> Resize                                                                                            (val)
// The reference runs this per instance on the host (transforms.py:86-106 allocates an [n, He, We] float canvas, :165-176 resizes every
// mask separately, dataset_base.py:58-79 resizes and scans every mask four more times, :43-56 once more).  Here Expand, the mirrors and
// the nearest resize compose into ONE source index per output pixel, so the canvas never exists:
//   v = min(floor(d * scale), Ce - 1), scale = 1 / (D / Ce) in double   (transforms.py:174, INTER_NEAREST: canvas size Ce -> output size D)
//   v = mirror ? Ce - 1 - v : v                                         (transforms.py:148-162)
//   s = v - offset, outside [0, size) -> the fill value 0               (transforms.py:99-104)
// The image goes through the same map per bilinear tap (transforms.py:170, float32 INTER_LINEAR as lin_taps.h / oracle/paste.py state
// it), after the photometric arithmetic (transforms.py:32,45: two float32 operations) and before dataset_base.py:104-106.
// Compiled with -ffp-contract=off: every float product and sum rounds as written.
//
// Ground truth may also arrive as ONE int32 label map per image (flag SP_LABELS) with a job table (img, id, y1, x1, y2, x2) in place of
// one plane per instance: kg_sp_warp_labels warps `labels == id` through the same source index, kg_sp_warp_labelmap the map itself.
// The index rule of label_common.h holds there, with its first exception, the caller's job table: img and the box are PREDICATES only.
// img selects an image record only inside (unsigned)img < (unsigned)N, the box is clamped to the map (kg_job_box) and only gates the
// load, and the address of the load is formed from the output pixel's own source index (sp_src: inside [0, h) x [0, w) or -1), never
// from the table and never from a label: id and the labels are compared only.  A hostile table gives zeros or wrong pixels and cannot
// leave the buffers.  The source is loaded only where the row and the column predicate hold, so an output pixel outside the forward
// image of the box costs a store and no load.
#include "kg_common.h"
#include "label_common.h"
#include "lin_taps.h"

#define SP_MAXW 4096            // widest output row (the column map of a row lives in LDS)
#define SP_MIRROR_W 1
#define SP_MIRROR_H 2
#define SP_BITS 4
#define SP_LABELS 8             // masks = int32 [h][w], the label map of the image (kg_sp_warp_labels, kg_sp_warp_labelmap); ld is ignored

// one image of the batch (80 bytes; sampleprep.py builds the table with the same layout)
struct SpImage {
    const unsigned char* img;   // uint8 [h][w][3]
    const void* masks;          // bytes [n][h][w] (any non-zero value is foreground) or, with SP_BITS, 64-bit words [n][ld] (bit-mask layout)
    int h, w, He, We;           // source size; canvas after Expand (== source size when Expand is off)
    int oy, ox, flags, perm;    // paste window origin; SP_* flags; source channel of output channel c = (perm >> 2c) & 3
    float delta, alpha;         // brightness / contrast (0 and 1 when off)
    int inst0, n;               // first instance of the image in the batch-wide instance order, instance count
    long ld;                    // elements between two masks: h * w bytes, or ld_words
    long pad_;
};
static_assert(sizeof(SpImage) == 80, "sampleprep.py mirrors this layout");

// source index of destination index d (canvas ce -> output dsize, then mirror, then the Expand window); -1 outside the window
__device__ __forceinline__ int sp_src(int d, int size, int ce, int off, bool mirror, int dsize) {
    const double scale = 1.0 / ((double)dsize / (double)ce);
    int v = (int)floor((double)d * scale);
    if (v > ce - 1) v = ce - 1;
    if (mirror) v = ce - 1 - v;
    const int s = v - off;
    return s >= 0 && s < size ? s : -1;
}

// ---- image ------------------------------------------------------------------------------------------------------------------------
// value of channel c (already permuted: pc = source channel) of the mirrored canvas at (vy, vx)
__device__ __forceinline__ float sp_canvas(const SpImage& im, int pc, int vy, int vx) {
    if (im.flags & SP_MIRROR_H) vy = im.He - 1 - vy;
    if (im.flags & SP_MIRROR_W) vx = im.We - 1 - vx;
    const int sy = vy - im.oy, sx = vx - im.ox;
    if (sy < 0 || sy >= im.h || sx < 0 || sx >= im.w) return 0.f;                    // Expand's mean (train.py: 0)
    const float v = (float)im.img[((long)sy * im.w + sx) * 3 + pc];
    const float a = v + im.delta;                                                    // transforms.py:45
    return a * im.alpha;                                                             // transforms.py:32
}

// one lane: 4 adjacent pixels of one row, the three channels; out [N][3][H][W]
__global__ __launch_bounds__(256) void sp_image_kernel(const SpImage* __restrict__ imgs, int H, int W, float* __restrict__ out) {
    const int q = blockIdx.x * 256 + threadIdx.x, qpr = W >> 2;
    if (q >= H * qpr) return;
    const int y = q / qpr, x0 = (q - y * qpr) << 2;
    const SpImage im = imgs[blockIdx.y];
    const bool same = im.He == H && im.We == W;
    const Taps ty = lin_taps(y, im.He, H, false);
    float v[3][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const Taps tx = lin_taps(x0 + e, im.We, W, true);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int pc = (im.perm >> (2 * c)) & 3;
            float r;
            if (same) r = sp_canvas(im, pc, y, x0 + e);
            else {
                const float r0 = lin_row(sp_canvas(im, pc, ty.s0, tx.s0), sp_canvas(im, pc, ty.s0, tx.s1), tx);
                const float r1 = lin_row(sp_canvas(im, pc, ty.s1, tx.s0), sp_canvas(im, pc, ty.s1, tx.s1), tx);
                const float a = r0 * ty.c0, b = r1 * ty.c1;
                r = a + b;
            }
            r = r < 0.f ? 0.f : (r > 255.f ? 255.f : r);                             // dataset_base.py:104
            const float d = r / 255.f;                                               // dataset_base.py:105
            v[c][e] = d - 0.5f;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
        *reinterpret_cast<float4*>(out + (((long)blockIdx.y * 3 + c) * H + y) * W + x0) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
}

// imgs: device SpImage [N]; out: device float32 [N][3][H][W] (dataset_base.py:104-108 + collater.py:20)
extern "C" int kg_sp_image(const void* imgs, int N, int H, int W, float* out, void* stream) {
    KG_CHECK_ARG(imgs && out && N > 0 && N <= 65535, "kg_sp_image: bad arguments");
    KG_CHECK_ARG(H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0 && H <= 65535 && W <= SP_MAXW, "kg_sp_image: output %d x %d must be multiples of 8, W <= %d", H, W,
                 SP_MAXW);
    hipLaunchKernelGGL(sp_image_kernel, dim3((unsigned)kg_cdiv((long)H * (W >> 2), 256), (unsigned)N), dim3(256), 0, (hipStream_t)stream,
                       (const SpImage*)imgs, H, W, out);
    KG_CHECK_LAUNCH("sp_image");
    return KG_OK;
}

// ---- masks ------------------------------------------------------------------------------------------------------------------------
// A workgroup serves one instance x 256 pixel groups; a lane produces PX adjacent pixels of one row and stores them as ONE dword (PX 4)
// or dwordx4 (PX 16).  The column map of the image is built once per workgroup in LDS; a lane walks its PX source columns through the
// current source row, re-reading a 64-bit word only when the column leaves it (bit sources: one word serves 64 source pixels).
// Boxes (dataset_base.py:58-79 at divide scales 1, 2, 4, 8 and :43-56): for H, W multiples of 8 the nearest-downscaled mask of scale s
// samples exactly the pixels (y s, x s), so the same pass yields all four: every lane that holds a one of scale s folds its row and its
// first / last column into the workgroup's LDS box, and the workgroup folds that into the instance's box with vector integer atomics.
// Encoding (all maxima, so a zero-filled buffer means "empty"): box[k][4 l + {0,1,2,3}] = {0x10000 - ymin, 0x10000 - xmin, ymax + 1, xmax + 1}.
template <int PX>
__global__ __launch_bounds__(256) void sp_warp_kernel(const SpImage* __restrict__ imgs, const int* __restrict__ inst_img, int ntot, int H, int W,
                                                      unsigned char* __restrict__ out, int* __restrict__ box) {
    __shared__ int xmap[SP_MAXW];
    __shared__ int sbox[16];
    const int gpr = W / PX, ngroups = H * gpr;
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int y = g / gpr, x0 = (g - y * gpr) * PX;
    for (int k = blockIdx.y; k < ntot; k += gridDim.y) {
        const SpImage im = imgs[inst_img[k]];
        __syncthreads();
        for (int x = threadIdx.x; x < W; x += 256) xmap[x] = sp_src(x, im.w, im.We, im.ox, im.flags & SP_MIRROR_W, W);
        if (threadIdx.x < 16) sbox[threadIdx.x] = 0;
        __syncthreads();
        if (g < ngroups) {
            const int sy = sp_src(y, im.h, im.He, im.oy, im.flags & SP_MIRROR_H, H);
            const long j = k - im.inst0;
            unsigned m = 0;
            if (sy >= 0) {
                if (im.flags & SP_BITS) {
                    const int wpr = (im.w + 63) >> 6;
                    const unsigned long long* row = (const unsigned long long*)im.masks + j * im.ld + (long)sy * wpr;
                    int cur = -1;
                    unsigned long long word = 0;
#pragma unroll
                    for (int e = 0; e < PX; ++e) {
                        const int sx = xmap[x0 + e];
                        if (sx < 0) continue;
                        if ((sx >> 6) != cur) { cur = sx >> 6; word = row[cur]; }
                        m |= (unsigned)((word >> (sx & 63)) & 1ull) << e;
                    }
                } else {
                    const unsigned char* row = (const unsigned char*)im.masks + j * im.ld + (long)sy * im.w;
#pragma unroll
                    for (int e = 0; e < PX; ++e) {
                        const int sx = xmap[x0 + e];
                        if (sx >= 0 && row[sx] != 0) m |= 1u << e;
                    }
                }
            }
            // 4 bits -> 4 bytes of 0 / 1: bit b of the nibble lands on bit 8 b of the product
            unsigned char* o = out + (long)k * H * W + (long)y * W + x0;
            if (PX == 16) {
                uint4 v;
                v.x = ((m & 15u) * 0x00204081u) & 0x01010101u;
                v.y = (((m >> 4) & 15u) * 0x00204081u) & 0x01010101u;
                v.z = (((m >> 8) & 15u) * 0x00204081u) & 0x01010101u;
                v.w = (((m >> 12) & 15u) * 0x00204081u) & 0x01010101u;
                *reinterpret_cast<uint4*>(o) = v;
            } else {
                *reinterpret_cast<unsigned*>(o) = ((m & 15u) * 0x00204081u) & 0x01010101u;
            }
            if (m) {
#pragma unroll
                for (int l = 0; l < 4; ++l) {
                    if (y & ((1 << l) - 1)) continue;
                    // bits e of the lane with (x0 + e) a multiple of 2^l (x0 is a multiple of PX)
                    unsigned pat = l == 0 ? 0xffffu : l == 1 ? 0x5555u : l == 2 ? 0x1111u : ((x0 & 7) ? 0u : 0x0101u);
                    const unsigned mm = m & pat & ((1u << PX) - 1u);
                    if (!mm) continue;
                    const int lo = (x0 + __builtin_ctz(mm)) >> l, hi = (x0 + 31 - __builtin_clz(mm)) >> l, ys = y >> l;
                    atomicMax(&sbox[4 * l + 0], 0x10000 - ys);
                    atomicMax(&sbox[4 * l + 1], 0x10000 - lo);
                    atomicMax(&sbox[4 * l + 2], ys + 1);
                    atomicMax(&sbox[4 * l + 3], hi + 1);
                }
            }
        }
        __syncthreads();
        if (threadIdx.x < 16 && sbox[threadIdx.x]) atomicMax(&box[(long)k * 16 + threadIdx.x], sbox[threadIdx.x]);
    }
}

// imgs: device SpImage [N]; inst_img: device int32 [ntot] = image of every instance (instances of image i are inst0 .. inst0 + n - 1);
// out: device bytes [ntot][H][W] of 0 / 1 (transforms.py:165-176 after :86-162); box: device int32 [ntot][16], ZERO-FILLED by the caller.
extern "C" int kg_sp_warp_masks(const void* imgs, const int* inst_img, int ntot, int H, int W, void* out, int* box, void* stream) {
    KG_CHECK_ARG(ntot >= 0 && (ntot == 0 || (imgs && inst_img && out && box)), "kg_sp_warp_masks: bad arguments");
    KG_CHECK_ARG(H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0 && H <= 65535 && W <= SP_MAXW, "kg_sp_warp_masks: output %d x %d must be multiples of 8, W <= %d",
                 H, W, SP_MAXW);
    if (ntot == 0) return KG_OK;
    const unsigned gy = (unsigned)(ntot < 65535 ? ntot : 65535);
    if (W % 16 == 0)
        hipLaunchKernelGGL(sp_warp_kernel<16>, dim3((unsigned)kg_cdiv((long)H * (W / 16), 256), gy), dim3(256), 0, (hipStream_t)stream,
                           (const SpImage*)imgs, inst_img, ntot, H, W, (unsigned char*)out, box);
    else
        hipLaunchKernelGGL(sp_warp_kernel<4>, dim3((unsigned)kg_cdiv((long)H * (W / 4), 256), gy), dim3(256), 0, (hipStream_t)stream,
                           (const SpImage*)imgs, inst_img, ntot, H, W, (unsigned char*)out, box);
    KG_CHECK_LAUNCH("sp_warp_masks");
    return KG_OK;
}

// ---- label maps -------------------------------------------------------------------------------------------------------------------
// The mask kernel's lane: PX bits of one output row -> ONE dword (PX 4) or dwordx4 (PX 16) of 0 / 1 bytes
template <int PX>
__device__ __forceinline__ void sp_store_bits(unsigned char* o, unsigned m) {
    if (PX == 16) {
        uint4 v;
        v.x = ((m & 15u) * 0x00204081u) & 0x01010101u;
        v.y = (((m >> 4) & 15u) * 0x00204081u) & 0x01010101u;
        v.z = (((m >> 8) & 15u) * 0x00204081u) & 0x01010101u;
        v.w = (((m >> 12) & 15u) * 0x00204081u) & 0x01010101u;
        *reinterpret_cast<uint4*>(o) = v;
    } else {
        *reinterpret_cast<unsigned*>(o) = ((m & 15u) * 0x00204081u) & 0x01010101u;
    }
}
// ... and its fold of the lane's ones (m != 0) into the workgroup's LDS box at the four divide scales, in kg_sp_warp_masks' encoding
template <int PX>
__device__ __forceinline__ void sp_fold_bits(int* sbox, unsigned m, int y, int x0) {
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        if (y & ((1 << l) - 1)) continue;
        const unsigned pat = l == 0 ? 0xffffu : l == 1 ? 0x5555u : l == 2 ? 0x1111u : ((x0 & 7) ? 0u : 0x0101u);
        const unsigned mm = m & pat & ((1u << PX) - 1u);
        if (!mm) continue;
        const int lo = (x0 + __builtin_ctz(mm)) >> l, hi = (x0 + 31 - __builtin_clz(mm)) >> l, ys = y >> l;
        atomicMax(&sbox[4 * l + 0], 0x10000 - ys);
        atomicMax(&sbox[4 * l + 1], 0x10000 - lo);
        atomicMax(&sbox[4 * l + 2], ys + 1);
        atomicMax(&sbox[4 * l + 3], hi + 1);
    }
}

// The mask kernel's shape (a workgroup = one job x 256 pixel groups, a lane = PX adjacent pixels of one output row), reading
// labels[sy][sx] == id in place of a mask plane.  Output pixel (y, x) of job k is 1 iff (unsigned)img < (unsigned)N, sy and sx lie inside
// the paste window, (sy, sx) lies inside the job box clamped to [0, h] x [0, w], and labels[sy][sx] == id; otherwise 0.
// The box makes most of the output a plain fill: a lane loads only when its row lies in the box's rows, and there only the pixels whose
// column lies in the box's columns.  A workgroup none of whose rows meets the box (a workgroup-uniform vote) stores its zeros and skips
// the column map, the fold and the atomics.  (A workgroup visits a second job only beyond 65 535 jobs, so keeping the column map between
// the jobs of one image would save nothing at any measured size: it is rebuilt per job, as in the mask kernel.)
template <int PX>
__global__ __launch_bounds__(256) void sp_warp_labels_kernel(const SpImage* __restrict__ imgs, int N, const int* __restrict__ jobs, int ntot, int H, int W,
                                                             unsigned char* __restrict__ out, int* __restrict__ box) {
    __shared__ int xmap[SP_MAXW];
    __shared__ int sbox[16];
    const int gpr = W / PX, ngroups = H * gpr;
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int y = g / gpr, x0 = (g - y * gpr) * PX;
    for (int k = blockIdx.y; k < ntot; k += gridDim.y) {
        const int* jb = jobs + (long)k * 6;
        const int img = jb[0], id = jb[1];
        const bool live = (unsigned)img < (unsigned)N;                               // the only place img may become an index
        const int ii = live ? img : 0;
        const SpImage im = imgs[ii];
        const KgBox b = kg_job_box(jb + 2, im.h, im.w);
        const bool open = live && (im.flags & SP_LABELS) && im.masks != nullptr;     // (a record that is no label map gives zeros)
        int sy = -1;
        if (open && g < ngroups) {
            sy = sp_src(y, im.h, im.He, im.oy, im.flags & SP_MIRROR_H, H);
            if ((unsigned)(sy - b.y1) >= (unsigned)b.h) sy = -1;                     // outside the window (-1) or outside the box's rows
        }
        // (also the barrier between the previous job's reads of xmap / sbox and the writes below)
        const int any = __syncthreads_or(sy >= 0 && b.w > 0);
        unsigned m = 0;
        if (any) {
            for (int x = threadIdx.x; x < W; x += 256) xmap[x] = sp_src(x, im.w, im.We, im.ox, im.flags & SP_MIRROR_W, W);
            if (threadIdx.x < 16) sbox[threadIdx.x] = 0;
            __syncthreads();
            if (sy >= 0) {
                const int* row = (const int*)im.masks + (long)sy * im.w;
#pragma unroll
                for (int e = 0; e < PX; ++e) {
                    const int sx = xmap[x0 + e];
                    if ((unsigned)(sx - b.x1) < (unsigned)b.w && row[sx] == id) m |= 1u << e;    // sx = -1 fails: b.x1 >= 0
                }
            }
        }
        if (g < ngroups) sp_store_bits<PX>(out + (long)k * H * W + (long)y * W + x0, m);
        if (any) {
            if (m) sp_fold_bits<PX>(sbox, m, y, x0);
            __syncthreads();
            if (threadIdx.x < 16 && sbox[threadIdx.x]) atomicMax(&box[(long)k * 16 + threadIdx.x], sbox[threadIdx.x]);
        }
    }
}

// imgs: device SpImage [N], label-map images (SP_LABELS: masks = int32 [h][w]); jobs: device int32 [ntot][6] = (img, id, y1, x1, y2, x2),
// the box half-open in source coordinates, rows inst0 .. inst0 + n - 1 those of image img; out: device bytes [ntot][H][W] of 0 / 1;
// box: device int32 [ntot][16], ZERO-FILLED by the caller, kg_sp_warp_masks' encoding.  One launch; every output element is written.
// Every index is a long: ntot * H * W < 2^31 * 2^16 * 2^12 and ntot * 16 fit it whatever the arguments.
extern "C" int kg_sp_warp_labels(const void* imgs, int N, const int* jobs, int ntot, int H, int W, void* out, int* box, void* stream) {
    const char* fn = "kg_sp_warp_labels";
    KG_CHECK_ARG(N >= 1 && N <= 65535, "%s: N %d (1 .. 65535)", fn, N);
    KG_CHECK_ARG(ntot >= 0, "%s: bad size (ntot %d)", fn, ntot);
    KG_CHECK_ARG(H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0 && H <= 65535 && W <= SP_MAXW, "%s: output %d x %d must be multiples of 8, H <= 65535, W <= %d", fn,
                 H, W, SP_MAXW);
    KG_CHECK_ARG((long)ntot <= LONG_MAX / ((long)H * W) && (long)ntot <= LONG_MAX / 64, "%s: ntot * H * W exceeds the index type", fn);
    if (ntot == 0) return KG_OK;
    KG_CHECK_ARG(imgs && jobs && out && box, "%s: null pointer", fn);
    const long obytes = (long)ntot * H * W, bbytes = (long)ntot * 64, jbytes = (long)ntot * 24;
    KG_CHECK_ARG(kg_aligned(imgs, 7) && kg_aligned(jobs, 3) && kg_aligned(box, 3) && kg_aligned(out, W % 16 == 0 ? 15 : 3), "%s: misaligned pointer", fn);
    KG_CHECK_ARG(kg_apart(out, obytes, box, bbytes) && kg_apart(out, obytes, jobs, jbytes) && kg_apart(box, bbytes, jobs, jbytes) &&
                     kg_apart(out, obytes, imgs, (long)N * 80) && kg_apart(box, bbytes, imgs, (long)N * 80),
                 "%s: an output overlaps an input or the other output", fn);
    const unsigned gy = (unsigned)(ntot < 65535 ? ntot : 65535);
    if (W % 16 == 0)
        hipLaunchKernelGGL(sp_warp_labels_kernel<16>, dim3((unsigned)kg_cdiv((long)H * (W / 16), 256), gy), dim3(256), 0, (hipStream_t)stream,
                           (const SpImage*)imgs, N, jobs, ntot, H, W, (unsigned char*)out, box);
    else
        hipLaunchKernelGGL(sp_warp_labels_kernel<4>, dim3((unsigned)kg_cdiv((long)H * (W / 4), 256), gy), dim3(256), 0, (hipStream_t)stream,
                           (const SpImage*)imgs, N, jobs, ntot, H, W, (unsigned char*)out, box);
    KG_CHECK_LAUNCH("sp_warp_labels");
    return KG_OK;
}

// out[i][y][x] = labels_i[sy][sx] inside the paste window, 0 outside (and 0 for a record that is no label map).  One lane: 4 adjacent
// pixels of one row, one 16-byte store.  The labels are stored values only; every address comes from sp_src.
__global__ __launch_bounds__(256) void sp_warp_labelmap_kernel(const SpImage* __restrict__ imgs, int H, int W, int* __restrict__ out) {
    const int q = blockIdx.x * 256 + threadIdx.x, qpr = W >> 2;
    if (q >= H * qpr) return;
    const int y = q / qpr, x0 = (q - y * qpr) << 2;
    const SpImage im = imgs[blockIdx.y];
    int v[4] = {0, 0, 0, 0};
    if ((im.flags & SP_LABELS) && im.masks != nullptr) {
        const int sy = sp_src(y, im.h, im.He, im.oy, im.flags & SP_MIRROR_H, H);
        if (sy >= 0) {
            const int* row = (const int*)im.masks + (long)sy * im.w;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int sx = sp_src(x0 + e, im.w, im.We, im.ox, im.flags & SP_MIRROR_W, W);
                if (sx >= 0) v[e] = row[sx];
            }
        }
    }
    *reinterpret_cast<int4*>(out + ((long)blockIdx.y * H + y) * W + x0) = make_int4(v[0], v[1], v[2], v[3]);
}

// imgs: device SpImage [N], label-map images; out: device int32 [N][H][W], the nearest resize of the expanded, mirrored label maps.
extern "C" int kg_sp_warp_labelmap(const void* imgs, int N, int H, int W, int* out, void* stream) {
    const char* fn = "kg_sp_warp_labelmap";
    KG_CHECK_ARG(N >= 1 && N <= 65535, "%s: N %d (1 .. 65535)", fn, N);
    KG_CHECK_ARG(H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0 && H <= 65535 && W <= SP_MAXW, "%s: output %d x %d must be multiples of 8, H <= 65535, W <= %d", fn,
                 H, W, SP_MAXW);
    KG_CHECK_ARG(imgs && out, "%s: null pointer", fn);
    KG_CHECK_ARG(kg_aligned(imgs, 7) && kg_aligned(out, 15), "%s: misaligned pointer", fn);
    KG_CHECK_ARG(kg_apart(out, (long)N * H * W * 4, imgs, (long)N * 80), "%s: the output overlaps the image table", fn);
    hipLaunchKernelGGL(sp_warp_labelmap_kernel, dim3((unsigned)kg_cdiv((long)H * (W >> 2), 256), (unsigned)N), dim3(256), 0, (hipStream_t)stream,
                       (const SpImage*)imgs, H, W, out);
    KG_CHECK_LAUNCH("sp_warp_labelmap");
    return KG_OK;
}

// ---- boxes ------------------------------------------------------------------------------------------------------------------------
// One workgroup per image turns the instance boxes into the five ordered lists of the sample: lists 0..3 = the keypoints of divide
// scales 1, 2, 4, 8 (dataset_base.py:72-78: kept iff y2 - y1 > 2 R + 1 and x2 - x1 > 2 R + 1), list 4 = gt_bboxes of
// load_gt_masks_bboxes (dataset_base.py:53-55: |y2 - y1| > 2 and |x2 - x1| > 2 at full scale).  Compaction keeps instance order
// (ballot prefix inside a wave, wave totals across the workgroup, a running base across chunks of 256 instances).
__global__ __launch_bounds__(256) void sp_boxes_kernel(const SpImage* __restrict__ imgs, const int* __restrict__ box, int ntot, int radius,
                                                       int* __restrict__ counts, float* __restrict__ gtb, float* __restrict__ kp,
                                                       int* __restrict__ keep) {
    __shared__ int wtot[4];
    const SpImage im = imgs[blockIdx.x];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int list = 0; list < 5; ++list) {
        const int l = list < 4 ? list : 0, lim = list < 4 ? 2 * radius + 1 : 2;
        int running = 0;
        for (int j0 = 0; j0 < im.n; j0 += 256) {
            const int j = j0 + threadIdx.x;
            int y1 = 0, x1 = 0, y2 = 0, x2 = 0;
            bool flag = false;
            if (j < im.n) {
                const int* b = box + (long)(im.inst0 + j) * 16 + 4 * l;
                if (b[0]) {
                    y1 = 0x10000 - b[0]; x1 = 0x10000 - b[1]; y2 = b[2] - 1; x2 = b[3] - 1;
                    flag = y2 - y1 > lim && x2 - x1 > lim;
                }
            }
            const unsigned long long bal = __ballot(flag);
            if (lane == 0) wtot[wv] = __popcll(bal);
            __syncthreads();
            int pos = running + __popcll(bal & ((1ull << lane) - 1ull));
            for (int q = 0; q < wv; ++q) pos += wtot[q];
            running += wtot[0] + wtot[1] + wtot[2] + wtot[3];
            __syncthreads();
            if (!flag) continue;
            if (list < 4) {
                float* o = kp + ((long)l * ntot + im.inst0 + pos) * 10;                    // tl, tr, bl, br, cc as (x, y)
                const float fx1 = (float)x1, fy1 = (float)y1, fx2 = (float)x2, fy2 = (float)y2;
                o[0] = fx1; o[1] = fy1; o[2] = fx2; o[3] = fy1; o[4] = fx1; o[5] = fy2; o[6] = fx2; o[7] = fy2;
                o[8] = (float)((double)(x1 + x2) / 2.0); o[9] = (float)((double)(y1 + y2) / 2.0);
            } else {
                float* o = gtb + (long)(im.inst0 + pos) * 5;
                o[0] = (float)y1; o[1] = (float)x1; o[2] = (float)y2; o[3] = (float)x2; o[4] = 1.f;
                keep[im.inst0 + pos] = j;
            }
        }
        if (threadIdx.x == 0) counts[blockIdx.x * 5 + list] = running;
    }
}

// box: kg_sp_warp_masks' boxes; counts: device int32 [N][5]; gtb: device float32 [ntot][5] (y1, x1, y2, x2, 1); kp: device float32
// [4][ntot][5][2]; keep: device int32 [ntot] (instance of the image behind every gtb row).  The lists of image i start at row inst0 of
// their table and hold counts[i][list] rows.
extern "C" int kg_sp_boxes(const void* imgs, int N, const int* box, int ntot, int kp_radius, int* counts, float* gtb, float* kp, int* keep,
                           void* stream) {
    KG_CHECK_ARG(imgs && counts && N > 0 && ntot >= 0 && kp_radius >= 0 && (ntot == 0 || (box && gtb && kp && keep)), "kg_sp_boxes: bad arguments");
    hipLaunchKernelGGL(sp_boxes_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, (const SpImage*)imgs, box, ntot, kp_radius, counts, gtb,
                       kp, keep);
    KG_CHECK_LAUNCH("sp_boxes");
    return KG_OK;
}
