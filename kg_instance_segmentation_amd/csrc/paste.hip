// paste.hip -- mask paste-back of the inference driver on gfx950.
// Reference: test.py:127-157 (`post_processing`): per detection cv2.resize(patch, (x2-x1, y2-y1)) -> paste into a zero
// (input_h, input_w) mask -> cv2.resize(mask, (image_w, image_h)) -> mask >= seg_thresh.  The reference builds every full-size
// mask on the host (two OpenCV resizes + a 1 MB array per detection); here one thread per output pixel evaluates the same
// two-stage bilinear expression directly from the patch probabilities that forward_seg left in HBM.
// Interpolation rule = the published generic INTER_LINEAR float path of OpenCV's resize.cpp (oracle/paste.py states it and why
// it is "parity unpinned": cv2 is absent here); compiled with -ffp-contract=off so that every product and sum rounds as written
// (horizontal pass first, float32).  HBM-bound: algorithmic bytes = the nd * image_h * image_w output bytes.
#include "label_common.h"        // kg_bits_ld, kg_check_bits_ld
#include "lin_taps.h"
#include <math.h>

struct PasteDet { int off, ph, pw, y1, x1, y2, x2, pad; };

// value of the patch resized to (bh, bw) at (ry, rx)
__device__ __forceinline__ float resized_patch(const float* __restrict__ p, int ph, int pw, int bh, int bw, int ry, int rx) {
    if (ph == bh && pw == bw) return p[ry * pw + rx];
    const Taps ty = lin_taps(ry, ph, bh, false), tx = lin_taps(rx, pw, bw, true);
    const float r0 = lin_row(p[ty.s0 * pw + tx.s0], p[ty.s0 * pw + tx.s1], tx);
    const float r1 = lin_row(p[ty.s1 * pw + tx.s0], p[ty.s1 * pw + tx.s1], tx);
    const float a = r0 * ty.c0, b = r1 * ty.c1;
    return a + b;
}
__device__ __forceinline__ float pasted(const float* __restrict__ p, const PasteDet& d, int y, int x) {
    if (y < d.y1 || y >= d.y2 || x < d.x1 || x >= d.x2) return 0.f;
    return resized_patch(p, d.ph, d.pw, d.y2 - d.y1, d.x2 - d.x1, y - d.y1, x - d.x1);
}

template <typename OUT>
__global__ __launch_bounds__(256) void paste_kernel(const float* __restrict__ flat, const PasteDet* __restrict__ dets, int nd, int in_h, int in_w,
                                                    int out_h, int out_w, float thresh, OUT* __restrict__ out) {
    const long per = (long)out_h * out_w, total = per * nd;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int k = (int)(i / per);
        const int rem = (int)(i - (long)k * per);
        const int oy = rem / out_w, ox = rem - oy * out_w;
        const PasteDet d = dets[k];
        const float* p = flat + d.off;
        float v;
        if (d.y2 <= d.y1 || d.x2 <= d.x1) v = 0.f;
        else if (in_h == out_h && in_w == out_w) v = pasted(p, d, oy, ox);
        else {
            const Taps ty = lin_taps(oy, in_h, out_h, false), tx = lin_taps(ox, in_w, out_w, true);
            if (ty.s1 < d.y1 || ty.s0 >= d.y2 || tx.s1 < d.x1 || tx.s0 >= d.x2) v = 0.f;
            else {
                const float r0 = lin_row(pasted(p, d, ty.s0, tx.s0), pasted(p, d, ty.s0, tx.s1), tx);
                const float r1 = lin_row(pasted(p, d, ty.s1, tx.s0), pasted(p, d, ty.s1, tx.s1), tx);
                const float a = r0 * ty.c0, b = r1 * ty.c1;
                v = a + b;
            }
        }
        out[i] = (OUT)(v >= thresh ? 1 : 0);
    }
}

// flat: fp32 patch probabilities (forward_seg's output buffer); dets: device int32 [nd][8] = {patch offset, patch h, patch w,
// y1, x1, y2, x2, 0} with the box already rounded / clamped as test.py:138-141; out: [nd][image_h][image_w], float32 (as the
// reference returns) when out_is_u8 == 0, bytes otherwise.
extern "C" int kg_mask_paste(const float* flat, const int* dets, int nd, int input_h, int input_w, int image_h, int image_w,
                             float seg_thresh, void* out, int out_is_u8, void* stream) {
    KG_CHECK_ARG(flat && dets && out && nd >= 0 && input_h > 0 && input_w > 0 && image_h > 0 && image_w > 0, "kg_mask_paste: bad arguments");
    if (nd == 0) return KG_OK;
    const long total = (long)nd * image_h * image_w;
    long blocks = (total + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    if (out_is_u8)
        hipLaunchKernelGGL(paste_kernel<unsigned char>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, flat, (const PasteDet*)dets, nd,
                           input_h, input_w, image_h, image_w, seg_thresh, (unsigned char*)out);
    else
        hipLaunchKernelGGL(paste_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, flat, (const PasteDet*)dets, nd,
                           input_h, input_w, image_h, image_w, seg_thresh, (float*)out);
    KG_CHECK_LAUNCH("mask_paste");
    return KG_OK;
}

// ---- bit-packed masks (include/kgnet_hip.h "bit-mask layout") ---------------------------------------------------------------------
// One mask = ld_words 64-bit words: row y takes wpr = ceil(W / 64) words, bit b of word k of row y is pixel (y, 64 k + b), bits at
// x >= W and the words from H * wpr on are zero.  A wave owns words: lane b evaluates pixel 64 k + b, __ballot forms the word, lane 0
// stores it (a vector store).  Every block is 4 waves, every wave walks KG_BITS_WPW consecutive words of one mask.
#define KG_BITS_WPW 8
static inline dim3 kg_bits_grid(int n, long ld_words) {
    return dim3((unsigned)((ld_words + 4 * KG_BITS_WPW - 1) / (4 * KG_BITS_WPW)), (unsigned)(n < 65535 ? n : 65535));
}

// kg_mask_paste with the thresholded pixels written as bits.  Per pixel the expression is paste_kernel's own (lin_taps / pasted /
// resized_patch above, same -ffp-contract=off translation unit).  A word whose 64-pixel span cannot reach the box skips the taps: the
// source taps s0 / s1 of lin_taps never decrease with the destination index, so paste_kernel's rejection test on the span's two ends
// (tx.s1 of the last pixel < x1, or tx.s0 of the first >= x2; the row test is the pixel's own) holds for every pixel between them.
// Such a pixel's value is 0, which is still compared with the threshold (seg_thresh <= 0 makes it foreground, as in paste_kernel).
__global__ __launch_bounds__(256) void paste_bits_kernel(const float* __restrict__ flat, const PasteDet* __restrict__ dets, int nd, int in_h, int in_w,
                                                         int out_h, int out_w, float thresh, unsigned long long* __restrict__ words, long ld_words) {
    const int lane = threadIdx.x & 63, wpr = (out_w + 63) >> 6;
    const long nw = (long)out_h * wpr;
    const long r0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * KG_BITS_WPW;
    const bool same = in_h == out_h && in_w == out_w;
    for (int k = blockIdx.y; k < nd; k += gridDim.y) {
        const PasteDet d = dets[k];
        const float* p = flat + d.off;
        const bool empty = d.y2 <= d.y1 || d.x2 <= d.x1;
        int oy = (int)(r0 / wpr), kw = (int)(r0 - (long)oy * wpr), ty_row = -1;
        Taps ty = {};
        bool row_skip = true;
        for (long r = r0; r < r0 + KG_BITS_WPW && r < ld_words; ++r) {
            unsigned long long word = 0;
            if (r < nw) {
                const int xa = kw << 6, xb = xa + 63 < out_w ? xa + 63 : out_w - 1, ox = xa + lane;
                float v = 0.f;
                if (empty) {
                } else if (same) {
                    if (!(oy < d.y1 || oy >= d.y2 || xb < d.x1 || xa >= d.x2) && ox < out_w) v = pasted(p, d, oy, ox);
                } else {
                    if (ty_row != oy) {
                        ty = lin_taps(oy, in_h, out_h, false);
                        row_skip = ty.s1 < d.y1 || ty.s0 >= d.y2;
                        ty_row = oy;
                    }
                    bool skip = row_skip;
                    if (!skip) skip = lin_taps(xb, in_w, out_w, true).s1 < d.x1 || lin_taps(xa, in_w, out_w, true).s0 >= d.x2;
                    if (!skip && ox < out_w) {
                        const Taps tx = lin_taps(ox, in_w, out_w, true);
                        if (!(tx.s1 < d.x1 || tx.s0 >= d.x2)) {
                            const float r0v = lin_row(pasted(p, d, ty.s0, tx.s0), pasted(p, d, ty.s0, tx.s1), tx);
                            const float r1v = lin_row(pasted(p, d, ty.s1, tx.s0), pasted(p, d, ty.s1, tx.s1), tx);
                            const float a = r0v * ty.c0, b = r1v * ty.c1;
                            v = a + b;
                        }
                    }
                }
                word = __ballot(ox < out_w && v >= thresh);
                if (++kw == wpr) { kw = 0; ++oy; }
            }
            if (lane == 0) words[(long)k * ld_words + r] = word;
        }
    }
}

// words: device 64-bit words [nd][ld_words], ld_words even and >= kg_mask_bits_ld(image_h, image_w); the other arguments as kg_mask_paste
extern "C" int kg_mask_paste_bits(const float* flat, const int* dets, int nd, int input_h, int input_w, int image_h, int image_w,
                                  float seg_thresh, void* words, long ld_words, void* stream) {
    KG_CHECK_ARG(flat && dets && words, "kg_mask_paste_bits: null pointer");
    KG_CHECK_ARG(nd >= 0 && input_h > 0 && input_w > 0 && image_h > 0 && image_w > 0, "kg_mask_paste_bits: bad size");
    KG_TRY(kg_check_bits_ld("kg_mask_paste_bits", image_h, image_w, ld_words));
    if (nd == 0) return KG_OK;
    hipLaunchKernelGGL(paste_bits_kernel, kg_bits_grid(nd, ld_words), dim3(256), 0, (hipStream_t)stream, flat, (const PasteDet*)dets, nd, input_h,
                       input_w, image_h, image_w, seg_thresh, (unsigned long long*)words, ld_words);
    KG_CHECK_LAUNCH("mask_paste_bits");
    return KG_OK;
}

// dense [n][H][W] (bytes or float32, any non-zero value = foreground) -> words
template <typename IN>
__global__ __launch_bounds__(256) void pack_bits_kernel(const IN* __restrict__ m, int n, int H, int W, unsigned long long* __restrict__ words,
                                                        long ld_words) {
    const int lane = threadIdx.x & 63, wpr = (W + 63) >> 6;
    const long nw = (long)H * wpr;
    const long r0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * KG_BITS_WPW;
    for (int k = blockIdx.y; k < n; k += gridDim.y) {
        const IN* src = m + (long)k * H * W;
        for (long r = r0; r < r0 + KG_BITS_WPW && r < ld_words; ++r) {
            unsigned long long word = 0;
            if (r < nw) {
                const int y = (int)(r / wpr), x = ((int)(r - (long)y * wpr) << 6) + lane;
                word = __ballot(x < W && src[(long)y * W + x] != (IN)0);
            }
            if (lane == 0) words[(long)k * ld_words + r] = word;
        }
    }
}
// words -> dense [n][H][W] of 0 / 1 (bytes or float32)
template <typename OUT>
__global__ __launch_bounds__(256) void unpack_bits_kernel(const unsigned long long* __restrict__ words, long ld_words, int n, int H, int W,
                                                          OUT* __restrict__ out) {
    const int lane = threadIdx.x & 63, wpr = (W + 63) >> 6;
    const long nw = (long)H * wpr;
    const long r0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * KG_BITS_WPW;
    for (int k = blockIdx.y; k < n; k += gridDim.y) {
        OUT* dst = out + (long)k * H * W;
        for (long r = r0; r < r0 + KG_BITS_WPW && r < nw; ++r) {
            const int y = (int)(r / wpr), x = ((int)(r - (long)y * wpr) << 6) + lane;
            const unsigned long long word = words[(long)k * ld_words + r];
            if (x < W) dst[(long)y * W + x] = (OUT)((word >> lane) & 1ull);
        }
    }
}

// ld_words of an H x W mask (host helper); -1 on bad arguments
extern "C" long kg_mask_bits_ld(int H, int W) {
    if (H <= 0 || W <= 0) {
        kg_set_error("kg_mask_bits_ld: bad size %d x %d", H, W);
        return -1;
    }
    return kg_bits_ld(H, W);
}
// masks: device [n][H][W], float32 (src_is_f32 != 0) or bytes; words: device [n][ld_words]
extern "C" int kg_mask_pack_bits(const void* masks, int src_is_f32, int n, int H, int W, void* words, long ld_words, void* stream) {
    KG_CHECK_ARG(masks && words, "kg_mask_pack_bits: null pointer");
    KG_CHECK_ARG(n > 0 && H > 0 && W > 0, "kg_mask_pack_bits: bad size");
    KG_TRY(kg_check_bits_ld("kg_mask_pack_bits", H, W, ld_words));
    if (src_is_f32)
        hipLaunchKernelGGL(pack_bits_kernel<float>, kg_bits_grid(n, ld_words), dim3(256), 0, (hipStream_t)stream, (const float*)masks, n, H, W,
                           (unsigned long long*)words, ld_words);
    else
        hipLaunchKernelGGL(pack_bits_kernel<unsigned char>, kg_bits_grid(n, ld_words), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)masks,
                           n, H, W, (unsigned long long*)words, ld_words);
    KG_CHECK_LAUNCH("mask_pack_bits");
    return KG_OK;
}
// out: device [n][H][W] of 0 / 1, bytes (out_is_u8 != 0) or float32
extern "C" int kg_mask_unpack_bits(const void* words, long ld_words, int n, int H, int W, void* out, int out_is_u8, void* stream) {
    KG_CHECK_ARG(words && out, "kg_mask_unpack_bits: null pointer");
    KG_CHECK_ARG(n > 0 && H > 0 && W > 0, "kg_mask_unpack_bits: bad size");
    KG_TRY(kg_check_bits_ld("kg_mask_unpack_bits", H, W, ld_words));
    if (out_is_u8)
        hipLaunchKernelGGL(unpack_bits_kernel<unsigned char>, kg_bits_grid(n, ld_words), dim3(256), 0, (hipStream_t)stream,
                           (const unsigned long long*)words, ld_words, n, H, W, (unsigned char*)out);
    else
        hipLaunchKernelGGL(unpack_bits_kernel<float>, kg_bits_grid(n, ld_words), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)words,
                           ld_words, n, H, W, (float*)out);
    KG_CHECK_LAUNCH("mask_unpack_bits");
    return KG_OK;
}

// ---- SEG_loss target preparation on the device (second half: seg_loss.py:57-80) ---------------------------------------
// For callers whose ground-truth masks are device-resident (float32 [n_i][H][W] tensors on the GPU): the crop of the matched mask
// [y1:y2, x1:x2] nearest-resized to the predicted patch (h1, w1) -- cv2.resize(..., INTER_NEAREST) as restated by kg_host_crop_masks:
// src = min(floor(dst * src_size / dst_size), src_size - 1), identity when the sizes agree -- written as bytes at the pair's offset of
// the target buffer kg_seg_loss reads.  One workgroup per (pair, 1024-pixel slab); the same work rows as the host function.
__global__ __launch_bounds__(256) void crop_masks_kernel(const float* const* __restrict__ masks, const int* __restrict__ work, int nwork,
                                                         int H, int W, unsigned char* __restrict__ out) {
    const int k = blockIdx.x;
    const int* w = work + 9 * k;
    const float* m = masks[w[0]] + (long)w[1] * H * W;
    const int ya = w[2], xa = w[4];
    int yb = w[3], xb = w[5];
    const int h1 = w[6], w1 = w[7];
    if (yb > H) yb = H;
    if (xb > W) xb = W;
    const int h0 = yb - ya, w0 = xb - xa;
    if (h0 <= 0 || w0 <= 0) return;          // (rejected on the host before the launch)
    const bool same = h0 == h1 && w0 == w1;
    const double fy = (double)h0 / h1, fx = (double)w0 / w1;
    unsigned char* o = out + w[8];
    for (int i = blockIdx.y * 256 + threadIdx.x; i < h1 * w1; i += gridDim.y * 256) {
        const int y = i / w1, x = i - y * w1;
        int sy = y, sx = x;
        if (!same) {
            sy = (int)floor(y * fy); if (sy > h0 - 1) sy = h0 - 1;
            sx = (int)floor(x * fx); if (sx > w0 - 1) sx = w0 - 1;
        }
        o[i] = (unsigned char)m[(long)(ya + sy) * W + xa + sx];
    }
}
// masks: DEVICE array of nimg device pointers (float32 [n_i][H][W]); work: device int32 [nwork][9] rows (img, gt index, y1, y2, x1, x2,
// h1, w1, out offset) -- the rows kg_host_crop_masks takes; out: device bytes.
extern "C" int kg_crop_masks(const void* masks, const int* work, int nwork, int H, int W, void* out, void* stream) {
    KG_CHECK_ARG(masks && work && out && nwork >= 0 && H > 0 && W > 0, "kg_crop_masks: bad arguments");
    if (nwork == 0) return KG_OK;
    hipLaunchKernelGGL(crop_masks_kernel, dim3(nwork, 4), dim3(256), 0, (hipStream_t)stream, (const float* const*)masks, work, nwork, H, W,
                       (unsigned char*)out);
    KG_CHECK_LAUNCH("crop_masks");
    return KG_OK;
}
