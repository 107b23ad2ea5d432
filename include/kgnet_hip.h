/*
 * kgnet_hip.h -- C ABI of libkgnet_hip.so: the MI355X (gfx950) hot path of KGnet.
 *
 * The reference (yijingru/KG_Instance_Segmentation) has no FFI; its boundary is the Python module
 * surface its drivers import (train.py:3-11, test.py:3-12).  The drop-in Python modules in
 * kg_instance_segmentation_amd/ bind the entry points below with ctypes; every entry point cites the
 * reference code it replaces.  Conventions:
 *   - extern "C", plain pointers and sizes, no torch types.  All pointers are DEVICE pointers unless
 *     stated otherwise; the library never retains a caller's pointer past the call (the recorded weight-gradient reductions between
 *     kg_wgrad_reduce_defer(1) and the flush excepted) and allocates no device memory of its own EXCEPT two per-device scratch buffers,
 *     created on first use and kept for the life of the process: the split-K partial tiles of under-filled conv launches (64 MB) and
 *     the partial maps of split kg_conv2d_halo_heads2 launches (grown to 3 x parts x N x 55 x H x W floats, <= 384 MB).  A launch that
 *     uses one is followed by its finishing launch on the same stream, so conv calls of ONE device must come from one stream at a time.
 *   - every call enqueues on the caller's `stream` (a hipStream_t) and does not synchronise.
 *   - return value: 0 = ok, otherwise kg_last_error() (thread-local) describes the failure.
 *   - activations ("rows"): bf16, pixel-major [row][ld] (NHWC), channel counts multiples of 8.
 *   - weights: fp32 OIHW master copies are packed to bf16 [Cout_pad][K] by kg_pack_weight.
 *   - precision: the reference computes in fp32 (KGnet.py:22-29 -> F.conv2d on fp32 tensors).  The fast matrix path of gfx950
 *     is bf16 MFMA with fp32 accumulation, so tensors that must carry more than bf16 are stored as P "planes" of bf16 whose
 *     sum is the value (P = 2: 16 significant bits, P = 3: the fp32 value exactly) and a product of an xP-plane activation
 *     with a wP-plane weight is the sum of the bf16 MFMA products x_i * w_j with i + j < max(xP, wP).  Entry points that
 *     take rows operands accept a `const kg_planes_t* planes` (host struct, NULL = single-plane bf16 everywhere); each
 *     documents which operand uses which slot.
 */
#ifndef KGNET_HIP_H
#define KGNET_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

typedef struct kg_planes {
    int a_planes, a_pstride;   /* first bf16 rows operand: planes, element stride between planes (same row, same ld) */
    int b_planes, b_pstride;   /* second bf16 rows operand */
    int c_planes, c_pstride;   /* third bf16 rows operand */
    int y_planes, y_pstride;   /* output rows */
    int w_planes;              /* planes of the packed weights (virtual-channel layout, see kg_pack_weight) */
    int reserved_;
    const float* scale;        /* device scalar or NULL: kg_grad_pack / kg_f32_to_planes multiply by *scale (kg_grad_scale) */
    const float* oscale;       /* device fp32 [Cout] or NULL: kg_conv2d_igemm / kg_conv2d_halo compute act(acc * oscale[co] + bias[co] (+ res)):
                                  an inference-mode BatchNorm folded into the conv (KGnet.py:82-97 conv -> bn -> relu as one launch;
                                  oscale = gamma / sqrt(running_var + eps), bias = beta - running_mean * oscale), applied to the fp32 accumulator */
} kg_planes_t;

/* The same C ABI is built for two 16-bit storage formats of the rows / packed-weight operands ("bf16 rows" above):
 *   libkgnet_hip.so      bfloat16 (kg_rows_format() == 0);
 *   libkgnet_hip_f16.so  IEEE half (kg_rows_format() == 1): 11 significant bits per plane, so hi + lo planes (22 bits, 3 MFMA
 *                        products per multiply) carry the reference's fp32 tensors where bf16 needs three planes (6 products).
 *                        Packed weights are stored times 2^12 and every conv epilogue scales its fp32 accumulators back; the
 *                        gradients of a backward pass are stored times a power of two chosen on the device (kg_grad_scale).
 * Entry points without rows operands (losses, post-processing, NMS, optimizer, ...) are format-independent and live in
 * libkgnet_hip.so only. */
int kg_rows_format(void);

const char* kg_last_error(void);
/* Measurement aid: the name rocprofv3 prints (without the argument list) for the conv-family kernel that the calling thread's most recent
 * kg_conv2d_* / kg_conv1x1 / kg_conv3x3_c64 / kg_conv2d_wgrad* call launched, e.g. "conv_halo_kernel<7, 1, 8, 0>" ("" before the first).
 * bench.py keys its per-kernel table with it, so that table and the rocprofv3 summaries under profiles/ use the same names. */
const char* kg_last_kernel(void);
int kg_version(void);
int kg_device_arch(char* out, int cap);   /* host buffer */
int kg_tr_probe(void* out_u16x256, void* stream);                       /* test probe: ds_read_b64_tr_b16 lane map */
int kg_f64_probe(const double* a, const double* b, double* out5n, int n, void* stream); /* test probe: fp64 rounding */

/* ---- convolution: torch.nn.Conv2d forward / input-gradient (KGnet.py:22-29, 131-209 -> F.conv2d) ----
 * y[m][co] = act( sum_{tap,ci} x[src(m,tap)][ci] * w[co][tap][ci] + bias[co] + res[m][co] ) (* mask>0)
 * mode 0: dense forward (H,W = input dims, OH,OW = output dims); mode 1: dense transposed = gradient w.r.t.
 * the input of a forward conv (H,W = dY dims, OH,OW = dX dims, weights packed transposed);
 * mode 2/3: the same on a ragged pixel list with per-row descriptors {(y<<16)|x, (h<<16)|w}.
 * y (bf16 rows) and/or y_f32 (fp32 NCHW [N][f32_C][OH*OW]) receive the result.  tile 0 = auto; 1..5 pin an output tile; 6 = split-K over the
 * waves of a 64-pixel x 64-cout tile for launches with too few output tiles to fill the chip (single-image inference: cin_pad % 64 == 0,
 * dense modes, rows output). */
int kg_conv2d_igemm(const void* x, const void* w, const float* bias, void* y, float* y_f32, const void* res,
                    const void* mask, const int* rowdesc, int M, int H, int W, int OH, int OW, int cin_pad, int ldx,
                    int Cout, int ldy, int ldres, int ldmask, int K, int KH, int KW, int stride, int pad, int dil,
                    int mode, int relu, int f32_C, int tile, const kg_planes_t* planes, void* stream);
                    /* planes: a = x, b = res, y = y; cin_pad = channels of ONE x plane */
/* the same convolution for stride 1, "same" padding, KS in {3,7}, cin_pad % 64 == 0: input halo resident in LDS
 * (the 7x7 head convolutions of KGnet.py:161-209 are 86 % of the network's FLOPs).  flip = 1: input gradient. */
int kg_conv2d_halo(const void* x, const void* w, const float* bias, void* y, float* y_f32, const void* res,
                   const void* mask, int N, int H, int W, int cin_pad, int ldx, int Cout, int ldy, int ldres, int ldmask,
                   int K, int KS, int flip, int relu, int f32_C, int wc, const int* tiletab, int ntiles, int total_rows,
                   const kg_planes_t* planes, void* stream);   /* planes: a = x, b = res, y = y.  tiletab != NULL: ragged boxes, one {row0,(h<<16)|w,(oy0<<16)|ox0,0} entry per workgroup */
                   /* wc: couts per workgroup / 64 (0 = default) | 256: the packed weights are zero for channels 32..63 of every chunk | 512 / 1024: the NARROW
                      input gradient (flip = 1, KS = 7, one single-plane 64-channel dY: only channels 0..7 / 8..23 carry data -- the kp / short second-layer
                      heads, KGnet.py:161-209 `.2`): w packed by kg_pack_weight_narrow (7 / 14 virtual taps of 64 columns), 4 / 2 kernel columns per k-step */
/* the three second-layer 7x7 head convolutions of one scale (KGnet.py:161-209 `.2` layers, sigmoid on kp :300) in one launch
 * over the fused hidden rows [N*H*W][>=3C]: w = packed [64 virtual couts][49][3C] (kg_pack_weight_rows), bias64 / vmap[64]
 * indexed by virtual cout (vmap: channel of kp 0-4 | short 5-14 | mid 15-54, or -1); fp32 NCHW outputs */
/* (maps with < 128 (tile, head) workgroups and 3-product inputs: one workgroup per plane product as well, fp32 partial maps in a library
 *  scratch, summed in a fixed order by a second launch -- single-image inference) */
int kg_conv2d_halo_heads2(const void* x, const void* w, const float* bias64, const int* vmap, float* kp, float* sh, float* md,
                          int N, int H, int W, int C, int ldx, int K, int kp_sigmoid, const kg_planes_t* planes, void* stream);   /* kp_sigmoid: 1 = torch.sigmoid on kp as KGnet.py:300, 0 = raw logits.  planes: a = x;
                          w holds [head][virtual planes][C] channels per tap (kg_pack_weight_rows with tap_stride) */
/* 3x3 stride-1 "same" conv / input gradient (flip) for cin_pad == 64 and Cout <= 64 (c0_conv.2, layer1 conv2, seg level 0): persistent
 * workgroups, all 9 taps' weights resident in LDS, the next 16x16 tile's halo fetched by LDS-direct loads during the current tile */
int kg_conv3x3_c64(const void* x, const void* w, const float* bias, void* y, const void* res, const void* mask, int N, int H, int W,
                   int ldx, int Cout, int ldy, int ldres, int ldmask, int K, int flip, int relu, const int* tiletab16, int ntiles,
                   void* stream);
/* 7x7 stride-1 "same" input gradient (flip = 1; 0: forward) of a NARROW conv -- the kp / short second-layer head convs (KGnet.py:161-209 `.2`: C -> 5 / 10):
 * the rows x [N*H*W][ldx] carry data in the chan_slot (8 or 16) channels from chan_lo on; w packed by kg_pack_weight_narrow (7 / 14 virtual taps of 64
 * columns, resident in LDS), persistent workgroups over 16 x 16-pixel tiles with compact double-buffered halos; y rows of Cout channels, zeroed where
 * mask <= 0 (ReLU backward of the hidden tensor; NULL: none).  Single 16-bit planes. */
int kg_conv7_narrow(const void* x, const void* w, void* y, const void* mask, int N, int H, int W, int ldx, int chan_lo, int chan_slot, int Cout, int ldy,
                    int ldmask, int K, int flip, void* stream);
/* Weight-stationary variant for the full-resolution 64 -> 64 channel 3x3 convs of the fp32-tolerance forward pass (c0_conv.2 KGnet.py:139-142,
 * c1_up_conv :153, seg_head.0 :145-147, skip_combine.0.up :116-119): x in hi + lo planes (planes->a_planes == 2), w packed by kg_pack_weight
 * with x_planes = w_planes = 2 (K >= 9 * 192), y = ReLU?(conv + bias) in 1 or 2 planes.  Dense (N images of H x W) or ragged
 * (tiletab8: one {row0, (h << 16) | w, (oy0 << 16) | ox0, 0} entry per 8 x 16 tile of a box). */
int kg_conv3x3_ws(const void* x, const void* w, const float* bias, void* y, int N, int H, int W, int ldx, int ldy, int K, int relu,
                  const int* tiletab8, int ntiles, const kg_planes_t* planes, void* stream);
/* 1x1 stride-1 convolution / its input gradient as a streaming GEMM over rows (dense or ragged): weight slab resident in
 * LDS, pixel fragments straight from global memory, persistent workgroups (KGnet.py:64-99,101-111,155-158) */
int kg_conv1x1(const void* x, const void* w, const float* bias, void* y, const void* res, const void* mask, long M, int K,
               int wK, int ldx, int Cout, int ldy, int ldres, int ldmask, int relu, void* stream);
/* fp32 OIHW parameter -> packed bf16 matrix rows (forward) or its transpose (data gradient).  x_planes / w_planes: split-bf16
 * layout; per tap the row holds one cin_pad-channel copy of weight plane j for every kept product x_i * w_j
 * (i + j < max(x_planes, w_planes)), ordered by descending i + j, then descending j (smallest products first, hi * hi last,
 * so that the fp32 accumulator rounds like the reference's); a conv kernel walks these "virtual channels" like a single-plane
 * conv with more input channels and only remaps the activation side to plane i.  (1, 1) = the plain bf16 matrix. */
int kg_pack_weight(const float* w, void* dst, int Cout, int Cin, int KH, int KW, int K, int cin_pad, int row0, int c0,
                   int transposed, int x_planes, int w_planes, void* stream);
/* forward packing with a row table: packed row of output channel co = rowmap[co] (device int array); tap_stride: channels per
 * tap row when several plane groups share the matrix (0 = vplanes * cin_pad) */
int kg_pack_weight_rows(const float* w, void* dst, int Cout, int Cin, int KH, int KW, int K, int cin_pad, const int* rowmap,
                        int c0, int x_planes, int w_planes, int tap_stride, void* stream);
/* transposed (input-gradient) packing of a narrow conv (Cout <= tap_stride in {8, 16}) for kg_conv2d_halo's wc | 512 / 1024 variants:
 * dst[(row0 + ci) * K + (ky * tap_pitch + kx) * tap_stride + c0 + co] = w[co][ci][ky][kx]; single plane; K >= KH * tap_pitch * tap_stride */
int kg_pack_weight_narrow(const float* w, void* dst, int Cout, int Cin, int KH, int KW, int K, int row0, int c0, int tap_stride, int tap_pitch,
                          void* stream);
/* all (re)packs of a step in one launch: jobs = device array of 80-byte records {const float* w; void* dst; const int* rowmap;
 * int Cout, Cin, taps, K, cin_pad, row0, c0, transposed, gx, blk0, x_planes, w_planes, tap_stride, tap_pitch;} (gx = Cout, or
 * ceil(Cout/64) when transposed; blk0 = first workgroup of the job); total_blocks = sum of gx * gy over the jobs */
int kg_pack_weight_batch(const void* jobs, int njobs, int total_blocks, void* stream);
/* im2col for <= 8 input channels (weight gradient of the stem conv1, KGnet.py:131, as a 1x1 weight-gradient GEMM):
 * out[m][tap * cin + ci] = x[src(m, tap)][ci]; out rows of Kpad >= KH*KW*cin bf16 values, padding columns pre-zeroed */
int kg_im2col_small(const void* x, void* out, int N, int H, int W, int OH, int OW, int KH, int KW, int stride, int pad, int cin,
                    int ldx, int Kpad, void* stream);
/* weight gradient (autograd of nn.Conv2d at train.py:153): partial sums [nsplit][Cout][taps][Cin] fp32 */
int kg_conv2d_wgrad(const void* x, const void* dy, float* dwp, const int* rowdesc, int M, int H, int W, int OH, int OW,
                    int ldx, int lddy, int Cin, int Cout, int cin_lim, int cout_lim, int KH, int KW, int stride, int pad,
                    int dil, int mode, int nsplit, long split_stride, const kg_planes_t* planes, void* stream);
                    /* planes: a = x, b = dy: the kept plane products x_i * dY_j are further passes over the pixels in the same launch */
/* weight gradient of a dense stride-1 "same" 3x3 / 7x7 conv with dY tile + X halo resident in LDS (all taps per staging pass) */
int kg_conv2d_wgrad_halo(const void* x, const void* dy, float* dwp, int N, int H, int W, int ldx, int lddy, int Cin, int Cout,
                         int cin_lim, int cout_lim, int KS, int nsplit, long split_stride, const int* tiletab16, int ntiles,
                         float* dbp, const kg_planes_t* planes, void* stream);   /* planes: a = x, b = dy.  tiletab16 != NULL: ragged boxes, one entry per 16x16 tile;
                         dbp != NULL: also writes the bias-gradient partials [nsplit][Cout] (sum over pixels of dy) */
int kg_bias_grad_final(const float* part, float* db, int nsplit, int C, int accumulate, void* stream);
int kg_wgrad_reduce(const float* part, float* grad_oihw, int Cout, int Cin, int KH, int KW, int nsplit, long split_stride,
                    int accumulate, void* stream);
/* the same for a conv fused along Cout (heads sharing their input): tensor k receives the next counts[k] rows; ngrads <= 4;
   grads / counts are HOST arrays */
int kg_wgrad_reduce_multi(const float* part, float* const* grads_oihw, const int* counts, int ngrads, int Cin, int KH, int KW,
                          int nsplit, long split_stride, int accumulate, void* stream);
/* kg_wgrad_reduce_multi + the bias gradient of the same conv in the same launch: bias_part = the [nsplit][bias_C] partials of
   kg_conv2d_wgrad_halo (dbp), db [bias_C]; bias_part == NULL: weights only */
int kg_wgrad_reduce_bias(const float* part, float* const* grads_oihw, const int* counts, int ngrads, int Cin, int KH, int KW,
                         int nsplit, long split_stride, int accumulate, const float* bias_part, float* db, int bias_C, void* stream);
/* Deferred reductions: between kg_wgrad_reduce_defer(1) and kg_wgrad_reduce_defer(0) the three reduce entry points above only record their
   job (per calling thread; the caller keeps every partial buffer alive and unmodified), kg_wgrad_reduce_flush launches the recorded jobs
   twelve per launch -- each with the block decomposition of its own single launch, so the sums are the same bits.  The reference has no
   counterpart (autograd's conv backward returns finished gradients, train.py:148-154); this only cuts ~70 launches of a few microseconds
   out of a backward pass. */
int kg_wgrad_reduce_defer(int on);
int kg_wgrad_reduce_pending(void);
int kg_wgrad_reduce_flush(void* stream);
int kg_bias_grad(const void* dy, float* db, float* scratch, int scratch_floats, int M, int C, int ld, int accumulate,
                 void* stream);
int kg_set_wgrad_tr(int use_transpose_read);   /* test switch: LDS transpose-read vs scalar fragment loads */

/* ---- backbone glue: image pack, BatchNorm2d (KGnet.py:82-97,132), MaxPool2d (KGnet.py:134), bilinear
 *      F.interpolate(align_corners=False) (KGnet.py:110,288-297), elementwise joins ---- */
/* planes slots of this group: a = first input (x / dy of bilinear_bwd), b = second input (res / dy), y = output; masks use plane 0 */
int kg_img_pack(const float* img_nchw, void* out_rows8, int ldout, int N, int C, int H, int W, const kg_planes_t* planes, void* stream);
int kg_bn_stats_train(const void* x, int ldx, int M, int C, const float* gamma, const float* beta, float* running_mean,
                      float* running_var, float momentum, float eps, float* mean_out, float* invstd_out, float* scale,
                      float* shift, float* scratch, int scratch_floats, const kg_planes_t* planes, void* stream);
/* BatchNorm statistics from the PRODUCING conv's epilogue (the conv of KGnet.py:82-93 that feeds a train-mode BatchNorm2d):
 * kg_conv_stats_begin arms the calling host thread's next kg_conv2d_igemm / kg_conv2d_halo launch (bf16 rows output, no ReLU / residual /
 * mask): that launch also writes per-(pixel tile, channel) {sum, sum of squares} partials of its fp32 accumulators into `part`;
 * kg_conv_stats_end returns the tile count nb (0: the launch used a kernel without this epilogue -- fall back to kg_bn_stats_train) and
 * disarms; kg_bn_finalize_train = the second stage of kg_bn_stats_train over those partials [nb][C][2]. */
int kg_conv_stats_begin(float* part, long cap_floats);
int kg_conv_stats_end(int* nb);
int kg_bn_finalize_train(const float* part, int nb, int M, int C, const float* gamma, const float* beta, float* running_mean,
                         float* running_var, float momentum, float eps, float* mean_out, float* invstd_out, float* scale,
                         float* shift, void* stream);
int kg_bn_scale_shift_eval(int C, const float* gamma, const float* beta, const float* running_mean,
                           const float* running_var, float eps, float* scale, float* shift, void* stream);
int kg_bn_apply(const void* x, int ldx, const float* scale, const float* shift, const void* res, int ldres, void* y,
                int ldy, int M, int C, int relu, const kg_planes_t* planes, void* stream);
int kg_bn_bwd(const void* x, int ldx, const void* dy, int lddy, const float* gamma, const float* mean,
              const float* invstd, float* dgamma, float* dbeta, int accumulate, void* dx, int lddx, int M, int C,
              float* scratch, int scratch_floats, const float* parts, int nb_parts, const float* parts_scale,
              const kg_planes_t* planes, void* stream);
/* Backward of a FROZEN BatchNorm2d (running statistics as constants in a training step -- torchvision's FrozenBatchNorm2d; the reference
 * fine-tunes an ImageNet backbone at batch size 2, train.py:22,71): y = x * scale + shift, scale = gamma * rsqrt(running_var + eps)
 * (kg_bn_scale_shift_eval).  ONE streaming pass: dx = scale[c] * dy, dbeta[c] = sum dy, dgamma[c] = sum dy * (x - running_mean[c]) *
 * rsqrt(running_var[c] + eps) (block partials in scratch, combined in double in fixed order: reproducible, no atomics).
 * dgamma == dbeta == NULL (gamma / beta frozen too): dx = scale[c] * dy alone -- x, running_mean, running_var, scratch may be NULL.
 * planes: a = x, b = dy, y = dx. */
int kg_bn_bwd_frozen(const void* x, int ldx, const void* dy, int lddy, const float* scale, const float* running_mean,
                     const float* running_var, float eps, float* dgamma, float* dbeta, int accumulate, void* dx, int lddx,
                     int M, int C, float* scratch, int scratch_floats, const kg_planes_t* planes, void* stream);
/* BACKWARD statistics from the input gradient that completes dy (train-mode BatchNorm under autograd, KGnet.py:82-93 + train.py:153):
 * kg_conv_bstats_begin arms the calling host thread's next dense input-gradient launch (kg_conv2d_igemm mode 1 on the gather kernel, kg_conv2d_halo
 * with flip = 1 and KS = 3; output channels a multiple of 64): besides storing the gradient rows g (after the residual add and the ReLU mask of
 * its epilogue) that launch writes per-(pixel tile, channel) partials {sum g, sum g * xhat}, xhat = (x - mean[c]) * invstd[c] over the rows x of
 * the BatchNorm's INPUT (same row index; x_planes planes, x_pstride elements apart).  kg_conv_stats_end returns the tile count (0: the launch took
 * a kernel without this epilogue) and disarms.  kg_bn_bwd takes the partials as parts / nb_parts and skips its own column reduction over x and
 * dy; parts_scale (optional device scalar): a power of two dy was multiplied by AFTER the partials were taken (kg_rows_rescale). */
int kg_conv_bstats_begin(float* part, long cap_floats, const void* x, int ldx, int x_planes, int x_pstride, const float* mean,
                         const float* invstd);
int kg_maxpool3s2_fwd(const void* x, int ldx, void* y, int ldy, void* argmax_u8, int N, int H, int W, int C, const kg_planes_t* planes, void* stream);
int kg_maxpool3s2_bwd(const void* x, int ldx, const void* dy, int lddy, void* dx, int lddx, const void* argmax_u8, int N, int H, int W, int C,
                      const kg_planes_t* planes, void* stream);   /* argmax_u8 (optional): [N*OH*OW][C] winning taps written by the forward */
int kg_bilinear_fwd(const void* x, int ldx, void* y, int ldy, int N, int IH, int IW, int OH, int OW, int C,
                    const int* boxdesc, const int* row2box, long total_out_rows, const kg_planes_t* planes, void* stream);
int kg_bilinear_bwd(const void* dy, int lddy, void* dx, int lddx, int N, int IH, int IW, int OH, int OW, int C,
                    const int* boxdesc, const int* row2box, long total_in_rows, const void* mask, int ldmask,
                    const kg_planes_t* planes, void* stream);
                    /* mask != NULL: dx is zeroed where mask <= 0 (ReLU backward of the upsampled tensor, KGnet.py:110) */
int kg_add_rows(const void* a, int lda, const void* b, int ldb, const void* mask, int ldm, void* y, int ldy, long M,
                int C, const float* scale, const float* scale2, const kg_planes_t* planes, void* stream);
                /* y = (a + b) [* *scale [* *scale2]] [where mask > 0]; scale / scale2: optional device scalars (powers of two: a gradient written
                   under an earlier running scale of the half-precision backward is converted inside the join that reads it, cf. kg_rows_scale) */
int kg_sigmoid_inplace(float* x, long n, void* stream);                              /* torch.sigmoid, KGnet.py:300,345 */
int kg_grad_pack(const float* g_nchw, const float* prob, void* out_rows, int N, int C, int H, int W, int ld, int cpad,
                 const kg_planes_t* planes, void* stream);   /* planes: y = out_rows */
int kg_grad_pack3(const float* g0_nchw, const float* g1_nchw, const float* g2_nchw, const float* prob0, void* out_rows, int N, int C0, int C1, int C2,
                  int H, int W, int ld, int pad0, int pad1, int pad2, const kg_planes_t* planes, void* stream);
                  /* the three map gradients of one pyramid level (kp | short | mid: the backward of KGnet.py:300-316) side by side in one pass: columns
                     [0, pad0) <- g0 (* prob0 (1 - prob0) when given), then pad1 columns of g1, pad2 of g2 (pads % 8 == 0, sum <= 64); planes: y = out_rows */

/* ---- losses: DetectionLossAll (loss.py:12-49) and the per-pair mask BCE of SEG_loss (seg_loss.py:86-94) ---- */
int kg_detection_loss_fwd(const float* kp, const float* sh, const float* md, const float* gt, int N, int H, int W,
                          float kp_radius, const float* den_override, float* scratch, int scratch_floats, float* out8,
                          void* stream);
int kg_detection_loss_bwd(const float* kp, const float* sh, const float* md, const float* gt, int N, int H, int W,
                          float kp_radius, const float* fin8, const float* grad_out, float* g_kp, float* g_sh,
                          float* g_md, void* stream);
int kg_seg_loss(const float* prob, const void* tgt_u8, const int* patches, const void* pairs, int npatches, float* part,
                float* out1, const float* grad_out, float* gprob, void* stream);

/* measurement hook (bench.py --mode eval): begin arms this host thread -- every kg_postproc_scale call then records HIP events at its
 * phase boundaries on its own stream; end waits and returns the summed milliseconds {Hough vote, Gaussian, peaks + ranking, grouping} */
int kg_postproc_timing_begin(void);
int kg_postproc_timing_end(float* ms4);
/* ---- post-processing in float64, bit-identical to postprocessing.py:16-261 and nms.py:4-53 ----
 * Capacities (kg_postproc_scale and, per image, kg_postproc_batch; tests/test_gpu_detect.py part D).  With T = the peaks of the map:
 *   npeaks_out                   T, the full count, whatever peak_cap is
 *   peaks_out, peak_conf_out     [3][peak_cap] (ids | xs | ys) and [peak_cap]: the first min(T, peak_cap) peaks in scan order (channel, then
 *                                row, then column); the entries behind them are unspecified.  Later peaks are dropped without an error.
 *   ranking, grouping            see those min(T, peak_cap) peaks only: the result is the reference's grouping of the truncated list
 *   nskel                        the skeletons formed, which may exceed skel_cap: rows [0, min(nskel, skel_cap)) of skel are written, none
 *                                beyond.  Up to 8192 ranked peaks on a map of at most 1024 x 1024 this is the full count of the reference's
 *                                grouping.  On larger inputs a skeleton beyond skel_cap is not remembered and cannot suppress a later seed near
 *                                it: once nskel > skel_cap it need not be the reference's count any more (the first skel_cap rows are exact either way).
 * kg_skeleton_boxes reads min(nskel, skel_cap) rows and adds the boxes it forms to nbox; rows at or beyond box_cap are dropped, nbox still
 * counts them, and a later appending call then writes nothing.  kg_nms reads min(nbox, box_cap) rows. */
long kg_postproc_workspace_bytes(int H, int W, int peak_cap, int skel_cap);
int kg_postproc_scale(const float* kp, const float* soff, const float* mid, int H, int W, double thresh, void* ws,
                      long ws_bytes, int peak_cap, int skel_cap, double* skel, int* nskel, double* heat_out,
                      double* blur_out, int* peaks_out, double* peak_conf_out, int* npeaks_out, void* stream);
int kg_skeleton_boxes(const double* skel, const int* nskel, int skel_cap, double scale, int do_refine, double* boxes,
                      int* nbox, int box_cap, void* stream);
int kg_nms(const double* boxes, const int* nbox, int box_cap, double thresh, void* ws, long ws_bytes, double* out,
           int* nkeep, void* stream);

/* ---- batched post-processing: N images per launch (test.py:105-116 for a batch).  kg_postproc_scale, kg_skeleton_boxes and kg_nms are
 * the N = 1 case of the same kernels; every result is bit-identical to the single-image call on that image's maps. ----
 * workspace of kg_postproc_batch: N slices of kg_postproc_workspace_bytes(H, W, peak_cap, skel_cap) bytes (a multiple of 256), one per image
 * (its own header, counters and fall-back flags); -1 on bad arguments */
long kg_postproc_batch_workspace_bytes(int N, int H, int W, int peak_cap, int skel_cap);
/* postprocessing.py:16-147 (Hough vote, Gaussian, peaks, grouping) of one scale for N images: kp [N][5][H][W], soff [N][10][H][W],
 * mid [N][40][H][W] device fp32, contiguous.  Outputs: skel [N][skel_cap][5][3] f64, nskel [N] (skeletons found; may exceed skel_cap) */
int kg_postproc_batch(const float* kp, const float* soff, const float* mid, int N, int H, int W, double thresh, void* ws,
                      long ws_bytes, int peak_cap, int skel_cap, double* skel, int* nskel, void* stream);
/* postprocessing.py:150-261 (refine + skeleton_to_box + gather_skeleton) for N images, one workgroup per image: skel, nskel, skel_cap and
 * scale are HOST arrays of nscales (<= 4) entries, skel[s] = device [N][skel_cap[s]][5][3] f64, nskel[s] = device int [N]; the boxes of
 * image n are appended scale after scale to boxes [N][box_cap][5] f64 from row 0, nbox[n] = their count (rows beyond box_cap dropped) */
int kg_skeleton_boxes_batch(int N, int nscales, const double* const* skel, const int* const* nskel, const int* skel_cap,
                            const double* scale, int do_refine, double* boxes, int* nbox, int box_cap, void* stream);
/* workspace of kg_nms_batch: N slices of box_cap * 9 bytes (+ alignment); -1 on bad arguments */
long kg_nms_batch_workspace_bytes(int N, int box_cap);
/* nms.py:4-53 for N images, one workgroup per image over boxes [N][box_cap][5] / nbox [N]: nkeep[n] = boxes kept of image n, out = the kept
 * rows of all images in pick order, image after image (image n from row nkeep[0] + .. + nkeep[n-1]); out holds N * box_cap rows */
int kg_nms_batch(int N, const double* boxes, const int* nbox, int box_cap, double thresh, void* ws, long ws_bytes, double* out,
                 int* nkeep, void* stream);

/* ---- ground-truth maps of one pyramid scale (preprocessing.get_ground_truth, preprocessing.py:107-118, assembled and cast
 * as dataset_base.py:99-109): kps = device float32 [n][5][2] (x,y) keypoints tl,tr,bl,br,centre; out = device float32
 * [55][H][W] (kp 5 | short 10 | mid 40), bit-identical to the reference's float32 tensors ---- */
int kg_gt_maps(const float* kps, int n, int H, int W, float* out, void* stream);

/* ---- training samples prepared on the device (BaseDataset.__getitem__, dataset_base.py:81-116, under train.py:77-85's transform
 * pipelines; csrc/sampleprep.hip).  imgs = device table of N 80-byte records, one per image:
 *   { const uint8* img [h][w][3]; const void* masks; int h, w, He, We; int oy, ox, flags, perm; float delta, alpha; int inst0, n;
 *     long ld; long pad; }
 * masks = bytes [n][h][w] (any non-zero value foreground) or, with flag 4, 64-bit words [n][ld] in the bit-mask layout below; (He, We) =
 * canvas after Expand and (oy, ox) the paste window's origin (transforms.py:86-106; source size and 0 when off); flags 1 / 2 = mirror
 * along w / h (transforms.py:148-162); perm = source channel of output channel c in bits 2c..2c+1 (transforms.py:56-66); delta, alpha =
 * brightness, contrast (transforms.py:22-46; 0 and 1 when off); inst0 = first instance of the image in the batch-wide instance order;
 * ld = elements between two masks.  H, W = network input size, multiples of 8, W <= 4096.
 * kg_sp_image: out = device float32 [N][3][H][W]: float32 INTER_LINEAR resize of the photometric, expanded, mirrored image
 *   (transforms.py:165-170; the rule of kg_mask_paste), then clip, / 255 - 0.5, CHW (dataset_base.py:104-106).  One launch.
 * kg_sp_warp_masks: out = device bytes [ntot][H][W] of 0 / 1, the nearest resize of the expanded, mirrored masks (transforms.py:171-176:
 *   src = min(floor(dst * scale), size - 1), scale = 1 / (dsize / ssize) in double) of all instances of the batch, inst_img = device
 *   int32 [ntot], the image of every instance; box = device int32 [ntot][16], zero-filled by the caller, receives the bounding boxes of
 *   the ones at divide scales 1, 2, 4, 8 (dataset_base.py:58-71), encoded as maxima.  One launch; the expanded canvas never exists.
 * kg_sp_boxes: box -> per image, in instance order: kp = device float32 [4][ntot][5][2], the keypoints (x, y) of tl, tr, bl, br, centre
 *   of the instances kept at each scale (dataset_base.py:72-78); gtb = device float32 [ntot][5] = (y1, x1, y2, x2, 1) and keep = device
 *   int32 [ntot] (instance index) of the instances load_gt_masks_bboxes keeps (dataset_base.py:43-56); the lists of image i start at row
 *   inst0 of their table; counts = device int32 [N][5] (scales 1, 2, 4, 8, gt).
 * Ground truth as a label map: with flag 8 (SP_LABELS) masks = int32 [h][w], the label map of the image, and ld is ignored; kg_sp_image
 *   and kg_sp_boxes ignore the flag, and such a record is never passed to kg_sp_warp_masks.
 * kg_sp_warp_labels: kg_sp_warp_masks for label-map images.  jobs = device int32 [ntot][6] = (img, id, y1, x1, y2, x2), the half-open
 *   box in source coordinates, rows inst0 .. inst0 + n - 1 those of image img; out = device bytes [ntot][H][W] of 0 / 1; box as above,
 *   zero-filled by the caller, in the same encoding.  With (sy, sx) the source index of output pixel (y, x) under the record of image img
 *   (the composite map above: -1 outside the paste window), pixel (y, x) of job k is 1 iff all of: (unsigned)img < (unsigned)N; sy and sx
 *   lie inside the paste window; (sy, sx) lies inside the job box clamped to [0, h] x [0, w]; labels[sy][sx] == id.  Otherwise it is 0:
 *   a pixel outside the window is 0 whatever id is, id = 0 included.  id is any int32 and is compared only; img and the box are
 *   predicates only, no address is formed from them nor from a label, so a wrong table gives zeros or wrong pixels and cannot leave the
 *   buffers; the source is loaded only inside the forward image of the box.  A record without flag 8 gives zeros.  One launch; every
 *   output element is written.  Refused before any launch: null pointers (ntot == 0 returns 0 with null buffers), N outside 1 .. 65535,
 *   ntot < 0, H or W no multiple of 8, H > 65535, W > 4096, jobs / box off 4-byte alignment (out off 16-byte alignment when W % 16 == 0),
 *   out, box and jobs overlapping.
 * kg_sp_warp_labelmap: out = device int32 [N][H][W], out[i][y][x] = labels_i[sy][sx] inside the paste window and 0 outside.  One
 *   launch.  For every job whose box holds all pixels of its id, kg_sp_warp_labels' out[k] == (out[img] == id). ---- */
int kg_sp_image(const void* imgs, int N, int H, int W, float* out, void* stream);
int kg_sp_warp_masks(const void* imgs, const int* inst_img, int ntot, int H, int W, void* out, int* box, void* stream);
int kg_sp_boxes(const void* imgs, int N, const int* box, int ntot, int kp_radius, int* counts, float* gtb, float* kp, int* keep,
                void* stream);
int kg_sp_warp_labels(const void* imgs, int N, const int* jobs, int ntot, int H, int W, void* out, int* box, void* stream);
int kg_sp_warp_labelmap(const void* imgs, int N, int H, int W, int* out, void* stream);

/* ---- fused multi-tensor Adam step (train.py:71,154), fp32, torch.optim.Adam's operation order.  jobs = device array of 48-byte
 * records {float* p; const float* g; float* m; float* v; long n; int blk0; int pad;}, blk0 = first workgroup of the job (4096
 * elements per workgroup); step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t) ---- */
int kg_adam_step(const void* jobs, int njobs, int total_blocks, float beta1, float beta2, float eps, float step_size, float bc2_sqrt,
                 float weight_decay, void* stream);

/* ---- host glue of SEG_loss (seg_loss.py:57-80), pure host code: crops of the matched ground-truth masks (float32 [n][H][W] per
 * image), nearest-resized to the patch size, as bytes.  work = int32 [nwork][9]: (img, gt, y1, y2, x1, x2, h1, w1, out offset) ---- */
int kg_host_crop_masks(const float* const* masks, const int* work, int nwork, int H, int W, unsigned char* out);
/* the same crops for DEVICE-resident masks (seg_loss.py:57-80 on the GPU): masks = device array of device pointers
 * (float32 [n_i][H][W]), work = device int32 [nwork][9] (the rows of kg_host_crop_masks), out = device bytes */
int kg_crop_masks(const void* masks, const int* work, int nwork, int H, int W, void* out, void* stream);
/* box tables of the per-box seg branch (host glue of KGnet.py:258-267,321-350; pure host code, integer arithmetic).
 * kg_host_tile_table: one {row0, (h << 16) | w, (oy0 << 16) | ox0, 0} entry per th x tw tile of every box (box-major); returns the count.
 * kg_host_bin_csr: per BS x BS bin of each image the ascending list of boxes touching it (tab = int32 [nb][8] rows {img, y1, x1, h, w, ..});
 * returns the number of (box, bin) incidences.  Both return -1 when the output does not fit cap. */
int kg_host_tile_table(const int* h, const int* w, const long* row0, int nb, int th, int tw, int* out, int cap);
int kg_host_bin_csr(const int* tab, int nb, int BS, int BY, int BX, int nbins, int* bin_start, int* bin_boxes, int cap);
/* matching of seg_loss.py:14-29,55-56 (jaccard_numpy >= thresh over all predicted x ground-truth boxes of an image), pure host code,
 * float32 in the reference's operation order: pairs = int32 [cap][2] (patch, gt) row-major, *count = matches */
int kg_host_match_boxes(const float* pb, int P, const float* gb, int G, int gstride, float thresh, int* pairs, int cap, int* count);

/* ---- evaluation metrics (eval_parts.mask_iou inside seg_evaluation, eval_parts.py:4-9,98-150): exact pixel counts.
 * masks = device bytes [n][ld], ld % 16 == 0, non-zero byte = foreground, padding zero ---- */
int kg_mask_areas(const void* masks, int n, long ld, int* area, void* stream);
int kg_mask_inter_pairs(const void* a, const void* b, const int* pairs, int npairs, long ld, int* inter, void* stream);

/* ---- bit-mask layout: one mask of H x W pixels as 64-bit words, one bit per pixel.
 *   - row-major; every image row takes wpr = ceil(W / 64) words;
 *   - bit b (value 1 << b) of word k of row y is pixel (y, 64 k + b); bits at x >= W are zero;
 *   - one mask occupies ld_words = round_up(H * wpr, 2) words, so every mask of a 16-byte aligned [n][ld_words] buffer starts 16-byte
 *     aligned; the padding word is zero.
 * On a little-endian host np.unpackbits(words.view(np.uint8), bitorder="little") recovers the pixels.  A 512 x 512 mask is 32 KB
 * (bytes: 256 KB, float32: 1 MB).
 * kg_mask_bits_ld: ld_words of an H x W mask (host helper; -1 on bad arguments).
 * kg_mask_pack_bits: device masks [n][H][W], float32 (src_is_f32 != 0) or bytes, any non-zero value foreground -> words [n][ld_words].
 * kg_mask_unpack_bits: words -> device [n][H][W] of 0 / 1, bytes (out_is_u8 != 0) or float32.
 * kg_bitmask_areas / kg_bitmask_inter_pairs: kg_mask_areas / kg_mask_inter_pairs on words (16-byte loads + popcount, exact int32 counts);
 * a and b hold na and nb rows -- the masks of all images of a batch that share one size, concatenated -- and a pair that names a row
 * outside them is not read: its count is -1.
 * Every entry checks its arguments (null pointers, counts and sizes <= 0, an ld_words that is odd or below kg_mask_bits_ld(H, W)) before
 * any HIP call. ---- */
long kg_mask_bits_ld(int H, int W);
int kg_mask_pack_bits(const void* masks, int src_is_f32, int n, int H, int W, void* words, long ld_words, void* stream);
int kg_mask_unpack_bits(const void* words, long ld_words, int n, int H, int W, void* out, int out_is_u8, void* stream);
int kg_bitmask_areas(const void* words, int n, long ld_words, int* area, void* stream);
int kg_bitmask_inter_pairs(const void* a, int na, const void* b, int nb, const int* pairs, int npairs, long ld_words, int* inter,
                           void* stream);
/* Instance results from the words (csrc/instances.hip).  Input: the masks of nimg images of one size H x W, rows concatenated; image i
 * owns rows [row_start[i], row_start[i + 1]) -- row_start is a HOST array of nimg + 1 ints, row_start[0] == 0, non-decreasing,
 * row_start[nimg] == n (what predict(packed=True) and inference.image_row_ranges produce).  Row order is priority order.
 * kg_instance_labels: labels = device int32 [nimg][H][W], 0 where no row of the image covers the pixel, else the id of the first covering
 * row: ids[row] (device int32 [n], values only) or, with ids == NULL, row - row_start[i] + 1.  table (optional) = device int64 [n][8], one
 * line per row: {area_full, area_visible, y1, x1, y2, x2, sum_y, sum_x} -- set bits of the row, pixels of the label map the row won,
 * their half-open bounding box (0, 0, 0, 0 if none) and their coordinate sums; exact integers.
 * kg_instance_overlay: apply_mask (test.py:29-37) for every row of an image in ascending row order, on image = device bytes
 * [nimg][H][W][3] into out (same shape, may equal image): every covered channel becomes (uint8)(v * (1 - alpha) + alpha * color[c] * 255)
 * in float64, truncated; colors = device float64 [n][3] in [0, 1], alpha in [0, 1].
 * Both write every element of labels / table / out (an image without rows: zeros / the image itself; n == 0 is valid), launch a number
 * of kernels that does not depend on n (one per 256 images and output), never synchronise, and validate on the host before any HIP call:
 * null pointers, H, W > 0, n >= 0, nimg > 0, ld_words, 16-byte alignment of words, row_start, nimg * H * W <= 2^31 - 1.  No kernel uses
 * a value read from device memory as an index. */
int kg_instance_labels(const void* words, long ld_words, int n, const int* row_start, int nimg, int H, int W, const int* ids, int* labels,
                       long long* table, void* stream);
int kg_instance_overlay(const void* image, const void* words, long ld_words, int n, const int* row_start, int nimg, int H, int W,
                        const double* colors, double alpha, void* out, void* stream);
/* Tiled whole-image inference (csrc/tiling.hip; tiling.py states the semantics in NumPy).  A grid is ny x nx tiles of th x tw pixels;
 * ys / xs are HOST arrays of the tile origins along each axis: 1 .. 256 entries, ys[0] >= 0, strictly ascending, the last below H (W).
 * Tile t = r * nx + c.  A tile may reach past the image.
 * kg_tile_cut: image = device bytes [H][W][3] -> out = device float32 [ny * nx][3][th][tw] (16-byte aligned, tw % 4 == 0), every element
 * written: float32(byte) / 255 - 0.5 in two float32 operations, channels in the image's order; a pixel outside the image is -0.5.
 * kg_bitmask_clip: clears in place every bit at y >= vh or x >= vw of n masks in the bit-mask layout (0 <= vh <= H, 0 <= vw <= W); the
 * padding word and rows >= n are not touched; vh == H && vw == W and n == 0 launch nothing.
 * kg_tile_stitch: tile_labels = device int32 [ny * nx][th][tw], values >= 0 -> labels = device int32 [H][W], every element written once:
 * the smallest non-zero value over the tiles that cover the pixel, 0 if there is none.  A gather: no atomics, no read of labels.
 * kg_label_table: jobs = device int32 [n][5] rows {id, y1, x1, y2, x2}, written and validated by the caller (0 <= y1 <= y2 <= H, the same
 * for x, id > 0; the kernel clamps the box to the map before it forms an address) -> table = device int64 [n][8], every element written:
 * {area_full[j] (device int64 [n]; 0 when NULL), then over the pixels of the box with labels == id: count, y1, x1, y2, x2 (half-open,
 * zeros if none), sum_y, sum_x}; n == 0 is valid.
 * All four validate on the host before any HIP call (null pointers, sizes, ny * nx * th * tw and H * W <= 2^31 - 1, alignment, the
 * origins), never synchronise, and use values read from device memory as stored values and predicates only. */
int kg_tile_cut(const void* image, int H, int W, const int* ys, int ny, const int* xs, int nx, int th, int tw, float* out, void* stream);
int kg_bitmask_clip(void* words, long ld_words, int n, int H, int W, int vh, int vw, void* stream);
int kg_tile_stitch(const int* tile_labels, const int* ys, int ny, const int* xs, int nx, int th, int tw, int H, int W, int* labels,
                   void* stream);
int kg_label_table(const int* labels, int H, int W, const int* jobs, int n, const long long* area_full, long long* table, void* stream);
/* Label-map evaluation (csrc/labelmetrics.hip; labelmetrics.py states the semantics in NumPy): the contingency of two instance label
 * maps -- the area of every id of either map and the pixel count of every (id_a, id_b) pair that meets -- from which the Kaggle score,
 * AJI, PQ, Dice and the reference's AP are computed on the host.
 * kg_label_stats: labels = device int32 [H][W] with ids 1 .. n (0 = background) -> stats = device int32 [n][5], row id - 1 =
 * {area, y1, x1, y2, x2} of the pixels equal to id (half-open box; zeros for an id with no pixel), and invalid[0] = the number of pixels
 * whose value lies outside [0, n].  This is the ONE entry of the family that forms an address from a value read from device memory, and
 * the rule that bounds it is: the index v - 1 is formed only inside the predicate (unsigned)(v - 1) < (unsigned)n (unsigned arithmetic,
 * so no value wraps into range); a pixel that fails it adds one to invalid and touches nothing else, and the stats of every valid id
 * are exact whatever the other pixels hold.  Three launches (init, walk, finish) whatever n is; the walk issues integer atomics (add,
 * min, max) once per run of equal labels inside a 64-pixel row segment, so the result does not depend on arrival order.  n == 0 is
 * valid (stats may then be NULL): every non-zero pixel is invalid.
 * kg_label_inter_jobs: a, b = device int32 [H][W]; jobs = device int32 [m][6] rows {id_a, id_b, y1, x1, y2, x2}, written by the caller
 * -> count = device int64 [m], count[j] = the pixels of the box with a == id_a && b == id_b.  One workgroup per job; the box is clamped
 * to the map before any address is formed (an empty or inverted box gives 0), labels are predicates only, no atomics.  m == 0 is valid
 * and launches nothing.
 * Both validate on the host before any HIP call (null pointers, H, W > 0, H * W <= 2^31 - 1, n, m >= 0, 4-byte alignment, 8 bytes for
 * count), never synchronise and write every output element. */
int kg_label_stats(const int* labels, int H, int W, int n, int* stats, int* invalid, void* stream);
int kg_label_inter_jobs(const int* a, const int* b, int H, int W, const int* jobs, int m, long long* count, void* stream);
/* Label-map clean-up (csrc/components.hip; components.py states the semantics in NumPy): connected components of label maps, what the
 * host needs to decide about them, and the decision written back.
 * kg_label_components: labels = device int32 [nimg][H][W], ANY int32 values (compared only, never an index).  Two pixels of one image
 * belong together if they hold the same value and are adjacent under the rule for that value: `connectivity` (4 or 8) for non-zero
 * values, `bg_connectivity` (0, 4 or 8) for the value 0; with bg_connectivity == 0 zero pixels belong to no component.  comp = device
 * int32 [nimg][H][W]: 0 for a pixel outside every component, else the number of its component, 1 .. m_i per image in raster order of
 * each component's first pixel (smallest y * W + x); ncomp = device int32 [nimg] = m_i.  Images are independent.  workspace = device
 * memory of at least kg_label_components_workspace_bytes (nimg, H, W) bytes (host helper; -1 on bad arguments), 4-byte aligned, contents
 * irrelevant on entry.  Six launches whatever the maps hold.
 * kg_component_stats: comp_start = HOST array of nimg + 1 ints, the prefix sums of ncomp the caller read back (comp_start[0] == 0, non-
 * decreasing, comp_start[nimg] == total) -> stats = device int32 [total][9], row comp_start[i] + c - 1 = {value, area, y1, x1, y2, x2,
 * border, nb_min, nb_max}: the label value of the component, its pixel count, its half-open box, border = 1 if a pixel lies on the first
 * or last row or column of its image, and the smallest and largest comp value over all 4-adjacent pixels of the same image whose comp
 * differs from c (pixels with comp == 0 count as 0; both -1 if there is none).  Integer atomics (add, min, max, or) at most once per run of equal
 * comp values inside a 64-pixel row segment -- one that cannot change its cell is skipped, and each wave folds the runs of one component
 * it meets segment after segment before it commits them -- so arrival order cannot change the result; a row no pixel names is {0, 0, 0, 0, 0, 0, 0, -1, -1}.  total == 0
 * is valid (stats may then be NULL).  Two launches plus one per 256 images.
 * kg_component_remap: newval = device int32 [total] -> out = device int32 [nimg][H][W] = newval[comp_start[i] + c - 1] where comp == c > 0,
 * 0 elsewhere; out may alias neither input.  One launch per 256 images.
 * All three validate on the host before any HIP call (null pointers, nimg, H, W > 0, nimg * H * W <= 2^31 - 1, the connectivities, the
 * workspace size, 4-byte alignment, comp_start), never synchronise and write every output element.
 * INDEX RULE.  This family is the second exception (after kg_label_stats) to "no kernel uses a value read from device memory as an
 * index": union-find cannot avoid it.  The parent array lives in `workspace`; the entry's own first kernel writes the whole array before
 * any kernel reads it; it only ever holds linear pixel indices of the same image, written by these kernels; a parent never exceeds its
 * own index (atomicMin only lowers values), so every find loop descends strictly; every dereference of a value v read from memory still
 * sits inside the predicate (unsigned)v < (unsigned)(H * W); every find and union loop also has a hard iteration bound.
 * kg_component_stats and kg_component_remap index by c - 1 only inside (unsigned)(c - 1) < (unsigned)m_i: a comp value that fails the
 * predicate touches nothing and writes 0.  The root of a set is its smallest linear index, so comp and ncomp are the same whatever
 * order the atomics land in. */
long kg_label_components_workspace_bytes(int nimg, int H, int W);
int kg_label_components(const int* labels, int nimg, int H, int W, int connectivity, int bg_connectivity, int* comp, int* ncomp,
                        void* workspace, long workspace_bytes, void* stream);
int kg_component_stats(const int* labels, const int* comp, int nimg, int H, int W, const int* comp_start, int total, int* stats,
                       void* stream);
int kg_component_remap(const int* comp, int nimg, int H, int W, const int* comp_start, int total, const int* newval, int* out, void* stream);
/* Per-instance measurements (csrc/measure.hip; measure.py states the semantics in NumPy): the exact integers every shape, contact and
 * intensity measurement of an instance is a function of; the host derives centroid, axes, orientation, perimeter, mean and std from them.
 * kg_label_measure: labels = device int32 [nimg][H][W], ANY int32 values (compared only); image = device [nimg][H][W][channels] of unsigned
 * elements of elem_bytes bytes (1 or 2), NULL exactly when channels == 0; jobs = device int32 [m][6] rows {img, id, y1, x1, y2, x2}
 * (half-open box), written by the caller -> out = device int64 [m][10 + 4 * channels], every element written.  With P = the pixels of the
 * box, clamped to the map, of image img with labels == id, a row is {area = |P|; sum_y, sum_x, sum_yy, sum_yx, sum_xx over P of the pixel
 * coordinates in the image; edges = the (pixel of P, direction up / down / left / right) pairs whose neighbour lies outside the map or
 * holds a value != id; edges_border = those whose neighbour lies outside the map; edges_contact = those whose neighbour lies inside the
 * map and holds a non-zero value != id; boundary_pixels = the pixels of P with at least one such edge; then per channel c: sum_c, sumsq_c,
 * min_c, max_c over P (min and max 0 when area == 0)}.  Neighbours are read from the MAP, never from the box: a box edge inside the map
 * is not an object edge, so the rows of bands that tile a box add up (min / max over the bands with area > 0) to the row of the box.
 * SIZE RULE.  H, W <= 32768, so area <= 2^30, a coordinate product < 2^30, a coordinate sum < 2^60 and a 16-bit sum of squares < 2^62:
 * every column fits int64; larger maps are refused.
 * INDEX RULE.  No value read from device memory becomes an index: the job table is the one device-read table, its box is clamped to the
 * map before any address is formed and its image index is used only inside (unsigned)img < (unsigned)nimg (a job that fails it, or whose
 * box is empty or inverted, writes a row of zeros); labels and pixel values are predicates and summands only; a neighbour outside the map
 * is decided by a predicate on its coordinates before its address exists.
 * One launch whatever m is (one workgroup per job, no atomics); m == 0 is valid and launches nothing (jobs and out may then be NULL).
 * Validates on the host before any HIP call (null pointers, nimg, H, W > 0, the size rule, nimg * H * W <= 2^31 - 1, channels in 0 .. 4,
 * elem_bytes in {1, 2} whatever channels is, m >= 0, 4-byte alignment of labels and jobs, 8 of out, 2 of a 2-byte image) and never
 * synchronises. */
int kg_label_measure(const int* labels, int nimg, int H, int W, const void* image, int channels, int elem_bytes, const int* jobs, int m,
                     long long* out, void* stream);
/* Nearest-other-label distance maps (csrc/distance.hip; distance.py states the semantics in NumPy): expand, ring, shrink, inscribed circle.
 * THE TRANSFORM.  labels = device int32 [nimg][H][W], ANY int32 values (compared only); max_d2 in 1 .. 4096, R = floor(sqrt(max_d2)) <= 64.
 * For a pixel p with value v, C(p) = the pixels q of the SAME image with labels[q] != v and |p - q|^2 <= max_d2; d2[p] = the smallest
 * |p - q|^2 over C(p) and nearest[p] = the smallest value (signed compare) among the q of C(p) at that distance; with C(p) empty
 * d2[p] = max_d2 + 1 ("saturated") and nearest[p] = v.  With frame != 0 the four sides of the image count as another value for d2 only:
 * f = min(y + 1, x + 1, H - y, W - x), and where f^2 <= max_d2, d2[p] = min(d2[p], f^2).  No order of execution changes the result.
 * kg_label_distance: d2, nearest = device int32 [nimg][H][W], every element written; either may be NULL (that output is skipped), not
 * both; neither may alias labels or the other.
 * kg_label_regrow: the same computation, only a result map reaches memory.  Needs 0 <= lo2 <= hi2 <= max_d2.
 *   op 0 (expand)  out = nearest where labels == 0 && d2 <= hi2, else labels; lo2 == 0, frame == 0
 *   op 1 (ring)    out = nearest where labels == 0 && lo2 < d2 <= hi2, else 0; frame == 0
 *   op 2 (shrink)  out = labels where labels != 0 && d2 > hi2, else 0; lo2 == 0, frame honoured
 * out may not alias labels.
 * kg_label_inscribed: d2 = kg_label_distance's map; jobs = device int32 [m][6] rows {img, id, y1, x1, y2, x2} (half-open box), the layout of
 * kg_label_measure -> out = device int32 [m][4] rows {d2max, y, x, count} over the pixels of the clamped box with labels == id: the
 * largest d2, the pixel with the smallest y * W + x among those that attain it, the pixel count; {0, -1, -1, 0} for a job with no pixel.
 * These rows are NOT additive over bands: the host takes the largest d2max, then the smallest index, and adds the counts.
 * SIZE RULE.  max_d2 <= 4096: a candidate distance is at most 8192, d2 <= 4097, a vertical run distance <= 64 fits a byte; nimg * H * W
 * <= 2^31 - 1: every pixel index fits int32.
 * INDEX RULE.  Labels and d2 values are predicates and stored values only; a row or column outside the image is decided by a predicate on
 * its coordinates before any address is formed; every loop is bounded by a kernel argument or a constant.  The job table is the one
 * device-read table: its box is clamped to the map before any address is formed and its image index is used only inside
 * (unsigned)img < (unsigned)nimg.  No atomics.
 * One launch per 65535 images (the image index is a grid dimension) for distance and regrow; one launch whatever m is for inscribed, and
 * m == 0 is valid and launches nothing (jobs and out may then be NULL).  All three validate on the host before any HIP call (null
 * pointers, nimg, H, W > 0, nimg * H * W <= 2^31 - 1, max_d2, op, lo2 / hi2, frame against op, 4-byte alignment, aliasing, m >= 0) and
 * never synchronise. */
int kg_label_distance(const int* labels, int nimg, int H, int W, int max_d2, int frame, int* d2, int* nearest, void* stream);
int kg_label_regrow(const int* labels, int nimg, int H, int W, int max_d2, int frame, int op, int lo2, int hi2, int* out, void* stream);
int kg_label_inscribed(const int* labels, const int* d2, int nimg, int H, int W, const int* jobs, int m, int* out, void* stream);
/* Touching-neighbour graph (csrc/neighbours.hip; neighbours.py states the semantics in NumPy): which other instances an instance touches,
 * and along how many pixel sides and corners.
 * kg_label_neighbours: labels = device int32 [nimg][H][W], ANY int32 values (compared only); connectivity = 4 or 8; jobs = device int32
 * [m][8] rows {img, id, y1, x1, y2, x2, resume, after} (half-open box), written by the caller -> out = device int64 [m][2 + 3 * slots] rows
 * {count, more, (value, sides, corners) x slots}, 1 <= slots <= 64, every element written.  With P = the pixels of the box, clamped to the
 * map, of image img with labels == id: for every p in P and each of the four side directions, the neighbour pixel, if it lies INSIDE THE
 * MAP and holds a value v with v != id and v != 0, adds 1 to sides[v]; under connectivity 8 the four diagonal directions add to
 * corners[v] by the same rule, under 4 corners is 0 and the diagonals are never read.  The neighbour set is {v : sides[v] + corners[v] >
 * 0}.  Neighbours are read from the MAP, never from the box: a box edge or band edge inside the map is not an object edge, so the rows of
 * bands that tile a box merge by value (sides and corners add) to the row of the box.  Values are compared only: INT_MIN, -1 and INT_MAX
 * are ordinary neighbour values, and id may be any value, 0 included.
 * The row lists the neighbour values in ASCENDING SIGNED ORDER, with resume != 0 only those > after (after is ignored when resume == 0);
 * count = the slots filled (<= slots); more = 1 exactly when a further qualifying value exists beyond the last one written; unused slots
 * are zeros.  A caller pages a long list by launching the job again with resume = 1 and after = the last value it got.
 * A job whose image index lies outside [0, nimg), whose box is empty or inverted, or whose id the box does not hold gets a row of zeros
 * and reads nothing else.
 * SIZE RULE.  H, W <= 32768 as for kg_label_measure: a count stays below 2^33 and fits int64; nimg * H * W <= 2^31 - 1.
 * INDEX RULE.  No value read from device memory becomes an index: the job table is the one device-read table, its box is clamped to the
 * map before any address is formed, its image index is used only inside (unsigned)img < (unsigned)nimg, and resume / after are compared
 * only; label values are compared and stored only; a neighbour outside the map is decided by a predicate on its coordinates before its
 * address exists.  No atomics and no hash table: one workgroup per job extracts the values in order, the smallest qualifying value above
 * a workgroup-uniform cursor per walk of the box, counting the previous one on the same walk -- at most slots + 1 walks per job, and the
 * same row from run to run.
 * One launch whatever m is; m == 0 is valid and launches nothing (jobs and out may then be NULL).  Validates on the host before any HIP
 * call (null pointers, nimg, H, W > 0, the size rule, connectivity, slots, m >= 0, 4-byte alignment of labels and jobs, 8 of out) and
 * never synchronises. */
int kg_label_neighbours(const int* labels, int nimg, int H, int W, int connectivity, const int* jobs, int m, int slots, long long* out,
                        void* stream);
/* Run-length lists (csrc/runlengths.hip; runlengths.py states the semantics in NumPy): the Kaggle rows and COCO counts of every instance
 * of a label map, and the way back from run-length rows to a label map.
 * PIXEL ORDER.  p = x * H + y: down the columns first, then left to right, 0-based (Kaggle's EncodedPixels numbers the same order from 1).
 * JOB.  {img, id, y1, x1, y2, x2}, the layout of kg_label_measure: a half-open box, clamped to the map before any address is formed.
 * P = the pixels of the clamped box in image img with labels == id.  Values are compared only, so id may be any int32, 0, INT_MIN and
 * INT_MAX included.  A job whose image index lies outside [0, nimg), whose box is empty or inverted, or whose id the box does not hold
 * produces nothing.
 * HEAD AND TAIL.  A pixel of P is a head when p == 0 or the map's pixel at p - 1 does not hold id; a tail when p == H * W - 1 or the
 * pixel at p + 1 does not hold id.  The pixel at p - 1 is (y - 1, x), or (H - 1, x - 1) when y == 0; the pixel at p + 1 is (y + 1, x), or
 * (0, x + 1) when y == H - 1.  Both are read from the MAP, never from the box, and a position outside the map is decided by a predicate
 * on its coordinates before its address exists.  A run therefore continues from the bottom of one column into the top of the next: the
 * 4 x 3 map with id at p = 2, 3, 4, 5, 7, 8 has the runs {2, 5} and {7, 8}, Kaggle's "3 4 8 2".
 * RUNS.  The k-th head and the k-th tail of a job in ascending p delimit its k-th run {first, last}, 0-based and inclusive; Kaggle's pair
 * is (first + 1, last - first + 1).  Because the neighbours come from the map, the heads and the tails of column bands that tile a box,
 * taken in ascending x, concatenate to the box's; a band can hold a head whose tail lies in a later band, so the two are counted and
 * offset separately.
 * kg_label_run_counts: labels = device int32 [nimg][H][W]; jobs = device int32 [m][6], written by the caller -> out = device int32 [m][2]
 * rows {heads, tails}, every element written.
 * kg_label_runs: jobs = device int32 [m][8] rows {img, id, y1, x1, y2, x2, head_at, tail_at} -> out = device int32 [R][2].  The k-th head
 * of a job stores its p into out[head_at + k][0], the k-th tail into out[tail_at + k][1], each only inside the 64-bit unsigned predicate
 * (head_at + k) < R (tail_at + k for a tail): a negative or oversized offset from a wrong table never leaves the buffer.  With a table
 * built from kg_label_run_counts (exclusive prefix sums of heads and of tails, R = their total) every element of out is written;
 * nothing else is touched.
 * kg_runs_paint: runs = device int32 [R][3] rows {first, last, value}, SORTED by first and DISJOINT -- the caller's promise, the entry
 * cannot check it -> out = device int32 [H][W], every element written: value where first <= p <= last for a row, else background.  One
 * lane per output pixel in row-major order; the row is found by a binary search over `first` whose loop bound derives from R.
 * R == 0 is valid (runs may then be NULL).
 * SIZE RULE.  H, W <= 32768 as for kg_label_measure; nimg * H * W <= 2^31 - 1 (H * W for kg_runs_paint), so p fits int32.
 * INDEX RULE.  The job table is the one device-read table: its box is clamped to the map before any address is formed and its image
 * index is used only inside (unsigned)img < (unsigned)nimg; label values are compared only.  The store of kg_label_runs is the family's
 * one exception: its slot is an offset of the table plus a PREFIX COUNT OF PREDICATES (not a label value), bounded by the predicate
 * above where it is made.  kg_runs_paint reads row i only for a search position i in [0, R); first, last and value are compared and
 * stored only.  No atomics.
 * One launch whatever m is (one workgroup per job); m == 0 launches nothing (jobs and out may then be NULL), and so does R == 0 for
 * kg_label_runs.  All three validate on the host before any HIP call (null pointers, nimg, H, W > 0, the size rule, m, R >= 0, 4-byte
 * alignment, out not overlapping labels / runs) and never synchronise. */
int kg_label_run_counts(const int* labels, int nimg, int H, int W, const int* jobs, int m, int* out, void* stream);
int kg_label_runs(const int* labels, int nimg, int H, int W, const int* jobs, int m, int* out, int R, void* stream);
int kg_runs_paint(const int* runs, int R, int H, int W, int background, int* out, void* stream);
/* Instance outlines (csrc/contours.hip; contours.py states the semantics in NumPy as contours_host): the outline of every instance of a
 * label map as polygon rings, exact in integers.
 * JOB.  {img, id, y1, x1, y2, x2}, a half-open box clamped to the map.  P = the pixels of the clamped box in image img with labels == id.
 * Everything else is non-P, the same id outside the box included: the polygon of P is self-contained in the box.  Values are compared
 * only: 0, -1, INT_MIN and INT_MAX are ordinary ids.  H, W <= 32768 as for kg_label_measure.
 * LATTICE.  Vertices are (Y, X) with 0 <= Y <= H and 0 <= X <= W; pixel (y, x) is the square between vertices (y, x) and (y + 1, x + 1).
 * CRACKS.  A directed crack leaves a vertex in one of four directions, E (x + 1) = 0, S (y + 1) = 1, W (x - 1) = 2, N (y - 1) = 3.  It
 * exists when P is on its right-hand side and non-P on its left.  With m(y, x) = "the pixel is in P" (false outside the box):
 *     E at (Y, X) iff m(Y, X) && !m(Y - 1, X)              (the top edge of a P pixel)
 *     S at (Y, X) iff m(Y, X - 1) && !m(Y, X)              (the right edge)
 *     W at (Y, X) iff m(Y - 1, X - 1) && !m(Y, X - 1)      (the bottom edge)
 *     N at (Y, X) iff m(Y - 1, X) && !m(Y - 1, X - 1)      (the left edge)
 * SUCCESSOR.  A crack with direction d arrives at vertex V; its successor is the first existing crack leaving V in the order right turn
 * (d + 1) & 3, straight d, left turn (d + 3) & 3.  One always exists.  Right first makes P 4-connected: two pixels that meet only at a
 * corner get separate rings.  8-connectivity is out of scope.
 * RINGS.  The cracks fall into disjoint cycles, the rings.  The vertices of a ring are the vertices where the direction changes.  An
 * outer boundary runs clockwise on the screen and has positive shoelace area; a hole runs the other way and has negative area.  A ring
 * may visit a vertex twice (a diagonal pinch); it never repeats a crack.
 * START.  A candidate is an E crack at (Y, X) with no E crack at (Y, X - 1): the start of a maximal run of top edges.  Every ring holds
 * at least one candidate, and a candidate vertex is always a corner.  The start of a ring is its candidate with the smallest (Y, X) in
 * raster order; the vertex list begins with that vertex and follows the traversal; the closing vertex is not repeated.
 * ORDER.  The rings of a job are ordered by start (Y, X) in raster order; starts are distinct.
 * PER RING.  count = the number of vertices (even, at least 4); perimeter = the number of cracks; area2 = the sum over the vertices of
 * x_i * y_(i+1) - x_(i+1) * y_i, a signed int64 (twice the shoelace area).  Coordinates are absolute map coordinates (Y, X), int32.
 * BAD JOBS.  An image index outside [0, nimg), an empty or inverted box, an id the box does not hold: zero rings.
 * SIZE.  A job is traced on the device when its bitmap fits 32 KiB of LDS: with h, w the clamped box,
 * (h + 2) * 32 * (ceil((w + 2) / 32) | 1) <= 2^18 -- one zero halo on each side and a row pitch of an odd number of dwords.  A job that
 * does not fit gets status = 1 and zero counts from kg_label_contour_counts and writes nothing in kg_label_contours; polygons cannot be
 * banded, so contours.py traces such a job on the host.
 * kg_label_contour_counts: labels = device int32 [nimg][H][W]; jobs = device int32 [m][6], written by the caller -> out = device int64
 * [m][4] rows {rings, vertices, perimeter, status}, every element written.
 * kg_label_contours: jobs = device int32 [m][8] rows {img, id, y1, x1, y2, x2, ring_at, vert_at} -> rings = device int64 [R][4] rows
 * {first, count, perimeter, area2}, verts = device int32 [V][2] rows (y, x).  The k-th ring of a job goes to row ring_at + k only inside
 * the 64-bit unsigned predicate (ring_at + k) < R; its first is vert_at plus the vertex counts of the job's rings before it, and its i-th
 * vertex goes to verts[first + i] only inside (first + i) < V: a negative or oversized offset from a wrong table never leaves the
 * buffers.  With a table built from kg_label_contour_counts (exclusive prefix sums of rings and of vertices, R and V their totals) every
 * element of both is written; nothing else is touched.
 * INDEX RULE.  The job table is the one device-read table: box clamped before any address is formed, image index only inside
 * (unsigned)img < (unsigned)nimg; label values are compared only.  The family's one new exception: the tracer's position is an LDS bit
 * index that depends on bits derived from labels; it is bounded by construction (a crack touches a P pixel of the box) and by an explicit
 * clamp.  No global address depends on a label; global stores depend only on the job table plus prefix counts, inside the range
 * predicates.  No atomics.
 * One launch whatever m is (one workgroup per job); m == 0 launches nothing (jobs and out may then be NULL), and so does R == V == 0 for
 * kg_label_contours.  Both validate on the host before any HIP call (null pointers, nimg, H, W > 0, the size rules, m, R, V >= 0,
 * alignment -- 4 bytes, 8 for the int64 rows --, outputs not overlapping labels or each other) and never synchronise. */
int kg_label_contour_counts(const int* labels, int nimg, int H, int W, const int* jobs, int m, long long* out, void* stream);
int kg_label_contours(const int* labels, int nimg, int H, int W, const int* jobs, int m, long long* rings, int R, int* verts, int V,
                      void* stream);
/* Polygon annotations to a label map (csrc/polygons.hip; polygons.py states the rule in NumPy as fill_host): the exact tiled polygon
 * fill, the inverse of the outlines above.  The fill rule is stated in integers, so the device, the host statement and any other
 * implementation agree on every pixel.
 * LATTICE.  The lattice is that of the outlines.  Pixel (y, x) is the square between vertices (x, y) and (x + 1, y + 1).  Its centre is
 * (x + 0.5, y + 0.5).
 * FIXED POINT.  F = 256.  The host turns a float64 vertex into integers by q = rint(v * 256) (round-half-even).  It rejects non-finite
 * values and |q| > 2^29 (about 2 M pixels).  Every coordinate difference then fits int32.  Every product below is a 32 x 32 -> 64 bit
 * multiply; no 64 x 64 multiply is needed.  A pixel centre is (256 x + 128, 256 y + 128).
 * EDGES.  Every ring contributes its edges, the closing one included, each ordered upward as (x0, y0, x1, y1) with y0 < y1.
 * Horizontal edges are dropped.  The host builds one int32 [E][4] table.  A ring that repeats its first vertex (GeoJSON) therefore
 * costs nothing.  A ring of one or two vertices covers nothing.
 * CROSSING.  An edge counts for a centre (cx, cy) iff
 *     y0 <= cy < y1  and  (x1 - x0) * (cy - y0) > (cx - x0) * (y1 - y0)      (int64)
 * That is, its intersection with the scanline lies strictly right of the centre.
 * PART.  A part is a list of rings.  It covers a pixel iff the number of counting edges over all its rings is odd (even-odd).  Holes,
 * islands in holes and self-intersections need no orientation.
 * ROW.  A row is a list of parts with one int32 value.  It covers a pixel iff any of its parts does (union).  This follows COCO's
 * several polygons per object and GeoJSON's MultiPolygon.
 * MAP.  out[y, x] is the value of the first row, in row order, that covers the pixel, else background.  top = "last" reverses the row
 * order; painter's order is what annotation tools draw.  cover[y, x] (optional) is the number of rows that cover the pixel, each row
 * counted once however many of its parts do.
 * CONSEQUENCES.  Top-left inclusive and watertight: a centre exactly on a left or top edge is inside, on a right or bottom edge it is
 * outside, and polygons that share edges give every pixel to exactly one of them.  The rings of the outlines above have integer
 * vertices, so no centre lies on an edge, and filling the outlines of a label map gives the map back exactly on the traced ids.
 * TABLES.  The map is cut into tiles of KG_POLY_TILE_H x KG_POLY_TILE_W pixels, tiles_y = ceil(H / KG_POLY_TILE_H) rows of tiles_x =
 * ceil(W / KG_POLY_TILE_W); tile t of the stack is (img * tiles_y + ty) * tiles_x + tx.  items = device int32 [n_items][4] rows {value,
 * edge_first, edge_count, row}, one per (tile, part): the part's edges are edges[edge_first .. edge_first + edge_count).  tile_ptr =
 * device int32 [nimg * tiles_y * tiles_x + 1]: tile t walks items[tile_ptr[t] .. tile_ptr[t + 1]) in list order.  For a pixel of tile t
 * an item covers the pixel iff the number of its counting edges is odd; out = the value of the first covering item of the list, else
 * background; cover = the number of covering items whose row differs from the row of the covering item counted before it for that pixel.
 * With the lists polygons.tile_lists builds -- every part in every tile its box meets, in row order, reversed for top = "last" -- this is
 * the MAP rule.  Every element of out (and of cover) is written, an empty tile with background (and 0).  One workgroup per tile stages
 * the edges of an item in LDS in chunks of KG_POLY_EDGE_CHUNK; the result does not depend on the chunking.
 * SIZE RULE.  H, W <= 32768 as for kg_label_measure; nimg * H * W <= 2^31 - 1; E, n_items are int32.
 * INDEX RULE.  Two levels of caller-written tables, the family's one new exception.  tile_ptr[t] and tile_ptr[t + 1] are used only
 * as a range clamped inside [0, n_items]; a decreasing pair is an empty range.  An item's edge_first, edge_count are used only inside
 * the 64-bit unsigned predicates edge_first <= E and edge_count <= E - edge_first (a negative number is a huge unsigned one); a failing
 * predicate empties the item.  No address depends on an edge coordinate, a value or a row.  A wrong table can therefore produce wrong
 * pixels, but it cannot reach outside edges, items, out or cover.  Coordinate differences of an edge table outside the fixed-point
 * range wrap modulo 2^32.  A gather: each pixel is written once by one lane, no atomics, no dependence on the order workgroups run in.
 * ONE launch whatever the sizes are (the grid strides over the tiles); E == 0 or n_items == 0 is valid (edges / items may then be NULL).
 * cover may be NULL.  Validates on the host before any HIP call (sizes, the size rule, null pointers, alignment -- 16 bytes for edges and
 * items, whose rows are read whole, 4 bytes for the rest --, out and cover not overlapping each other or a table) and never
 * synchronises. */
#define KG_POLY_TILE_H 32
#define KG_POLY_TILE_W 64
#define KG_POLY_EDGE_CHUNK 256
int kg_polygons_fill(const int* edges, int E, const int* items, int n_items, const int* tile_ptr, int nimg, int H, int W, int background,
                     int* out, int* cover, void* stream);
/* Convex hulls (csrc/hulls.hip; hulls.py states the semantics in NumPy / Python integers as hulls_host): the convex hull of every
 * instance of a label map and the descriptors that are functions of it -- convex area (solidity), maximum and minimum Feret diameter,
 * hull perimeter (convexity) -- exact in integers.
 * JOB.  {img, id, y1, x1, y2, x2}, a half-open box clamped to the map.  P = the pixels of the clamped box in image img with labels == id.
 * Values are compared only: 0, -1, INT_MIN and INT_MAX are ordinary ids.  H, W <= 32768 as for kg_label_measure.
 * LATTICE.  As for the outlines: pixel (y, x) is the square between vertices (y, x) and (y + 1, x + 1).  C(P) is the set of the four
 * corners of every pixel of P.
 * HULL.  The convex hull of C(P), as the ring of its STRICT vertices: no vertex lies on the segment between its neighbours.
 * RING ORDER.  The ring runs clockwise on the screen: area2 = the sum over the vertices of x_i * y_(i+1) - x_(i+1) * y_i is positive, the
 * sign of an outer ring of the outlines.  It starts at the vertex with the smallest (Y, X) in raster order; the closing vertex is not
 * repeated.  Coordinates are absolute map coordinates (Y, X), int32.
 * EXTENT FORM.  For a lattice line Y let L(Y) be the smallest and R(Y) the largest X of a corner of C(P) on that line; both are defined
 * where pixel row Y - 1 or Y of the box holds a pixel of P.  The ring is, in this order: (top, L(top)); the vertices of the upper concave
 * envelope of R from top to bottom; the vertices of the lower convex envelope of L from bottom to top, excluding the start.  (Y_i, F_i)
 * is a strict envelope vertex iff for all defined j < i < k
 *     (Y_i - Y_j)(F_k - F_i) - (Y_k - Y_i)(F_i - F_j) > 0 for L, < 0 for R;
 * equivalently the largest slope to a defined line before it is strictly below the smallest slope to a defined line after it (above
 * and the largest, for R), both rationals compared by cross-multiplication in int64.  The first and last defined lines always give
 * vertices.  The extent form equals Andrew's monotone chain over C(P) with the start and sign above (tests/test_hulls_cpu.py).
 * ROW.  int64 [10] = {area, count, area2, feret_max2, fmax_i, fmax_j, minw_num, minw_den2, minw_edge, status}.  area = |P|.  count is the
 * number of ring vertices, even or odd, at least 4.  area2 is twice the hull's area.  feret_max2 is the largest squared distance
 * between two ring vertices and (fmax_i, fmax_j), i < j, the ring indices of that pair; a tie goes to the lexicographically smallest
 * pair.  For edge k (ring vertex k to k + 1, cyclic) c_k = the maximum over the ring vertices u of |cross(v_(k+1) - v_k, u - v_k)| and
 * d_k = |v_(k+1) - v_k|^2.  The minimum caliper width squared is the minimum over k of c_k^2 / d_k; minw_num = c_k, minw_den2 = d_k and
 * minw_edge = k of that minimum.  Edges are compared exactly, c_a^2 d_b < c_b^2 d_a, a tie to the smallest k.  With coordinates up to
 * 32768 these products reach 2^93: the comparison is made in 128 bits (two 64 x 64 -> 128 bit products) on the device and in Python
 * integers on the host, never in int64 or float.
 * STATUS.  0 = ok.  1 = the clamped box has more than 4095 rows, the device limit (4096 lattice lines of L and R in 32 KiB of LDS): the
 * row is zero and nothing is stored; hulls.py never produces it, see BANDS.  2 = count > cap: the statistics are right and only the first
 * cap vertices are stored.
 * BAD JOBS.  An image index outside [0, nimg), an empty or inverted box, an id the box does not hold: a row of zeros, no vertices.
 * BANDS.  The hull of a union is the hull of the hulls.  hulls.py cuts a job into pieces of at most max_job_pixels pixels and at most
 * 4095 rows; the host adds the areas, takes the hull (the same monotone chain) of the pieces' ring vertices and recomputes the other
 * columns from the merged ring by the function hulls_host uses.  No job falls back to the host.
 * kg_label_hulls: labels = device int32 [nimg][H][W]; jobs = device int32 [m][8] rows {img, id, y1, x1, y2, x2, vert_at, cap}, written
 * by the caller -> rows = device int64 [m][10], every element written; verts = device int32 [V][2] rows (y, x): ring vertex k of a job
 * goes to verts[vert_at + k] only inside the unsigned predicates k < cap (a negative cap is 0) and (vert_at + k) < V in 64 bits: a
 * negative or oversized offset from a wrong table never leaves the buffer.  With slabs of 2 * (h + 1) vertices (one L and one R per
 * lattice line of the clamped box) no slab can overflow.  Nothing else of verts is touched.
 * INDEX RULE.  The job table is the one device-read table: box clamped before any address is formed, image index only inside
 * (unsigned)img < (unsigned)nimg; label values are compared only.  The one new exception is of the run-slot kind: the vertex slot is
 * vert_at plus a PREFIX COUNT OF PREDICATES, stored only inside the two predicates above.  No atomics on global memory (LDS integer
 * min / max from run heads and tails only).
 * One launch whatever m is (one workgroup of 256 per job, the grid strides beyond 2^20 jobs); m == 0 launches nothing (jobs and rows may
 * then be NULL); V == 0 is valid (verts may then be NULL) and gives the rows alone.  Validates on the host before any HIP call (null
 * pointers, nimg, H, W > 0, the size rules, m, V >= 0, alignment -- 4 bytes, 8 for the int64 rows --, rows and verts not overlapping
 * labels, jobs or each other) and never synchronises. */
int kg_label_hulls(const int* labels, int nimg, int H, int W, const int* jobs, int m, long long* rows, int* verts, int V, void* stream);
/* Per-instance intensity quantiles and histograms (csrc/intensity.hip; intensity.py states the semantics in NumPy as quantiles_host /
 * histograms_host): the order statistics the sums of kg_label_measure cannot give -- median, quartiles, a 5 % / 95 % range, a per-object
 * histogram -- exact in integers.
 * JOB.  {img, id, y1, x1, y2, x2}, the layout and clamp of kg_label_measure.  P = the pixels of the clamped box in image img with
 * labels == id.  Labels are compared only: 0, -1, INT_MIN and INT_MAX are ordinary ids.  image = device [nimg][H][W][channels] of unsigned
 * elements of elem_bytes bytes (1 or 2), 1 <= channels <= 4.  H, W <= 32768 and nimg * H * W <= 2^31 - 1, so a count fits int32.
 * QUANTILE.  A rational num / den with 0 <= num <= den <= 1 000 000; 1 <= Q <= 8 of them per call, passed as the device table
 * qtab = int32 [Q][2] rows {num, den}.  For a channel let n = |P| and v_0 <= ... <= v_(n-1) the sorted values of P.  t = num * (n - 1) in
 * 64 bits; k_lo = t / den, rem = t % den, k_hi = k_lo + (rem != 0).  The device returns the two order statistics lo = v_(k_lo) and
 * hi = v_(k_hi).
 * ROW.  out = device int32 [m][channels][1 + 2 Q] = {n, lo_0, hi_0, ..., lo_(Q-1), hi_(Q-1)}, every element written.  A bad job -- an image
 * index outside [0, nimg), an empty or inverted box, an id the box does not hold -- gets zeros everywhere.  A table row with den <= 0,
 * num < 0 or num > den yields lo = hi = 0 for that quantile without a division.
 * HOST-DERIVED VALUES.  From those integers only, in float64, in code the device route and the host statement share (intensity.py,
 * Quantiles): lower = lo; higher = hi; linear = lo + (hi - lo) * rem / den, numpy's default percentile; iqr where both 1/4 and 3/4 were
 * asked for; n == 0 gives NaN.
 * HISTOGRAM.  A histogram job is int32 [9] = {img, id, y1, x1, y2, x2, channel, shift, prefix}; out = device int32 [m][256], every element
 * written.  With w = value >> shift, 0 <= shift <= 8: prefix < 0: every pixel of P counts into bin min(w, 255), so bin 255 is "255 and
 * above"; prefix >= 0: only the pixels with (w >> 8) == prefix count, into bin w & 255.  channel is used only inside
 * (unsigned)channel < (unsigned)channels and shift only inside (unsigned)shift <= 8: a job that fails either, or is a bad job as above,
 * gets a row of zeros.  8-bit data with shift = 0, prefix = -1 is the exact 256-bin histogram; 16-bit data with shift = 4 the exact
 * histogram of 12-bit camera data; shift = 8 the histogram of the high byte, and shift = 0, prefix = b that of the low bytes under high
 * byte b: the two levels intensity.py selects a quantile of a job too large for one workgroup from.
 * INDEX RULE.  The one new exception of the family: an LDS bin index formed from a pixel value, bounded by construction (& 255, after
 * min(., 255) where the last bin collects, immediately before use, inside a 256-entry array).  No GLOBAL address depends on a pixel or
 * label value; the job table's box is clamped before any address is formed, its image index is used only inside
 * (unsigned)img < (unsigned)nimg; qtab is read at fixed positions.  A wrong job or quantile table gives wrong numbers and cannot leave
 * the buffers.  LDS integer atomics only, none on global memory: the counts are integers, so no order of execution changes a result.
 * One launch each whatever m is (one workgroup of 256 per job, the grid strides beyond 2^20 jobs and clears its LDS per job); m == 0
 * launches nothing (jobs and out may then be NULL).  Both validate on the host before any HIP call (null pointers -- image included --,
 * nimg, H, W > 0, the size rules, channels in 1 .. 4, elem_bytes in {1, 2}, Q in 1 .. 8, m >= 0, 4-byte alignment of labels, jobs, qtab
 * and out, 2 of a 2-byte image) and never synchronise. */
int kg_label_quantiles(const int* labels, int nimg, int H, int W, const void* image, int channels, int elem_bytes, const int* jobs, int m,
                       const int* qtab, int Q, int* out, void* stream);
int kg_label_histograms(const int* labels, int nimg, int H, int W, const void* image, int channels, int elem_bytes, const int* jobs, int m,
                        int* out, void* stream);
/* Merged instances split (csrc/split.hip; split.py states the semantics in NumPy as split_host / regrow_host): two touching nuclei
 * under one id become two ids again -- core seeds, then a seeded geodesic regrow inside the instance.  Everything is an exact integer.
 * SPLIT, the statement split.py composes from existing entries plus kg_label_split.  Inputs: a label map with ids 1 .. n per image, a
 * distance 1 <= d <= 64, connectivity c in {4, 8}, min_seed_area >= 1, frame, and `only` (all ids, or the ids that may be split).
 *   1. CORE.  core = the shrunk labels of kg_label_regrow (op 2) at distance d with the same frame.
 *   2. SEEDS.  The components of core under kg_label_components with connectivity c and bg_connectivity 0.  A seed of id k is a
 *      component of value k with area >= min_seed_area; the seeds of k get ranks 1 .. S_k in ascending component number, which is the
 *      raster order of their first pixels.
 *   3. WHICH.  An id with S_k <= 1, or not in `only`, is untouched.
 *   4. REGROW, for an id with S_k >= 2, over P = the pixels of the id's box with labels == k: see REGROW below.
 *   5. IDS.  Rank 1 keeps k; rank r >= 2 becomes first_new_k + r - 2; the new ids are n + 1, n + 2, ... per image in ascending (k, r).
 *      Every other pixel is copied.
 *   6. RESULTS.  parent = int32 [n_new]: row i < n is i itself, the row of a new id is k - 1.  The per-instance table comes from
 *      kg_label_table over the parents' boxes; a new row's area_full is its parent's.
 * JOB.  {img, id, y1, x1, y2, x2, nseeds, first_new}, a half-open box clamped to the map.  P = the pixels of the clamped box in image img
 * with labels == id.  Values are compared only: 0, -1, INT_MIN and INT_MAX are ordinary ids.  H, W <= 32768 as for kg_label_measure.
 * SEED MAP.  seeds = device int32 of the labels' shape, ANY values.  The rank of a pixel p of P is seeds[p] when
 * 1 <= seeds[p] <= min(nseeds, 16382), else 0 (no seed); a seeds value on a pixel outside P is never used.  Seed s is the set of the
 * pixels of P with rank s; it need not be connected, and a rank may be empty.
 * REGROW.  Two pixels are adjacent when they differ by one step along an axis (c = 4) or also along a diagonal (c = 8).  g(p, s) is the
 * number of steps of the shortest path of adjacent pixels from p to any pixel of seed s that stays inside P: 0 on the seed, infinite
 * without such a path.  A pixel p of P goes to the seed of smallest rank among those with the smallest finite g(p, s).  A pixel no seed
 * reaches is UNREACHED and is handled as rank 1: a piece of the id that holds no seed stays with the id.  Equivalently, a
 * level-synchronous flood: level 0 assigns the seeds; in level L + 1 every unassigned pixel of P with a neighbour assigned in levels <= L
 * takes the smallest rank among those neighbours.  (By induction a pixel is assigned in level min_s g(p, s), and the ranks its
 * neighbours of the level before carry are exactly the ranks s with g(p, s) minimal.)  The result does not depend on any scheduling order.
 * OUTPUT.  out = device int32 of the labels' shape, not overlapping labels or seeds.  The entry fills it as a copy of labels on the stream;
 * the kernel then stores first_new + r - 2 (32-bit wrap-around) on the pixels of rank r >= 2 and nothing else, so every element is
 * written.  Two jobs of one image with different ids never store the same pixel; two jobs with the same id and overlapping boxes are
 * the caller's error (the pixel then holds the value of either).
 * ROW.  rows = device int32 [m][4] = {members, unreached, levels, status}, every element written: members = |P|, unreached as above,
 * levels = the largest finite min_s g(p, s) over P (0 without a seed).  A bad job -- an image index outside [0, nimg), an empty or inverted
 * box, an id the box does not hold -- gets zeros and stores nothing.
 * SIZE.  A job is regrown on the device when its state fits 32 KiB of LDS at 16 bits per pixel with a one-pixel zero halo: with h, w the
 * clamped box, (h + 2) * (w + 2) <= 16384 (126 x 126, or 1 x 5459).  A job that does not fit gets the row {0, 0, 0, 1} and is left as
 * copied.  A geodesic flood cannot be banded, so split.py regrows such a box on the host from that box copied back and writes it in.
 * kg_label_split: labels, seeds = device int32 [nimg][H][W]; connectivity = 4 or 8; jobs = device int32 [m][8], written by the caller.
 * INDEX RULE.  No new exception.  The job table is the one device-read table: box clamped before any address is formed, image index only
 * inside (unsigned)img < (unsigned)nimg; nseeds is the bound of a predicate and first_new a stored value, never an address.  The LDS state
 * is indexed by box-local coordinates alone: no LDS or global address depends on a label, a seed or a rank.  No atomics, no global
 * scratch.
 * One copy and ONE launch whatever m is (one workgroup of 256 per job, the grid strides beyond 2^20 jobs); m == 0 launches only the copy
 * (jobs and rows may then be NULL).  Validates on the host before any HIP call (null pointers, nimg, H, W > 0, the size rules, the
 * connectivity, m >= 0, 4-byte alignment, out not overlapping labels or seeds, rows not overlapping a map, jobs not overlapping out or
 * rows) and never synchronises. */
int kg_label_split(const int* labels, const int* seeds, int nimg, int H, int W, int connectivity, const int* jobs, int m, int* out, int* rows,
                   void* stream);
/* Per-instance texture (csrc/texture.hip; texture.py states the semantics in NumPy as glcm_host): the grey-level co-occurrence matrices
 * of every instance, from which the host derives Haralick's features -- what an instance looks like inside.  A co-occurrence count is a
 * function of PAIRS of pixels: no function of the sums of kg_label_measure or of the bins of kg_label_histograms.  Exact in integers.
 * JOB.  int32 [10] = {img, id, y1, x1, y2, x2, channel, distance, lo, span}: a half-open box with the clamp of kg_label_measure.  P = the
 * pixels of the clamped box in image img with labels == id.  Labels are compared only: 0, -1, INT_MIN and INT_MAX are ordinary ids.
 * image = device [nimg][H][W][channels] of unsigned elements of elem_bytes bytes (1 or 2), 1 <= channels <= 4.  H, W <= 32768 and
 * nimg * H * W <= 2^31 - 1, the rules of kg_label_quantiles, so a count fits int32.
 * LEVEL.  For a pixel value v of channel `channel`: u = max(v - lo, 0), lev = min(u * L / span, L - 1), with 2 <= L <= 32 the per-call
 * argument `levels` and the quotient rounded down.  The value is the exact one for every lo and span > 0 (the int32 one wherever int32
 * does not overflow).  8-bit data with lo = 0, span = 256, L = 16 gives v >> 4; a 12-bit camera uses span = 4096; per-object normalisation
 * uses lo = min, span = max - min + 1 from kg_label_measure.
 * DIRECTIONS.  Four, numbered 0 .. 3, with offsets (dy, dx) = (0, d), (d, d), (d, 0), (d, -d), d = distance.  G[k][i][j] = the number of
 * pixels p of P such that p + o_k lies inside the H x W map, carries the label id, lev at p is i and lev at p + o_k is j.  The partner is
 * read from the MAP, never from the box: a box that cuts an object still counts the pairs that leave the box, and so the matrices of
 * disjoint pieces of a box add up exactly (the banding argument of kg_label_measure).  The matrix of the opposite offset -o_k is the
 * transpose of G[k] taken over the whole object; G + G^T is the symmetric matrix Haralick's features are defined on.
 * ROW.  out = device int32 [m][4][L][L], every element written.  A bad job gets zeros, and nothing divides by span unless it is positive:
 * img outside [0, nimg); an empty or inverted box; channel failing (unsigned)channel < (unsigned)channels; distance failing
 * (unsigned)(distance - 1) < 32; span <= 0.
 * ROUTES.  A workgroup whose clamped box has (h + d) * (w + 2 d) <= 16384 stages the rectangle of rows y1 .. y2 - 1 + d and columns
 * x1 - d .. x2 - 1 + d into LDS, one byte per pixel (the level, or 0xFF for a pixel outside the map or of another label), so that every
 * pixel is loaded and divided once, and counts the pairs from LDS; a larger box counts them straight from global memory.  The route is
 * chosen from the clamped box and d alone, uniformly per workgroup, and both give the same rows.
 * HOST-DERIVED VALUES.  From those integers only, in float64, in code the device route and the host statement share (texture.py,
 * CoMatrices): pairs, the symmetric matrix, Haralick's f1 .. f13 (the formulas stand in texture.py).
 * INDEX RULE.  The exception of kg_label_quantiles' kind: an LDS index formed from pixel values, i * L + j, each level bounded by
 * min(., L - 1) immediately before use, inside int [4][1024].  The staged byte is indexed by a box-local coordinate alone.  No GLOBAL
 * address depends on a pixel or label value; the job table's box is clamped before any address is formed; img, channel, distance and span
 * are used only inside the predicates above, which empty the box when they fail; lo is subtracted and compared only.  A wrong job table
 * gives wrong numbers and cannot leave the buffers.  LDS integer atomics only, none on global memory: no order of execution changes a
 * result; out is written with plain vector stores.
 * One launch whatever m is (one workgroup of 256 per job, the grid strides beyond 2^20 jobs and clears its LDS per job); m == 0 launches
 * nothing (jobs and out may then be NULL).  Validates on the host before any HIP call (null pointers -- image included --, nimg, H, W > 0,
 * the size rules, channels in 1 .. 4, elem_bytes in {1, 2}, levels in 2 .. 32, m >= 0, 4-byte alignment of labels, jobs and out, 2 of a
 * 2-byte image) and never synchronises. */
int kg_label_glcm(const int* labels, int nimg, int H, int W, const void* image, int channels, int elem_bytes, const int* jobs, int m,
                  int levels, int* out, void* stream);
/* Instance midlines (csrc/thinning.hip; thinning.py states the semantics in NumPy as thin_host / midlines_host): the topological
 * skeleton of every instance by exact parallel thinning, and the length, tips and branch points read from it -- what an object with
 * processes (a neural cell, a leaf on its petiole) is measured by.  It is called thinning / midlines everywhere: "skeleton" already means
 * the keypoint skeleton of the post-processing.  Everything is an exact integer.
 * JOB.  {img, id, y1, x1, y2, x2}, a half-open box clamped to the map.  P = the pixels of the clamped box in image img with labels == id.
 * Everything outside the clamped box is background, so a box that cuts an object thins the cut part.  Values are compared only: 0, -1,
 * INT_MIN and INT_MAX are ordinary ids.  H, W <= 32768 as for kg_label_measure.
 * NEIGHBOURS.  Named clockwise from north, y growing downward: P2 = N, P3 = NE, P4 = E, P5 = SE, P6 = S, P7 = SW, P8 = W, P9 = NW.
 * PASS.  One pass is two sub-iterations.  Each is fully synchronous: every decision reads the state at the start of the sub-iteration.
 * A set pixel is deleted iff C == 1 and 2 <= N <= 3 and m == 0, where
 *   C  = (!P2 & (P3|P4)) + (!P4 & (P5|P6)) + (!P6 & (P7|P8)) + (!P8 & (P9|P2))
 *   N1 = (P9|P2) + (P3|P4) + (P5|P6) + (P7|P8)
 *   N2 = (P2|P3) + (P4|P5) + (P6|P7) + (P8|P9)
 *   N  = min(N1, N2)
 *   m  = (P6 | P7 | !P9) & P8        in the first sub-iteration
 *   m  = (P2 | P3 | !P5) & P4        in the second
 * (Guo-Hall's parallel thinning with OpenCV's order of the sub-iterations).  Passes repeat until one deletes nothing, or max_passes
 * have run (max_passes >= 1; 0 means no limit; a negative value is refused).  passes = the number of passes that deleted something.
 * S is what remains: a subset of P with P's 8-connected components and P's 4-connected background components, and -- without a limit --
 * a fixed point of the rule.  Thinning stopped after k passes is an erosion that never deletes a component and never opens or closes
 * a hole.  Pinned by the host statement: a 2 x 2 square leaves its upper-right pixel in 1 pass; a 7 x 54 bar leaves the 48 pixels of
 * its middle row, three in from either end, in 3 passes; an 8 x 8 checkerboard is a fixed point (0 passes).
 * ROW.  rows = device int32 [m][9] = {members, pixels, isolated, ends, junctions, ortho, diag, passes, status}, every element written,
 * counted on S with 8-neighbourhoods inside S: members = |P|; pixels = |S|; isolated = pixels without a neighbour; ends = pixels with
 * exactly one neighbour; junctions = pixels with at least three 0 -> 1 transitions in the cyclic sequence P2 .. P9; ortho = the
 * unordered pairs of S pixels that share a side; diag = the unordered diagonal pairs neither of whose two common side-neighbours is in
 * S (a diagonal that an L already bridges is no edge).  The midline's length is ortho + sqrt(2) * diag, taken on the host in float64.
 * status 0 is ok; status 1: the box does not fit (SIZE), the other columns are 0 and nothing is stored for the job.  A bad job -- an
 * image index outside [0, nimg), an empty or inverted box -- gets a row of zeros with status 0; an id the box does not hold likewise.
 * Example: in a 16 x 21 map, id 1 on rows 2..4 x columns 2..18 plus rows 5..13 x columns 9..11 gives {78, 23, 0, 3, 1, 20, 2, 2, 0};
 * S is row 3 without column 10, plus column 10 on rows 4..12.
 * MAP.  skel = device int32 [nimg][H][W], not overlapping labels: id on the pixels of S of every job, 0 elsewhere.  The entry zeroes it
 * on the stream first, the kernel then stores id on S and nothing else, so every element is written.  It is a label map: every other
 * entry of the family works on it unchanged.  Jobs of one id whose boxes overlap store the union of their results.
 * SIZE.  A job is thinned on the device when one bit per pixel with a one-pixel zero halo fits 16 KiB of LDS (two such bitmaps, 32 KiB
 * per workgroup): with h, w the clamped box and pw = ceil((w + 2) / 32) words per row, (h + 2) * pw <= 4096 -- 126 x 126, 254 x 510 and
 * 4094 x 30 fit, 255 x 510 does not.  Thinning cannot be banded, so thinning.py thins such a box on the host from that box copied back
 * and writes it in.
 * INDEX RULE.  No new exception.  The job table is the one device-read table: box clamped before any address is formed, image index only
 * inside (unsigned)img < (unsigned)nimg.  Every LDS index is a box-local coordinate plus a fixed offset inside the halo; the predicate of
 * the store is an LDS bit and its address a box coordinate: no LDS or global address depends on a label.  No atomics, no global scratch.
 * One clear and ONE launch whatever m is (one workgroup of 256 per job, the grid strides beyond 2^20 jobs and zeroes both bitmaps per
 * job); m == 0 launches only the clear (jobs and rows may then be NULL).  Validates on the host before any HIP call (null pointers, nimg,
 * H, W > 0, the size rules, max_passes >= 0, m >= 0, 4-byte alignment, skel not overlapping labels, rows not overlapping a map, jobs not
 * overlapping skel or rows) and never synchronises. */
int kg_label_thin(const int* labels, int nimg, int H, int W, const int* jobs, int m, int max_passes, int* skel, int* rows, void* stream);
/* Boundary distances between two label maps (csrc/boundaries.hip; boundaries.py states the semantics in NumPy as border_d2_host): for
 * every source pixel of one instance the exact squared distance to the nearest outline pixel of an instance of ANOTHER map.  Hausdorff,
 * HD95, ASSD and the surface Dice are host float64 over these integers.  Every distance is an exact integer.
 * MAPS.  a, b = device int32 [nimg][H][W], one shape, one device, H, W <= 32768 as for kg_label_measure, nimg * H * W <= 2^31 - 1.  Values
 * are compared only: 0, -1, INT_MIN and INT_MAX are ordinary ids.  a and b may be the same map.
 * BORDER PIXEL of id v in a map.  A pixel that holds v and has at least one of its four side-neighbours either outside the map or holding
 * another value.  The neighbours are read from the MAP, never from a box, and a position outside the map is decided by a predicate on
 * its coordinates before its address exists.  It is mask & ~binary_erosion(mask) with the 4-connected cross and a border value of 0.
 * JOB.  int32 [13] = {img, dir, id_s, sy1, sx1, sy2, sx2, id_t, ty1, tx1, ty2, tx2, first}.  dir == 0 takes the sources from a and the
 * targets from b, dir != 0 the other way round; dir is a predicate only.  Both boxes are half-open and clamped to the map before any
 * address is formed.
 * MODE.  Two bits.  Bit 0, sources: 0 = the border pixels of id_s inside the clamped source box, 1 = all pixels of id_s inside it.
 * Bit 1, targets: 0 = border (surface to surface, the medpy / MONAI convention), 2 = region (GlaS).
 * SOURCES S.  As the mode says, in raster order of the source box.  TARGETS T.  The border pixels of id_t inside the clamped target box,
 * always.
 * VALUE.  d2(s) = min over t in T of (ys - yt)^2 + (xs - xt)^2.  In region mode d2(s) = 0 when s lies inside the clamped target box and
 * the target map holds id_t at s.  When T is empty and the region rule does not apply, d2(s) = -1.  d2 fits int32: 2 * 32767^2 < 2^31.
 * Because borders are read from the map and a minimum is taken, pieces compose exactly: the sources of bands of whole rows that tile a
 * source box, in ascending y, concatenate to the box's; the values of rectangles that tile a target box merge by the element-wise
 * minimum with -1 as +infinity (the region rule gives 0 in the one rectangle that holds s).
 * SIZE RULE.  The clamped target box of a job holds at most KG_BORDER_MAX_TARGET_PIXELS = 8192 pixels, so every target fits one 32 KiB
 * LDS list of box-local (y << 16 | x) words whatever the map holds; the boxes alone decide it.  A job that breaks the rule gets the
 * count {0, 0} with status 1 and stores nothing.  The source box has no bound: it is streamed.
 * BAD JOBS.  An image index outside [0, nimg), or an empty or inverted box on either side: counts {0, 0, 0}, nothing stored.
 * kg_label_border_counts: counts = device int32 [m][3] rows {n_sources, n_targets, status}, every element written; `first` is ignored.
 * kg_label_border_d2: d2 = device int32 [D], D <= 2^31 - 1.  The d2 of the k-th source of job j is stored at d2[first_j + k], only
 * inside the 64-bit unsigned predicate first_j + k < D: a negative or oversized first from a wrong table gives wrong values and cannot
 * leave the buffer.  With first = the exclusive prefix sum of n_sources and D = their total every element is written.
 * INDEX RULE.  The d2 slot is of the kg_label_runs kind (an offset of the job table plus a prefix count of predicates); no other
 * exception.  LDS is indexed by compaction counts and holds coordinates, never a label.  No atomics, no global scratch.
 * One launch per entry whatever m is (one workgroup of 256 per job, the grid strides beyond 2^20 jobs); m == 0 launches nothing (jobs
 * and the output may then be NULL), and so does D == 0.  Both validate on the host before any HIP call (null pointers, nimg, H, W > 0,
 * the size rules of both maps, m >= 0, mode in 0 .. 3, D >= 0, 4-byte alignment, the output overlapping neither a map nor the jobs) and
 * never synchronise. */
#define KG_BORDER_MAX_TARGET_PIXELS 8192
int kg_label_border_counts(const int* a, const int* b, int nimg, int H, int W, const int* jobs, int m, int mode, int* counts, void* stream);
int kg_label_border_d2(const int* a, const int* b, int nimg, int H, int W, const int* jobs, int m, int mode, int* d2, int D, void* stream);
/* Instance crops (csrc/crops.hip; crops.py states the semantics in NumPy as crops_host): one fixed-size image patch and one mask per job, the
 * instance itself in the form a second network takes.  A gather with integer arithmetic: everything is exact in integers.
 * JOB.  int32 [10] = {img, id, oy, ox, ay, by, cy, ax, bx, cx}.  Output pixel (i, j), 0 <= i < OH, 0 <= j < OW, samples the source position,
 * in units of 1/65536 pixel with pixel centres at integers,
 *   Y = (oy << 16) + ay * i + by * j + cy        X = (ox << 16) + ax * i + bx * j + cx        (int64)
 * The kernel knows nothing of windows or angles: crops.affine_jobs builds the table (align_corners=False windows, rotations, flips).
 * MASK.  yn = (Y + 32768) >> 16, xn = (X + 32768) >> 16 with arithmetic shifts.  mask = 1 iff 0 <= yn < H, 0 <= xn < W and
 * labels[img][yn][xn] == id, otherwise 0.  Labels are compared only: 0, -1, INT_MIN and INT_MAX are ordinary ids.
 * PATCH, LINEAR (flags bit 0 clear).  y0 = Y >> 16, fy = Y & 65535; x0, fx likewise.  A tap (y, x) inside the map is the image element
 * of the channel, read unsigned; a tap outside is `fill`.  acc = (65536 - fy) * ((65536 - fx) * v00 + fx * v01) + fy * ((65536 - fx) * v10
 * + fx * v11) with v00 = (y0, x0), v01 = (y0, x0 + 1), v10 = (y0 + 1, x0), v11 = (y0 + 1, x0 + 1); the value is (acc + 2^31) >> 32.
 * acc < 2^48, so unsigned 64-bit arithmetic holds it for 2-byte elements.
 * PATCH, NEAREST (flags bit 0 = KG_CROPS_NEAREST).  The tap at (yn, xn), or fill.
 * MASKED (flags bit 1 = KG_CROPS_MASKED).  After sampling, a pixel whose mask is 0 becomes fill.
 * OUTPUTS.  patches = device [m][channels][OH][OW] of the image's element type (channel-first), masks = device uint8 [m][OH][OW].  Either
 * may be absent: a NULL image (with NULL patches) gives masks only, NULL masks gives patches only; at least one is required.  1 <= OH, OW <=
 * 256; 0 <= fill <= 65535, and <= 255 when 1-byte patches are written; m * channels * OH * OW <= 2^31 - 1 (m * OH * OW without patches).
 * image = device [nimg][H][W][channels] of unsigned elements of elem_bytes bytes (1 or 2), 1 <= channels <= 4; H, W <= 32768 and
 * nimg * H * W <= 2^31 - 1 as for kg_label_measure.
 * BAD JOBS.  A job whose img lies outside [0, nimg) gets fill and a zero mask.  No other job is bad: a window that lies beyond the map is
 * padding, not an error.  Every output element is written.
 * Consequences, pinned by the host statement: ay = bx = 65536 with the other coefficients 0 copies the slice; ay = bx = 131072, cy = cx =
 * 32768 gives the mean of each 2 x 2 block rounded half up; an image of 65535 stays 65535 under any fractions; {ay, by, ax, bx} =
 * {0, -65536, 65536, 0} gives the patch and the mask turned by 90 degrees.
 * INDEX RULE.  The first kind of exception, the caller's job table: img is used inside (unsigned)img < (unsigned)nimg, and every tap inside
 * the unsigned 64-bit predicates (unsigned long long)y < H, (unsigned long long)x < W, formed from the int64 Y, X before any narrowing, so
 * extreme coefficients and far origins give fill and cannot leave the buffers.  No address depends on a label or a pixel value.  No
 * atomics, no LDS, no synchronisation.
 * ONE launch whatever m is: a work item is (job, chunk of 1024 output positions in raster order), the grid is capped at 2^20 workgroups of
 * 256 that stride over what is left; a thread owns 4 consecutive positions and stores them as 32-bit words where the plane offset is
 * aligned.  m == 0 launches nothing (jobs and the outputs may then be NULL).  Validates on the host before any HIP call (null pointers, nimg,
 * H, W > 0, the size rules, channels, elem_bytes, the output size, flags, fill, m >= 0, alignment, the outputs overlapping neither an input
 * nor each other) and never synchronises. */
#define KG_CROPS_NEAREST 1
#define KG_CROPS_MASKED 2
int kg_label_crops(const int* labels, int nimg, int H, int W, const void* image, int channels, int elem_bytes, const int* jobs, int m, int OH,
                   int OW, int flags, int fill, void* patches, unsigned char* masks, void* stream);
/* Linking label maps (csrc/linking.hip; linking.py states the semantics in NumPy): which values of ANOTHER map lie under the pixels of an
 * instance -- the overlap lists behind tracks through time-lapse frames, planes stitched into a volume and child / parent relations.
 * kg_label_overlaps: a = device int32 [nimg_a][H][W], b = device int32 [nimg_b][H][W], ANY int32 values (compared only); b may be the
 * same buffer as a (frames of one stack, img_b = img_a + 1); jobs = device int32 [m][11] rows {img_a, id, y1, x1, y2, x2, img_b, dy, dx,
 * resume, after} (half-open box), written by the caller -> out = device int64 [m][5 + 2 * slots] rows {count, more, area, zero, outside,
 * (value, pixels) x slots}, 1 <= slots <= 64, every element written; out overlaps neither map nor the job table.
 * With P = the pixels of the box, clamped to the map, of image img_a of a that hold id, the PARTNER of a pixel (y, x) of P is the pixel
 * (y + dy, x + dx) of image img_b of b.  area = |P|; outside = the pixels of P whose partner does not lie in the map; zero = those whose
 * partner holds 0; pixels[v] = those whose partner holds v, for every v != 0.  area = zero + outside + the sum of pixels[v] over all v.
 * The ids of the two maps are unrelated: id itself is an ordinary partner value, and so are INT_MIN, -1 and INT_MAX.  The rows of bands
 * that tile a box merge by value (pixels add; area, zero and outside add) to the row of the box.
 * The row lists the partner values v != 0 with pixels[v] > 0 in ASCENDING SIGNED ORDER, with resume != 0 only those > after (after is
 * ignored when resume == 0); count = the slots filled (<= slots); more = 1 exactly when a further qualifying value exists beyond the
 * last one written; unused slots are zeros.  area, zero and outside are over all of P on every row, a resumed one included.  A caller
 * pages a long list by launching the job again with resume = 1 and after = the last value it got.
 * A job either of whose image indices lies outside its [0, nimg), whose box is empty or inverted, or whose id the box does not hold gets
 * a row of zeros and reads nothing else.
 * SIZE RULE.  H, W <= 32768 as for kg_label_measure: a count stays at or below 2^30 and fits int64; nimg_a * H * W and nimg_b * H * W
 * <= 2^31 - 1.
 * INDEX RULE.  No value read from device memory becomes an index: the job table is the one device-read table, its box is clamped to the
 * map before any address is formed, img_a and img_b are used only inside (unsigned)img < (unsigned)nimg predicates that empty the box,
 * the partner coordinate is formed in 64 bits and used only inside (unsigned long long)(y + dy) < H and (unsigned long long)(x + dx) < W
 * before its address exists (dy / dx of INT_MIN / INT_MAX read nothing), and resume / after are compared only; label values of either
 * map are compared, counted and stored only.  No atomics and no hash table: one workgroup per job extracts the values in order as
 * kg_label_neighbours does -- at most slots + 1 walks per job, the header counts on the first, and the same row from run to run.
 * One launch whatever m is; m == 0 is valid and launches nothing (jobs and out may then be NULL).  Validates on the host before any HIP
 * call (null pointers, nimg_a, nimg_b, H, W > 0, the size rule, slots, m >= 0, 4-byte alignment of a, b and jobs, 8 of out, out apart
 * from a, b and jobs) and never synchronises. */
int kg_label_overlaps(const int* a, int nimg_a, const int* b, int nimg_b, int H, int W, const int* jobs, int m, int slots, long long* out,
                      void* stream);

/* ---- per-box segmentation branch (KGnet.py:246-267, 321-350): ragged row bookkeeping ---- */
int kg_seg_build_rows(const int* boxtab8, int nb, int* rowdesc, int* row2box, int* srcrow, void* stream);
int kg_seg_build_rows_levels(int nlev, const int* const* boxtab8, const int* nb, int* const* rowdesc, int* const* row2box, int* const* srcrow,
                             void* stream);   /* kg_seg_build_rows for all (<= 8) pyramid levels in one launch: HOST arrays of device pointers / box counts */
int kg_rows_gather(const void* src, int ldsrc, const int* srcrow, void* dst, int lddst, long nrows, int C, void* stream);
int kg_rows_gather_planes(const void* src, int ldsrc, int src_pstride, const int* srcrow, void* dst, int lddst, int dst_pstride, long nrows, int C,
                          int P, void* stream);     /* kg_rows_gather for the P planes of split rows in one launch (plane p at column p * pstride) */
/* seg_head.2 (KGnet.py:145-147: Conv2d(64, 1, 3, padding=1), used at KGnet.py:266): the one-output-channel 3x3 conv over the ragged pixel
 * list as a per-pixel dot product (zero padding at the box border, as each crop is convolved on its own).  x: rows [M][ldx], C = 64 channels
 * (planes: a); w: fp32 OIHW [1][64][3][3], the master parameter itself; bias: fp32 [1] or NULL; rowdesc: kg_seg_build_rows; y: fp32 [M] logits. */
int kg_seg_conv3_c1(const void* x, int ldx, int C, const float* w, const float* bias, const int* rowdesc, long M, float* y,
                    const kg_planes_t* planes, void* stream);
int kg_f32_to_bf16_rows(const float* acc, void* out, int C, long rows, int ldout, const void* addto, int ldadd,
                        void* stream);
/* crops of the fp32 feature maps forward_dec returns (KGnet.py:318 -> get_patches :246-256): dst (planes y) = src_f32[srcrow[r]] */
int kg_rows_gather_f32(const float* src, int ldsrc, const int* srcrow, void* dst, int lddst, long nrows, int C,
                       const kg_planes_t* planes, void* stream);
/* fp32 export of a rows tensor (planes a) -- the feature maps c0..c4 of forward_dec's return value (KGnet.py:318) -- and back
 * (planes y = acc (+ addto, planes b)): the gradients autograd hands forward_dec for them */
int kg_planes_to_f32(const void* x, int ldx, float* out, int ldout, long rows, int C, const kg_planes_t* planes, void* stream);
int kg_f32_to_planes(const float* acc, int ldacc, void* out, int ldout, const void* addto, int ldadd, long rows, int C,
                     const kg_planes_t* planes, void* stream);
/* gradient of get_patches' slicing (KGnet.py:246-256) w.r.t. a feature map, deterministic: out[n][y][x][0:C] (fp32, every
 * element written) = sum over the boxes containing (y, x), in ascending box order, of their crop-gradient row.  Rows
 * [0, rows_a) of the ragged list are read from ga, the others from gb (row r - rows_a); boxtab = {n,y1,x1,h,w,row0,H,W}
 * per box; bin_start / bin_boxes = CSR lists of the boxes touching each bin_size x bin_size bin of each image.
 * planes: a = ga, b = gb */
int kg_crop_grad_reduce(const void* ga, int lda, const void* gb, int ldb, long rows_a, const int* boxtab, const int* bin_start,
                        const int* bin_boxes, int bin_size, int N, int H, int W, int C, float* out, void* out_rows, int ldout,
                        const kg_planes_t* planes, void* stream);   /* exactly one of out (fp32) / out_rows (split-bf16 rows, planes y) */


/* ---- mask paste-back of the inference driver (test.py:127-157): cv2.resize(patch, box size) -> paste into a zero
 * (input_h, input_w) mask -> cv2.resize(mask, (image_w, image_h)) -> mask >= seg_thresh, for all detections in one launch.
 * flat = forward_seg's fp32 patch probabilities; dets = device int32 [nd][8] {patch offset, patch h, patch w, y1, x1, y2, x2, 0}
 * (box rounded / clamped as test.py:138-141); out = [nd][image_h][image_w] float32 (out_is_u8 = 0) or bytes.  The interpolation
 * is OpenCV's published generic INTER_LINEAR float path (oracle/paste.py) ---- */
int kg_mask_paste(const float* flat, const int* dets, int nd, int input_h, int input_w, int image_h, int image_w,
                  float seg_thresh, void* out, int out_is_u8, void* stream);
/* the same masks in the bit-mask layout above: words = device [nd][ld_words], bit-identical to kg_mask_paste's thresholded pixels
 * (same per-pixel expression; a 64-pixel word that cannot reach the detection's box is stored without evaluating it) */
int kg_mask_paste_bits(const float* flat, const int* dets, int nd, int input_h, int input_w, int image_h, int image_w,
                       float seg_thresh, void* words, long ld_words, void* stream);

/* ---- gradient scale of the half-precision backward pass (csrc/gradscale.hip) ----
 * kg_grad_scale: out[0] = S = 2^(target_log2 - e), out[1] = 1 / S, where max |v| over the n <= 24 fp32 device tensors
 * ptrs[i][0 .. counts[i]) (host arrays of device pointers / counts) = f * 2^e, f in [0.5, 1); S = 1 when the maximum is 0 or not
 * finite.  probs (optional host array, entries may be NULL): sigmoid outputs -- the value taken is then v * q * (1 - q), the gradient
 * w.r.t. the logit (what kg_grad_pack stores).  scratch: 2 zero-initialised unsigned on the device (left zeroed).  The tensors are the gradients of the loss w.r.t.
 * the network outputs (12 head maps + the seg probabilities: what `loss.backward()` hands to KGnet.forward's node, train.py:153).
 * kg_scale_tensors: multiplies njobs fp32 tensors by a device scalar each in ONE launch: jobs = device array of 32-byte records
 * {float* p; long n; const float* scale; int blk0; int pad;} (blk0 = first workgroup of the job, 4096 elements per workgroup).
 * kg_rows_rescale (re-normalisation point of the backward pass: a complete gradient rows tensor, csrc/norm_pool.hip): r = the power of
 * two <= 1 that brings max |g| of the rows tensor back into [2^(t-1), 2^t) when it exceeds 2^t (r = 1 otherwise: the scale only ever goes
 * down); g *= r in place; cum_out = {cum_in[0] * r, 1 / (cum_in[0] * r)}, r_out[0] = r (all on the device).  kg_rows_scale: rows *= *r (* *r2:
 * a gradient written under an earlier scale is converted with scale_now and 1 / scale_then) in place; kg_rows_scale_multi: the same for
 * up to 8 rows tensors in one launch: desc = host int64 [n][6] rows {pointer, ld, M, C, planes, plane stride}.  planes: a = g. */
int kg_grad_scale(const void* const* ptrs, const void* const* probs, const long* counts, int n, int target_log2, void* scratch, float* out, void* stream);
int kg_scale_tensors(const void* jobs, int njobs, int total_blocks, int* nonfinite, void* stream);   /* nonfinite: optional device int, set to 1 on an inf / NaN result */
int kg_rows_rescale(void* g, int ld, long M, int C, int target_log2, const float* cum_in, float* cum_out, float* r_out, void* scratch,
                    const kg_planes_t* planes, void* stream);
int kg_rows_scale(void* g, int ld, long M, int C, const float* r, const float* r2, const kg_planes_t* planes, void* stream);   /* *= *r * (r2 ? *r2 : 1) */
int kg_rows_scale_multi(const long* desc, int n, const float* r, const float* r2, void* stream);

#ifdef __cplusplus
}
#endif
#endif
