// thinning.hip -- the midline of every instance of a label map on gfx950 (thinning.py): exact parallel thinning, 32 pixels per instruction.
//   kg_label_thin   skel = 0, then per job {img, id, y1, x1, y2, x2}: P (the pixels of the clamped box with labels == id) is thinned by
//                   Guo-Hall's rule until a pass deletes nothing (or max_passes have run); id is stored on what remains, S, and the row
//                   {members, pixels, isolated, ends, junctions, ortho, diag, passes, status} is written
//
// Semantics (include/kgnet_hip.h is the normative text).  Neighbours clockwise from north, P2 = N .. P9 = NW.  A pass is two fully
// synchronous sub-iterations; a set pixel is deleted iff C == 1 and 2 <= min(N1, N2) <= 3 and m == 0, with
//   C  = (!P2 & (P3|P4)) + (!P4 & (P5|P6)) + (!P6 & (P7|P8)) + (!P8 & (P9|P2))
//   N1 = (P9|P2) + (P3|P4) + (P5|P6) + (P7|P8),   N2 = (P2|P3) + (P4|P5) + (P6|P7) + (P8|P9)
//   m  = (P6 | P7 | !P9) & P8 in the first sub-iteration, (P2 | P3 | !P5) & P4 in the second.
//
// One block per job (the grid strides when there are more jobs than KG_LABEL_MAX_BLOCKS), 256 threads, 32 KiB of LDS:
//   STATE     two bitmaps of 16 KiB, one bit per pixel of the box plus a one-pixel zero halo: pitch pw = ceil((w + 2) / 32) words,
//             h + 2 rows, pixel (yy, xx) of the box at bit (xx + 1) & 31 of word (yy + 1) * pw + ((xx + 1) >> 5).  Both are zeroed for every
//             job, halo and pad bits included, before the fill; the fill takes 64 bits of a row per wave from a ballot, so a word has one
//             writer and no atomic is needed.
//   PASS      a thread owns whole words (flat over h * pw, consecutive lanes on consecutive words: no bank conflict).  It reads its word
//             and the eight around it -- the left / right word of a row is 0 at k == 0 / k == pw - 1, never the neighbouring row's --,
//             forms the eight neighbour planes by shifts with the carry bits, evaluates the rule as a Boolean circuit (C == 1 as
//             exactly-one of four bits, the N condition as N1 >= 2 & N2 >= 2 & (N1 <= 3 | N2 <= 3) from two-bit adders), masks the halo
//             and pad bits and writes the other bitmap.  ONE barrier per sub-iteration is enough: a sub-iteration reads one bitmap and
//             writes the other, every owned word is written every time, and the barrier separates the last read of a bitmap from its
//             next write.
//   END       __syncthreads_or of "I deleted a bit" is the second barrier of a pass and workgroup-uniform: the loop ends with the first
//             pass that deletes nothing, after max_passes, and after h * w passes at the latest (every other pass deletes a pixel).
//   COUNTS    popcounts of plane expressions over the owned words, wave sums, four partials.
//   STORE     the owned words are walked once more: a set bit stores id at its box coordinate.  skel was zeroed by the entry, on the
//             stream, so every element is written.
//
// The index rule of label_common.h holds here WITHOUT a new exception: every LDS index is a box-local coordinate plus a fixed offset
// inside the halo, never a label; the predicate of the store is an LDS bit (masked to the box's columns) and its address a box
// coordinate; the job table's box is clamped before any address is formed and its image index is used only inside
// (unsigned)img < (unsigned)nimg.  No atomics, no global scratch, plain C++ and vector memory operations only.
#include "label_common.h"

#define KG_TH_WORDS 4096                // the LDS budget of ONE bitmap: (h + 2) * pw words of 32 bits, 16 KiB

struct KgThPlanes { unsigned c, p2, p3, p4, p5, p6, p7, p8, p9; };
// the word at i = r * pw + k and its eight neighbour planes; r - 1 and r + 1 are rows of the bitmap (the halo rows at the least)
__device__ __forceinline__ KgThPlanes kg_th_planes(const unsigned* bm, int i, int k, int pw) {
    const bool l = k > 0, r = k + 1 < pw;                              // the zero halo, not the neighbouring row
    const unsigned al = l ? bm[i - pw - 1] : 0u, ac = bm[i - pw], ar = r ? bm[i - pw + 1] : 0u;
    const unsigned cl = l ? bm[i - 1] : 0u, cc = bm[i], cr = r ? bm[i + 1] : 0u;
    const unsigned bl = l ? bm[i + pw - 1] : 0u, bc = bm[i + pw], br = r ? bm[i + pw + 1] : 0u;
    KgThPlanes p;
    p.c = cc;
    p.p2 = ac; p.p3 = (ac >> 1) | (ar << 31); p.p9 = (ac << 1) | (al >> 31);
    p.p4 = (cc >> 1) | (cr << 31); p.p8 = (cc << 1) | (cl >> 31);
    p.p6 = bc; p.p5 = (bc >> 1) | (br << 31); p.p7 = (bc << 1) | (bl >> 31);
    return p;
}
// the bits of word k of a row that are pixels of the box: 1 <= 32 k + b <= w (bit 0 of word 0 is the halo column)
__device__ __forceinline__ unsigned kg_th_valid(int k, int w) {
    const int hi = w - 32 * k;
    if (hi < 0) return 0u;
    const unsigned upto = hi >= 31 ? ~0u : (2u << hi) - 1u;
    return k == 0 ? upto & ~1u : upto;
}
// the pixels the rule deletes in sub-iteration `second`
__device__ __forceinline__ unsigned kg_th_deleted(const KgThPlanes& p, bool second) {
    const unsigned a1 = p.p9 | p.p2, a2 = p.p3 | p.p4, a3 = p.p5 | p.p6, a4 = p.p7 | p.p8;       // the terms of N1 (and of C)
    const unsigned b1 = p.p2 | p.p3, b2 = p.p4 | p.p5, b3 = p.p6 | p.p7, b4 = p.p8 | p.p9;       // the terms of N2
    const unsigned c1 = ~p.p2 & a2, c2 = ~p.p4 & a3, c3 = ~p.p6 & a4, c4 = ~p.p8 & a1;
    const unsigned one = ((c1 ^ c2) ^ (c3 ^ c4)) & ~(c1 & c2) & ~(c3 & c4);                     // exactly one of the four
    const unsigned a_hi1 = a1 & a2, a_hi2 = a3 & a4, b_hi1 = b1 & b2, b_hi2 = b3 & b4;
    const unsigned a_ge2 = a_hi1 | a_hi2 | ((a1 ^ a2) & (a3 ^ a4)), b_ge2 = b_hi1 | b_hi2 | ((b1 ^ b2) & (b3 ^ b4));
    const unsigned n_ok = a_ge2 & b_ge2 & ~(a_hi1 & a_hi2 & b_hi1 & b_hi2);                      // N1 <= 3 | N2 <= 3
    const unsigned m = second ? (p.p2 | p.p3 | ~p.p5) & p.p4 : (p.p6 | p.p7 | ~p.p9) & p.p8;
    return p.c & one & n_ok & ~m;
}

__global__ __launch_bounds__(256) void label_thin_kernel(const int* __restrict__ labels, int nimg, int H, int W, const int* __restrict__ jobs, int m,
                                                         int max_passes, int* __restrict__ skel, int* __restrict__ rows) {
    __shared__ unsigned bm[2][KG_TH_WORDS];
    __shared__ int part[4][7];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (long j = blockIdx.x; j < m; j += gridDim.x) {
        const int* jb = jobs + j * 6;
        const int img = jb[0], id = jb[1];
        KgBox box = kg_job_box(jb + 2, H, W);
        if (!((unsigned)img < (unsigned)nimg)) box.h = box.w = 0;      // the only use of img before it scales an address
        const long base = (long)img * H * W;                           // used only with a non-empty box: img < nimg
        int* row = rows + 9 * j;
        const int pw = (box.w + 2 + 31) >> 5;
        const long cells = (long)(box.h + 2) * pw;                     // h, w <= 2^15
        if (box.h == 0 || box.w == 0 || cells > KG_TH_WORDS) {         // a bad job: zeros; the size rule: status 1, nothing stored
            if (tid < 9) row[tid] = tid == 8 && box.h > 0 && box.w > 0;
            continue;
        }
        const KgBox words = KgBox{1, 0, box.h, pw};                    // the owned words as a box: f(r, k), word r * pw + k
        for (int i = tid; i < (int)cells; i += 256) bm[0][i] = bm[1][i] = 0u;
        __syncthreads();
        int members = 0;
        {                                                              // the fill: a wave takes 64 bits of a row at a time
            const int cpr = (pw + 1) >> 1;
            int yy = 0, ch = wave;
            while (ch >= cpr) { ch -= cpr; ++yy; }
            while (yy < box.h) {
                const int xx = 64 * ch + lane - 1;
                const bool in = xx >= 0 && xx < box.w && labels[base + (long)(box.y1 + yy) * W + (box.x1 + xx)] == id;
                const unsigned long long bits = __ballot(in);
                if (lane < 2 && 2 * ch + lane < pw) bm[0][(yy + 1) * pw + 2 * ch + lane] = (unsigned)(bits >> (32 * lane));
                if (lane == 0) members += __popcll(bits);
                ch += 4;
                while (ch >= cpr) { ch -= cpr; ++yy; }
            }
        }
        __syncthreads();
        const int most = box.h * box.w;                                // <= 32 * KG_TH_WORDS
        const int limit = max_passes > 0 && max_passes < most ? max_passes : most;
        int passes = 0;
        while (passes < limit) {
            int deleted = 0;
            for (int sub = 0; sub < 2; ++sub) {
                const unsigned* src = bm[sub];
                unsigned* dst = bm[sub ^ 1];
                kg_box_walk(words, [&](int r, int k) {
                    const int i = r * pw + k;
                    unsigned now = src[i];
                    if (now) {
                        const unsigned del = kg_th_deleted(kg_th_planes(src, i, k, pw), sub == 1);
                        deleted |= del != 0u;
                        now = now & ~del & kg_th_valid(k, box.w);
                    }
                    dst[i] = now;
                });
                if (sub == 0) __syncthreads();
            }
            if (!__syncthreads_or(deleted)) break;
            ++passes;
        }
        int cnt[6] = {0, 0, 0, 0, 0, 0};                               // pixels, isolated, ends, junctions, ortho, diag
        kg_box_walk(words, [&](int r, int k) {
            const int i = r * pw + k;
            const unsigned s = bm[0][i] & kg_th_valid(k, box.w);
            if (!s) return;
            const KgThPlanes p = kg_th_planes(bm[0], i, k, pw);
            const unsigned nb[8] = {p.p2, p.p3, p.p4, p.p5, p.p6, p.p7, p.p8, p.p9};
            unsigned any = 0u, two = 0u, t1 = 0u, t2 = 0u, t3 = 0u;
            for (int q = 0; q < 8; ++q) {
                two |= any & nb[q]; any |= nb[q];
                const unsigned t = ~nb[q] & nb[(q + 1) & 7];           // a 0 -> 1 transition of the cyclic sequence P2 .. P9
                t3 |= t2 & t; t2 |= t1 & t; t1 |= t;
            }
            cnt[0] += __popc(s);
            cnt[1] += __popc(s & ~any);
            cnt[2] += __popc(s & any & ~two);
            cnt[3] += __popc(s & t3);
            cnt[4] += __popc(s & p.p4) + __popc(s & p.p6);
            cnt[5] += __popc(s & p.p5 & ~p.p4 & ~p.p6) + __popc(s & p.p7 & ~p.p8 & ~p.p6);
            const int Y = box.y1 + r - 1, x0 = box.x1 + 32 * k - 1;    // bit b of the word is box column 32 k + b - 1, inside [0, w)
            for (unsigned rest = s; rest; rest &= rest - 1u) skel[base + (long)Y * W + (x0 + __builtin_ctz(rest))] = id;
        });
        members = kg_wave_sum(members);
        for (int q = 0; q < 6; ++q) cnt[q] = kg_wave_sum(cnt[q]);
        if (lane == 0) {
            part[wave][0] = members;
            for (int q = 0; q < 6; ++q) part[wave][q + 1] = cnt[q];
        }
        __syncthreads();
        if (tid < 7) row[tid] = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
        if (tid == 7) row[7] = passes;
        if (tid == 8) row[8] = 0;
        __syncthreads();                                               // the bitmaps and part are written again by the block's next job
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// labels: device int32 [nimg][H][W]; jobs: device int32 [m][6] = (img, id, y1, x1, y2, x2), written by the caller; max_passes: 0 = until
// nothing is deleted; skel: device int32 [nimg][H][W]; rows: device int32 [m][9]
extern "C" int kg_label_thin(const int* labels, int nimg, int H, int W, const int* jobs, int m, int max_passes, int* skel, int* rows,
                             void* stream) {
    const char* fn = "kg_label_thin";
    KG_TRY(kg_check_job_stack(fn, labels, nimg, H, W, jobs, m));
    KG_CHECK_ARG(max_passes >= 0, "%s: max_passes %d (0 = no limit, or >= 1)", fn, max_passes);
    KG_CHECK_ARG(skel, "%s: null pointer (skel)", fn);
    KG_CHECK_ARG(rows || m == 0, "%s: null pointer (rows)", fn);
    KG_CHECK_ARG(kg_aligned(skel, 3) && kg_aligned(rows, 3), "%s: misaligned pointer", fn);
    const long lbytes = 4L * nimg * H * W;
    KG_CHECK_ARG(kg_apart(skel, lbytes, labels, lbytes), "%s: skel aliases labels", fn);
    KG_CHECK_ARG(!rows || (kg_apart(rows, 36L * m, labels, lbytes) && kg_apart(rows, 36L * m, skel, lbytes)), "%s: rows aliases a map", fn);
    KG_CHECK_ARG(!jobs || (kg_apart(jobs, 24L * m, skel, lbytes) && kg_apart(jobs, 24L * m, rows, 36L * m)), "%s: jobs aliases skel / rows", fn);
    hipStream_t s = (hipStream_t)stream;
    KG_HIP(hipMemsetAsync(skel, 0, (size_t)lbytes, s));
    if (m == 0) return KG_OK;
    hipLaunchKernelGGL(label_thin_kernel, dim3(kg_grid_cap(m)), dim3(256), 0, s, labels, nimg, H, W, jobs, m, max_passes, skel, rows);
    KG_CHECK_LAUNCH("label_thin");
    return KG_OK;
}
