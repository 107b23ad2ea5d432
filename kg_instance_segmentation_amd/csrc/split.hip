// split.hip -- merged instances of a label map split on gfx950 (split.py): the seeded geodesic regrow inside every instance.
//   kg_label_split  out = labels, then per job {img, id, box, nseeds, first_new}: every pixel of P (the pixels of the clamped box with
//                   labels == id) goes to the seed of smallest rank among the geodesically nearest ones; the pixels of the ranks r >= 2
//                   are stored as first_new + r - 2, and the row {members, unreached, levels, status} is written
//
// Semantics (include/kgnet_hip.h is the normative text).  g(p, s) = the steps of the shortest c-connected path inside P from p to seed s;
// p takes the smallest rank among the seeds with the smallest finite g(p, s); a pixel no seed reaches counts as unreached and keeps the
// id, as rank 1 does.  A seeds value outside 1 .. min(nseeds, KG_SP_MAX_RANK), or on a pixel that is not in P, is 0.
//
// One block per job (the grid strides when there are more jobs than KG_LABEL_MAX_BLOCKS), 256 threads, 32 KiB of LDS:
//   STATE     one 16-bit cell per pixel of the box plus a one-pixel zero halo: pitch w + 2, h + 2 rows, pixel (yy, xx) of the box at
//             (yy + 1) * (w + 2) + xx + 1, so a neighbour read needs no bounds test.  0 = not in P (the halo too); else bits 0 .. 13 = the
//             rank, KG_SP_OPEN (all ones) while unassigned, and bits 14 .. 15 = the tag: 0 settled, 1 / 2 assigned in an even / odd level.
//   FLOOD     level-synchronous and exact, ONE barrier per level.  In level L (tag t = (L & 1) + 1) a thread walks its own cells.  An open
//             cell takes the smallest rank over its neighbours that are assigned and do NOT carry tag t -- the cells assigned before level
//             L, whatever the other threads do meanwhile: a neighbour can only change from open to tag t (ignored either way) or from the
//             other tag to settled (the same rank either way).  The owner clears the tag of the cells it assigned in level L - 1 during
//             its walk of level L, behind the barrier that ended L - 1 and before tag t comes round again in L + 2.  A thread with no open
//             cell and no tag to clear skips its walk.  Only the owner of a cell writes it.
//   END       __syncthreads_or of "I assigned a cell" is workgroup-uniform: the flood ends with the first level that assigns nothing, and
//             after h * w levels at the latest (every level but the last assigns a pixel).
//   STORE     the box is walked once more: a cell of rank r >= 2 stores first_new + r - 2, an open cell counts as unreached.  out was
//             filled as a copy of labels by the entry, on the stream, so every element is written; two jobs of one image with different
//             ids never store the same pixel.
//
// The index rule of label_common.h holds here WITHOUT a new exception: every LDS index is a box-local coordinate (plus a fixed
// neighbour offset, inside the halo), never a label, a seed or a rank; the job table's box is clamped before any address is formed, its
// image index is used only inside (unsigned)img < (unsigned)nimg, and nseeds / first_new are a predicate bound and a stored value.  No
// atomics, no global scratch.
#include "label_common.h"

#define KG_SP_CELLS 16384               // the LDS budget: (h + 2) * (w + 2) cells of 16 bits, 32 KiB
#define KG_SP_OPEN 0x3fff               // the rank field of a pixel of P that no seed has reached yet
#define KG_SP_MAX_RANK 16382            // h * w <= 126 * 126 < KG_SP_MAX_RANK for every box that fits: no seed list of distinct pixels is cut

template <bool CONN8>
__global__ __launch_bounds__(256) void label_split_kernel(const int* __restrict__ labels, const int* __restrict__ seeds, int nimg, int H, int W,
                                                          const int* __restrict__ jobs, int m, int* __restrict__ out, int* __restrict__ rows) {
    __shared__ __align__(16) unsigned short st[KG_SP_CELLS];
    __shared__ int part[4][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned* st32 = (unsigned*)st;
    for (long j = blockIdx.x; j < m; j += gridDim.x) {
        const int* jb = jobs + j * 8;
        const int img = jb[0], id = jb[1];
        KgBox box = kg_job_box(jb + 2, H, W);
        if (!((unsigned)img < (unsigned)nimg)) box.h = box.w = 0;      // the only use of img before it scales an address
        const long base = (long)img * H * W;                           // used only with a non-empty box: img < nimg
        const int ns = jb[6] < 0 ? 0 : jb[6] > KG_SP_MAX_RANK ? KG_SP_MAX_RANK : jb[6];
        const unsigned first_new = (unsigned)jb[7];
        int* row = rows + 4 * j;
        const int pitch = box.w + 2;
        const int cells = (box.h + 2) * pitch;                         // h, w <= 2^15: below 2^31
        if (cells > KG_SP_CELLS) {                                     // the size rule: the job is left as copied
            if (tid < 4) row[tid] = tid == 3;
            continue;
        }
        for (int i = tid; i < (cells + 1) >> 1; i += 256) st32[i] = 0u;
        __syncthreads();
        int members = 0, open = 0;
        kg_box_walk(box, [&](int Y, int X) {
            const long p = base + (long)Y * W + X;
            if (labels[p] == id) {
                const int s = seeds[p];
                const bool seeded = (unsigned)(s - 1) < (unsigned)ns;
                st[(Y - box.y1 + 1) * pitch + (X - box.x1 + 1)] = (unsigned short)(seeded ? s : KG_SP_OPEN);
                ++members; open += !seeded;
            }
        });
        __syncthreads();
        const int limit = box.h * box.w;
        int level = 0;
        bool pending = false;                                          // this thread assigned a cell in the level before: a tag to clear
        while (level < limit) {
            const int tag = (level & 1) + 1;
            int changed = 0;
            if (open > 0 || pending) {
                bool fresh = false;
                kg_box_walk(box, [&](int Y, int X) {
                    const int i = (Y - box.y1 + 1) * pitch + (X - box.x1 + 1);
                    const int c = st[i];
                    const int r = c & KG_SP_OPEN, t = c >> 14;
                    if (c == 0) return;
                    if (r == KG_SP_OPEN) {
                        int best = KG_SP_OPEN;
                        auto look = [&](int k) {
                            const int v = st[k];
                            const int rv = v & KG_SP_OPEN;
                            if (rv != 0 && (v >> 14) != tag && rv < best) best = rv;
                        };
                        look(i - pitch); look(i - 1); look(i + 1); look(i + pitch);
                        if (CONN8) { look(i - pitch - 1); look(i - pitch + 1); look(i + pitch - 1); look(i + pitch + 1); }
                        if (best != KG_SP_OPEN) {
                            st[i] = (unsigned short)((tag << 14) | best);
                            changed = 1; fresh = true; --open;
                        }
                    } else if (t != 0 && t != tag) {
                        st[i] = (unsigned short)r;
                    }
                });
                pending = fresh;
            }
            if (!__syncthreads_or(changed)) break;
            ++level;
        }
        int unreached = 0;
        kg_box_walk(box, [&](int Y, int X) {
            const int r = st[(Y - box.y1 + 1) * pitch + (X - box.x1 + 1)] & KG_SP_OPEN;
            unreached += r == KG_SP_OPEN;
            if (r >= 2 && r != KG_SP_OPEN) out[base + (long)Y * W + X] = (int)(first_new + (unsigned)(r - 2));
        });
        members = kg_wave_sum(members); unreached = kg_wave_sum(unreached);
        if (lane == 0) { part[wave][0] = members; part[wave][1] = unreached; }
        __syncthreads();
        if (tid == 0) {
            row[0] = part[0][0] + part[1][0] + part[2][0] + part[3][0];
            row[1] = part[0][1] + part[1][1] + part[2][1] + part[3][1];
            row[2] = level;
            row[3] = 0;
        }
        __syncthreads();                                               // st and part are written again by the block's next job
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// labels, seeds: device int32 [nimg][H][W]; jobs: device int32 [m][8] = (img, id, y1, x1, y2, x2, nseeds, first_new), written by the
// caller; out: device int32 [nimg][H][W]; rows: device int32 [m][4]
extern "C" int kg_label_split(const int* labels, const int* seeds, int nimg, int H, int W, int connectivity, const int* jobs, int m, int* out,
                              int* rows, void* stream) {
    const char* fn = "kg_label_split";
    KG_TRY(kg_check_job_stack(fn, labels, nimg, H, W, jobs, m));
    KG_CHECK_ARG(connectivity == 4 || connectivity == 8, "%s: connectivity %d (4 or 8)", fn, connectivity);
    KG_CHECK_ARG(seeds && out, "%s: null pointer (seeds / out)", fn);
    KG_CHECK_ARG(rows || m == 0, "%s: null pointer (rows)", fn);
    KG_CHECK_ARG(kg_aligned(seeds, 3) && kg_aligned(out, 3) && kg_aligned(rows, 3), "%s: misaligned pointer", fn);
    const long lbytes = 4L * nimg * H * W;
    KG_CHECK_ARG(kg_apart(out, lbytes, labels, lbytes) && kg_apart(out, lbytes, seeds, lbytes), "%s: out aliases labels / seeds", fn);
    KG_CHECK_ARG(!rows || (kg_apart(rows, 16L * m, labels, lbytes) && kg_apart(rows, 16L * m, seeds, lbytes) &&
                           kg_apart(rows, 16L * m, out, lbytes)), "%s: rows aliases a map", fn);
    KG_CHECK_ARG(!jobs || (kg_apart(jobs, 32L * m, out, lbytes) && kg_apart(jobs, 32L * m, rows, 16L * m)), "%s: jobs aliases out / rows", fn);
    hipStream_t s = (hipStream_t)stream;
    KG_HIP(hipMemcpyAsync(out, labels, (size_t)lbytes, hipMemcpyDeviceToDevice, s));
    if (m == 0) return KG_OK;
    if (connectivity == 8)
        hipLaunchKernelGGL(label_split_kernel<true>, dim3(kg_grid_cap(m)), dim3(256), 0, s, labels, seeds, nimg, H, W, jobs, m, out, rows);
    else
        hipLaunchKernelGGL(label_split_kernel<false>, dim3(kg_grid_cap(m)), dim3(256), 0, s, labels, seeds, nimg, H, W, jobs, m, out, rows);
    KG_CHECK_LAUNCH("label_split");
    return KG_OK;
}
