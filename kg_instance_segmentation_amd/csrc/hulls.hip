// hulls.hip -- the convex hull of every instance of a label map on gfx950 (hulls.py).
//   kg_label_hulls  per job {img, id, box, vert_at, cap}: the row {area, count, area2, feret_max2, fmax_i, fmax_j, minw_num, minw_den2,
//                   minw_edge, status} and the ring of strict hull vertices into verts[vert_at .. vert_at + min(count, cap)) as (y, x)
//
// Semantics (include/kgnet_hip.h is the normative text).  P = the pixels of the clamped box with labels == id; C(P) = the four lattice
// corners of every pixel of P; the ring is the convex hull of C(P), strict vertices only, clockwise on the screen (positive area2) from
// the vertex with the smallest (Y, X).  EXTENT FORM: with L(Y) / R(Y) the smallest / largest X of a corner of C(P) on lattice line Y
// (defined where box row Y - 1 or Y holds a pixel of P), the ring is (top, L(top)), the vertices of the upper concave envelope of R from
// top to bottom, the vertices of the lower convex envelope of L from bottom to top without the start.  Line i is a vertex of the L
// chain iff its largest slope to a defined line above is strictly below its smallest slope to a defined line below (the other way round
// for R); slopes are rationals compared by cross-multiplication (exact: the bounds are at ENVELOPE below).
//
// One block per job (the grid strides when there are more jobs than KG_LABEL_MAX_BLOCKS), 256 threads, 33 KiB of LDS:
//   EXTENTS   the box as one flat row-major list (consecutive lanes, consecutive x).  A pixel of P whose left (right) neighbour in the box
//             row is not in P -- the ballot of the wave says so, a second load only for lanes 0 and 63 -- is the head (tail) of a run:
//             only heads and tails issue LDS integer min / max, on the two lattice lines their row touches.  The area is the sum of the
//             ballots' popcounts.  No global atomics.
//   ENVELOPE  lanes take lattice lines in chunks of 256; a lane scans the lines above and below its own (two loops with wave-uniform
//             bounds, so every LDS read is a broadcast) and keeps the extreme slopes.  The ballots of the two vertex predicates go to LDS,
//             one 64-bit word per wave and chunk.
//   COMPACT   popcounts of those words -- below the lane, of the waves before, a carry across chunks -- give every vertex its index in
//             its chain.  The chains are compacted IN PLACE over the extents (index <= line, one barrier between the reads and the writes
//             of a chunk), a vertex packed as (line << 16 | x), box-local.  Ring position p is lo[0] for p == 0, hi[p - 1] for p <= nR,
//             lo[count - p] beyond: the right chain by a prefix count, the left chain by the totals minus a prefix count.
//   STATS     the ring stays in LDS (the slab of the table may be shorter than the ring: status 2 still has the right statistics).
//             Thread i owns vertex i and edge i and walks all vertices u (broadcast reads): the shoelace term, the farthest u > i, the
//             largest |cross| of the edge.  The pair (largest d2, then smallest (i, j)) and the edge (smallest c^2 / d compared as
//             c_a^2 d_b < c_b^2 d_a in 128 bits, then smallest k) are total orders, carried through shuffles and four LDS partials.
//
// The index rule of label_common.h holds here, with ONE new exception of the run-slot kind: the vertex slot is vert_at of the job table
// plus a prefix count of predicates, and a store happens only inside the unsigned predicates k < cap and vert_at + k < V.  LDS indices
// are box rows (< 4096 by the height rule), chain indices (<= the line they come from) and ring positions (< count <= 2 * lines).  No
// address depends on a label.
#include "label_common.h"

#define KG_HL_LINES 4096                // lattice lines of one job: a box of at most 4095 rows

// edge a is narrower than edge b: c_a^2 / d_a < c_b^2 / d_b, a tie to the smaller k; k < 0 is "no edge".  c < 2^31 and d < 2^32, so
// c^2 fits 64 bits and c^2 * d needs up to 94: the two products are compared as (high, low) pairs of 64 x 64 -> 128 bit multiplies.
__device__ __forceinline__ bool kg_hl_narrower(unsigned long long ca, unsigned long long da, int ka, unsigned long long cb,
                                               unsigned long long db, int kb) {
    if (ka < 0) return false;
    if (kb < 0) return true;
    const unsigned long long a2 = ca * ca, b2 = cb * cb;
    const unsigned long long ah = __umul64hi(a2, db), al = a2 * db, bh = __umul64hi(b2, da), bl = b2 * da;
    if (ah != bh) return ah < bh;
    if (al != bl) return al < bl;
    return ka < kb;
}
// pair a is better than pair b: the larger squared distance, a tie to the lexicographically smaller (i, j); d2 < 0 is "no pair"
__device__ __forceinline__ bool kg_hl_farther(int da, int ia, int ja, int db, int ib, int jb) {
    if (da != db) return da > db;
    return ia < ib || (ia == ib && ja < jb);
}

__global__ __launch_bounds__(256) void label_hulls_kernel(const int* __restrict__ labels, int nimg, int H, int W, const int* __restrict__ jobs,
                                                          int m, long long* __restrict__ rows, int* __restrict__ verts, long long V) {
    __shared__ __align__(16) int lo[KG_HL_LINES];                                    // L of every lattice line, then the left chain
    __shared__ __align__(16) int hi[KG_HL_LINES];                                    // R of every lattice line, then the right chain
    __shared__ unsigned long long vbits[2][KG_HL_LINES / 64];          // the vertex predicates of R and L, one word per 64 lines
    __shared__ long long part[4][8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int4* lo4 = (const int4*)lo;
    const int4* hi4 = (const int4*)hi;
    for (long j = blockIdx.x; j < m; j += gridDim.x) {
        const int* jb = jobs + j * 8;
        const int img = jb[0], id = jb[1];
        KgBox box = kg_job_box(jb + 2, H, W);
        if (!((unsigned)img < (unsigned)nimg)) box.h = box.w = 0;      // the only use of img before it scales an address
        const long base = (long)img * H * W;                           // used only with a non-empty box: img < nimg
        const long long vert_at = jb[6];
        const int cap = jb[7] > 0 ? jb[7] : 0;
        long long* row = rows + 10 * j;
        const bool live = box.h > 0 && box.w > 0, tall = live && box.h >= KG_HL_LINES;
        if (!live || tall) {                                           // the same in every thread
            if (tid < 10) row[tid] = tid == 9 && tall ? 1 : 0;
            continue;
        }
        const int h = box.h, w = box.w, nl = h + 1, nw = (nl + 63) >> 6;   // nl <= 4096 lines, nw <= 64 words
        __syncthreads();                                               // the job before has been read
        for (int y = tid; y < ((nl + 3) & ~3); y += 256) { lo[y] = INT_MAX; hi[y] = -1; }        // <= KG_HL_LINES entries
        __syncthreads();

        // ---- EXTENTS
        int cnt = 0;                                                   // the same in every lane of a wave
        {
            const int total = h * w;                                   // < 2^27
            const int sy = 256 / w, sx = 256 - sy * w;
            int yy = tid / w, xx = tid - yy * w;
            for (int e0 = 0; e0 < total; e0 += 256) {
                const bool on = e0 + tid < total;                      // yy < h: inside the box, hence inside the map
                const long p = base + (long)(box.y1 + yy) * W + (box.x1 + xx);
                bool in = false;
                if (on) in = labels[p] == id;
                const unsigned long long b = __ballot(in);
                cnt += __popcll(b);
                if (in) {                                              // lane - 1 / lane + 1 hold the neighbours of the box row
                    bool left = false, right = false;
                    if (xx > 0) left = lane == 0 ? labels[p - 1] == id : (b >> (lane - 1)) & 1ull;
                    if (xx < w - 1) right = lane == 63 ? labels[p + 1] == id : (b >> (lane + 1)) & 1ull;
                    if (!left) { atomicMin(&lo[yy], xx); atomicMin(&lo[yy + 1], xx); }              // yy + 1 <= h < KG_HL_LINES
                    if (!right) { atomicMax(&hi[yy], xx + 1); atomicMax(&hi[yy + 1], xx + 1); }
                }
                xx += sx; yy += sy;
                if (xx >= w) { xx -= w; ++yy; }
            }
        }
        if (lane == 0) part[wave][0] = cnt;
        __syncthreads();
        const long long area = part[0][0] + part[1][0] + part[2][0] + part[3][0];
        if (area == 0) {                                               // the box does not hold the id
            if (tid < 10) row[tid] = 0;
            continue;
        }

        // ---- ENVELOPE: slopes n / d with 0 < d < 2^12 and |n| < 2^16 (a sentinel: 2^17), so a cross product stays below 2^29: the
        // 24-bit multiply gives the very number the int64 product of the statement gives, at the full vector rate
        for (int c0 = 0; c0 < nl; c0 += 256) {
            const int Y = c0 + tid, w0 = c0 + (wave << 6);             // w0: the first line of the wave
            const int Li = Y < nl ? lo[Y] : INT_MAX, Ri = Y < nl ? hi[Y] : -1;
            int lan = -(1 << 17), lad = 1, lbn = 1 << 17, lbd = 1;     // L: the largest slope above, the smallest below
            int ran = 1 << 17, rad = 1, rbn = -(1 << 17), rbd = 1;     // R: the smallest slope above, the largest below
            const int above_end = w0 + 63 < nl ? w0 + 63 : w0 < nl ? nl : 0;        // a wave past the last line scans nothing
            auto above = [&](int q, int Lq, int Rq) {
                if (Lq != INT_MAX && q < Y) {
                    const int d = Y - q, nL = Li - Lq, nR = Ri - Rq;
                    if (__mul24(nL, lad) > __mul24(lan, d)) { lan = nL; lad = d; }
                    if (__mul24(nR, rad) < __mul24(ran, d)) { ran = nR; rad = d; }
                }
            };
            auto under = [&](int q, int Lq, int Rq) {
                if (Lq != INT_MAX && q > Y) {
                    const int d = q - Y, nL = Lq - Li, nR = Rq - Ri;
                    if (__mul24(nL, lbd) < __mul24(lbn, d)) { lbn = nL; lbd = d; }
                    if (__mul24(nR, rbd) > __mul24(rbn, d)) { rbn = nR; rbd = d; }
                }
            };
            // four lines per 16-byte LDS read: the lines from nl up to the next multiple of 4 are undefined (the fill above), and a line
            // on the wrong side of Y fails its predicate, so both loops may start and end on a multiple of 4
            for (int q = 0; q < above_end; q += 4) {
                const int4 l = lo4[q >> 2], r = hi4[q >> 2];
                above(q, l.x, r.x); above(q + 1, l.y, r.y); above(q + 2, l.z, r.z); above(q + 3, l.w, r.w);
            }
            for (int q = (w0 + 1) & ~3; q < nl; q += 4) {               // w0 + 1 >= nl for a wave past the last line
                const int4 l = lo4[q >> 2], r = hi4[q >> 2];
                under(q, l.x, r.x); under(q + 1, l.y, r.y); under(q + 2, l.z, r.z); under(q + 3, l.w, r.w);
            }
            const bool def = Li != INT_MAX;
            const unsigned long long bR = __ballot(def && __mul24(ran, rbd) > __mul24(rbn, rad));
            const unsigned long long bL = __ballot(def && __mul24(lan, lbd) < __mul24(lbn, lad));
            if (lane == 0) { vbits[0][(c0 >> 6) + wave] = bR; vbits[1][(c0 >> 6) + wave] = bL; }      // (c0 >> 6) + wave <= 63
        }
        __syncthreads();

        // ---- COMPACT
        int nR = 0, nL = 0;
        for (int k = 0; k < nw; ++k) { nR += __popcll(vbits[0][k]); nL += __popcll(vbits[1][k]); }
        const int count = nR + nL;
        {
            int cR = 0, cL = 0;                                        // the carries: the same in every thread
            for (int c0 = 0; c0 < nl; c0 += 256) {
                const int Y = c0 + tid;
                const int a = Y < nl ? lo[Y] : 0, b = Y < nl ? hi[Y] : 0;
                int pR = cR, pL = cL;
                unsigned long long mR = 0, mL = 0;
                for (int k = 0; k < 4; ++k) {
                    const int wk = (c0 >> 6) + k;
                    if (wk < nw) {
                        const unsigned long long r = vbits[0][wk], l = vbits[1][wk];
                        if (k < wave) { pR += __popcll(r); pL += __popcll(l); }
                        if (k == wave) { mR = r; mL = l; }
                        cR += __popcll(r); cL += __popcll(l);
                    }
                }
                pR += __popcll(mR & below); pL += __popcll(mL & below);
                __syncthreads();                                       // the lines of this chunk have been read
                if ((mR >> lane) & 1ull) hi[pR] = (Y << 16) | b;       // pR, pL <= Y: a line read in this chunk or before
                if ((mL >> lane) & 1ull) lo[pL] = (Y << 16) | a;
            }
        }
        __syncthreads();
        auto ring = [&](int p) -> int { return p <= nR ? (p ? hi[p - 1] : lo[0]) : lo[count - p]; };      // 0 <= p < count
        for (int p = tid; p < count; p += 256) {
            const unsigned long long at = (unsigned long long)(vert_at + p);
            if (p < cap && at < (unsigned long long)V) {
                const int v = ring(p);
                verts[2 * at] = box.y1 + (v >> 16); verts[2 * at + 1] = box.x1 + (v & 0xffff);
            }
        }

        // ---- STATS: box-local coordinates, y <= 4095 and x <= 32768, so a cross product stays below 2^28 and a squared distance
        // below 2^31; the shoelace sum alone takes absolute coordinates
        long long a2 = 0;
        int fd = -1, fi = 0, fj = 0;
        unsigned long long wc = 0, wd = 0;
        int wk = -1;
        for (int i0 = 0; i0 < count; i0 += 256) {
            const int i = i0 + tid;
            const bool on = i < count;
            int y0 = 0, x0 = 0, ey = 0, ex = 0;
            if (on) {
                const int v0 = ring(i), v1 = ring(i + 1 == count ? 0 : i + 1);
                y0 = v0 >> 16; x0 = v0 & 0xffff;
                ey = (v1 >> 16) - y0; ex = (v1 & 0xffff) - x0;
                a2 += (long long)(box.x1 + x0) * (box.y1 + y0 + ey) - (long long)(box.x1 + x0 + ex) * (box.y1 + y0);
            }
            int dbest = -1, jbest = 0, cmax = 0;
            auto visit = [&](int u, int v) {
                const int uy = (v >> 16) - y0, ux = (v & 0xffff) - x0;
                const int d2 = uy * uy + ux * ux;
                if (u > i && d2 > dbest) { dbest = d2; jbest = u; }    // u ascends: the smallest j of a tie stays
                int cr = ex * uy - ey * ux;
                cr = cr < 0 ? -cr : cr;
                cmax = cr > cmax ? cr : cmax;
            };
            visit(0, lo[0]);
            for (int u = 1; u <= nR; ++u) visit(u, hi[u - 1]);
            for (int u = nR + 1; u < count; ++u) visit(u, lo[count - u]);
            if (on) {
                if (dbest >= 0 && kg_hl_farther(dbest, i, jbest, fd, fi, fj)) { fd = dbest; fi = i; fj = jbest; }
                const unsigned long long c = (unsigned long long)cmax, d = (unsigned long long)((long long)ex * ex + (long long)ey * ey);
                if (kg_hl_narrower(c, d, i, wc, wd, wk)) { wc = c; wd = d; wk = i; }
            }
        }
        a2 = kg_wave_sum(a2);
        for (int o = 32; o; o >>= 1) {
            const int td = __shfl_xor(fd, o), ti = __shfl_xor(fi, o), tj = __shfl_xor(fj, o);
            if (kg_hl_farther(td, ti, tj, fd, fi, fj)) { fd = td; fi = ti; fj = tj; }
            const unsigned long long tc = __shfl_xor(wc, o), tw = __shfl_xor(wd, o);
            const int tk = __shfl_xor(wk, o);
            if (kg_hl_narrower(tc, tw, tk, wc, wd, wk)) { wc = tc; wd = tw; wk = tk; }
        }
        if (lane == 0) {
            part[wave][1] = a2; part[wave][2] = fd; part[wave][3] = fi; part[wave][4] = fj;
            part[wave][5] = (long long)wc; part[wave][6] = (long long)wd; part[wave][7] = wk;
        }
        __syncthreads();
        if (tid == 0) {
            for (int k = 1; k < 4; ++k) {
                a2 += part[k][1];
                if (kg_hl_farther((int)part[k][2], (int)part[k][3], (int)part[k][4], fd, fi, fj)) {
                    fd = (int)part[k][2]; fi = (int)part[k][3]; fj = (int)part[k][4];
                }
                if (kg_hl_narrower((unsigned long long)part[k][5], (unsigned long long)part[k][6], (int)part[k][7], wc, wd, wk)) {
                    wc = (unsigned long long)part[k][5]; wd = (unsigned long long)part[k][6]; wk = (int)part[k][7];
                }
            }
            row[0] = area; row[1] = count; row[2] = a2; row[3] = fd; row[4] = fi; row[5] = fj;
            row[6] = (long long)wc; row[7] = (long long)wd; row[8] = wk; row[9] = count > cap ? 2 : 0;
        }
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// labels: device int32 [nimg][H][W]; jobs: device int32 [m][8] = (img, id, y1, x1, y2, x2, vert_at, cap), written by the caller;
// rows: device int64 [m][10]; verts: device int32 [V][2] = (y, x)
extern "C" int kg_label_hulls(const int* labels, int nimg, int H, int W, const int* jobs, int m, long long* rows, int* verts, int V,
                              void* stream) {
    const char* fn = "kg_label_hulls";
    KG_TRY(kg_check_job_stack(fn, labels, nimg, H, W, jobs, m));       // H, W <= KG_LABEL_MAX_SIDE: a box-local x fits the 16 bits of a packed vertex
    KG_CHECK_ARG(V >= 0, "%s: bad size (V %d)", fn, V);
    KG_CHECK_ARG(rows || m == 0, "%s: null pointer (rows)", fn);
    KG_CHECK_ARG(verts || V == 0, "%s: null pointer (verts)", fn);
    KG_CHECK_ARG(kg_aligned(rows, 7) && kg_aligned(verts, 3), "%s: misaligned pointer", fn);
    const long lbytes = 4L * nimg * H * W;
    KG_CHECK_ARG(!rows || kg_apart(rows, 80L * m, labels, lbytes), "%s: rows aliases labels", fn);
    KG_CHECK_ARG(!verts || kg_apart(verts, 8L * V, labels, lbytes), "%s: verts aliases labels", fn);
    KG_CHECK_ARG(!rows || !verts || kg_apart(rows, 80L * m, verts, 8L * V), "%s: rows aliases verts", fn);
    KG_CHECK_ARG(!rows || !jobs || kg_apart(rows, 80L * m, jobs, 32L * m), "%s: rows aliases jobs", fn);
    KG_CHECK_ARG(!verts || !jobs || kg_apart(verts, 8L * V, jobs, 32L * m), "%s: verts aliases jobs", fn);
    if (m == 0) return KG_OK;
    hipLaunchKernelGGL(label_hulls_kernel, dim3(kg_grid_cap(m)), dim3(256), 0, (hipStream_t)stream, labels, nimg, H, W, jobs, m, rows, verts,
                       (long long)V);
    KG_CHECK_LAUNCH("label_hulls");
    return KG_OK;
}
