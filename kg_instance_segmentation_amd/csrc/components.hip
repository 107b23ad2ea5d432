// components.hip -- connected components of an instance label map on gfx950 (components.py states the semantics in NumPy).
//   kg_label_components   label maps [nimg][H][W] -> comp (component number of every pixel, 1 .. m_i per image, 0 outside) and ncomp = m_i
//   kg_component_stats    per component {value, area, y1, x1, y2, x2, border, nb_min, nb_max}
//   kg_component_remap    out = newval[component] (the host's decision written back into a label map)
//
// The rules of label_common.h hold here, with the exception its index rule names (below): the number of launches depends neither on the
// image content nor on the number of components.
//
// Algorithm of kg_label_components: union-find whose root is the SMALLEST linear pixel index of a set.
//   1. cc_tile_kernel     one workgroup per 64 x 64 tile resolves the tile in LDS (labels + parents, 32 KB): one wave owns a 64-pixel row, the
//                         row runs come from a __shfl_up compare and the 64-bit __ballot (every pixel starts at its run head), the vertical
//                         (and, for 8-connectivity, diagonal) unions between consecutive rows use LDS atomicMin; the tile is then flattened
//                         and every pixel's parent is written to the global parent array as a linear index of the image.
//   2. cc_seam_kernel     unions across tile seams with global atomicMin: the top row of every tile but the first row of tiles against the
//                         row above it, the left column against the column to its left, the diagonals for 8-connectivity.
//   3. cc_flatten_kernel  every pixel looks its root up and lowers its own parent to it; the roots of every 4096-pixel block are counted.
//   4. cc_scan_kernel     exclusive scan of the block counts of every image (one workgroup per image); the total is ncomp.
//   5. cc_number_kernel   every root gets offset + rank within its block + 1, in raster order, straight into comp; pixels outside every
//                         component get 0.
//   6. cc_spread_kernel   every other pixel copies the number of its root (comp of a root is not written in this launch).
//
// INDEX RULE.  Union-find cannot avoid using values read from memory as indices; this is what bounds them:
//   - the parent array lives in the caller's workspace and cc_tile_kernel writes ALL of it before any kernel reads it;
//   - it only ever holds linear pixel indices of the same image, written by these kernels;
//   - a parent never exceeds its own index (a pixel starts at its run head or at the smaller root of its tile, and atomicMin only lowers
//     values), so every find loop descends strictly;
//   - every dereference of a value v read from memory sits inside the predicate (unsigned)v < (unsigned)(H * W) (4096 in LDS): cc_find_*
//     steps from cur to p only when (unsigned)p < (unsigned)cur, and cur starts at the caller's own pixel;
//   - every find and union loop has a hard iteration bound (the number of pixels: a strictly descending chain cannot be longer);
//   - kg_component_stats and kg_component_remap form the index c - 1 only inside (unsigned)(c - 1) < (unsigned)m_i; a comp value that
//     fails it touches nothing (stats) / writes 0 (remap).
// Because the root of a set is its smallest index whatever order the atomics land in, and the numbering is the raster order of the
// roots, comp and ncomp do not depend on arrival order.  Label VALUES are only ever compared.
#include "label_common.h"

#define KG_CC_STATS_BLOCKS 512         // grid of the stats walk: 2048 waves, each carrying one component from segment to segment
#define KG_CC_BLOCK 4096                // pixels per block of the flatten / number / spread kernels (16 per thread)

__device__ __forceinline__ int cc_conn(int v, int conn, int bg) { return v ? conn : bg; }
// what a cell other workgroups update with atomics holds now (or held a moment ago)
__device__ __forceinline__ int cc_peek(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- union-find ------------------------------------------------------------------------------------------------------------------------
// root of i in a 64 x 64 LDS tile; i is the caller's own (or an already checked) index < 4096
__device__ __forceinline__ int cc_find_lds(int* par, int i) {
    int cur = i;
    for (int it = 0; it < 4096; ++it) {
        const int p = __hip_atomic_load(par + cur, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (!((unsigned)p < 4096u) || !((unsigned)p < (unsigned)cur)) break;       // a root (p == cur), or not a smaller index: stop
        cur = p;
    }
    return cur;
}
__device__ __forceinline__ void cc_union_lds(int* par, int a, int b) {
    for (int it = 0; it < 4096; ++it) {
        a = cc_find_lds(par, a); b = cc_find_lds(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(par + a, b);
        if (!((unsigned)old < (unsigned)a)) return;                                 // a was a root and now points at b
        a = old;                                                                    // somebody lowered a first: join that chain with b
    }
}
// the same over the global parents of one image (par = parent + image base, n = H * W)
__device__ __forceinline__ int cc_find(int* par, int i, int n) {
    int cur = i;
    for (int it = 0; it < n; ++it) {
        const int p = __hip_atomic_load(par + cur, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!((unsigned)p < (unsigned)n) || !((unsigned)p < (unsigned)cur)) break;
        cur = p;
    }
    return cur;
}
__device__ __forceinline__ void cc_union(int* par, int a, int b, int n) {
    for (int it = 0; it < n; ++it) {
        a = cc_find(par, a, n); b = cc_find(par, b, n);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(par + a, b);
        if (!((unsigned)old < (unsigned)a)) return;
        a = old;
    }
}

// ---- 1. tiles ----------------------------------------------------------------------------------------------------------------------------
// Wave w owns rows 16 w .. 16 w + 15 of the tile, lane = column.  A pixel outside the image (ragged last tiles) or of a value whose
// connectivity is 0 joins nothing: it is its own run head and is never united.  Between rows y - 1 and y two runs of one value overlap in
// a column range whose first column is the head of one of them, so one union per (run, run) contact is enough: a pixel unites with the
// pixel above when it or that pixel is a run head; the diagonals (8) matter only where the pixel above differs.
__global__ __launch_bounds__(256) void cc_tile_kernel(const int* __restrict__ labels, int nimg, int H, int W, int ntx, int nty, int conn, int bg,
                                                      int* __restrict__ parent) {
    __shared__ int lab[4096];
    __shared__ int par[4096];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long tpi = (long)ntx * nty, ntile = tpi * nimg, HW = (long)H * W;
    for (long t = blockIdx.x; t < ntile; t += gridDim.x) {
        const long img = t / tpi;
        const int tt = (int)(t - img * tpi), ty = tt / ntx, tx = tt - ty * ntx;
        const long base = img * HW;
        const int gx = tx * 64 + lane;
        for (int r = 0; r < 16; ++r) {
            const int ly = wave * 16 + r, gy = ty * 64 + ly;
            const bool live = gx < W && gy < H;
            const int v = live ? labels[base + (long)gy * W + gx] : 0;
            const int c = live ? cc_conn(v, conn, bg) : 0;
            const int left = __shfl_up(v, 1);
            const bool joined = lane > 0 && c != 0 && v == left;                    // (a live lane's left neighbour is live)
            const unsigned long long heads = __ballot(!joined);
            const unsigned long long upto = lane == 63 ? heads : heads & ((2ull << lane) - 1ull);
            lab[ly * 64 + lane] = v;
            par[ly * 64 + lane] = ly * 64 + (63 - __clzll(upto));                   // lane 0 is always a head: upto != 0
        }
        __syncthreads();
        for (int r = 0; r < 16; ++r) {
            const int ly = wave * 16 + r, gy = ty * 64 + ly, l = ly * 64 + lane;
            if (ly == 0 || !(gx < W && gy < H)) continue;
            const int v = lab[l], c = cc_conn(v, conn, bg);
            if (c == 0) continue;
            const int up = lab[l - 64];
            if (up == v) {
                if (lane == 0 || lab[l - 1] != v || lab[l - 65] != v) cc_union_lds(par, l, l - 64);
            } else if (c == 8) {
                if (lane > 0 && lab[l - 65] == v && lab[l - 1] != v) cc_union_lds(par, l, l - 65);
                if (lane < 63 && gx + 1 < W && lab[l - 63] == v) cc_union_lds(par, l, l - 63);
            }
        }
        __syncthreads();
        for (int r = 0; r < 16; ++r) {
            const int ly = wave * 16 + r, gy = ty * 64 + ly;
            if (!(gx < W && gy < H)) continue;
            const int root = cc_find_lds(par, ly * 64 + lane);
            parent[base + (long)gy * W + gx] = (ty * 64 + (root >> 6)) * W + tx * 64 + (root & 63);
        }
        __syncthreads();                                                            // lab / par are written again by the block's next tile
    }
}

// ---- 2. seams ----------------------------------------------------------------------------------------------------------------------------
// Items of one image: the (nty - 1) * W pixels on the top row of a tile that has a tile above, then the (ntx - 1) * H pixels on the left
// column of a tile that has a tile to its left.  A diagonal is tried only where the straight neighbour differs: where it is equal, the
// diagonal pixel is joined to the straight one by a tile union or by another seam item.
__global__ __launch_bounds__(256) void cc_seam_kernel(const int* __restrict__ labels, int nimg, int H, int W, int ntx, int nty, int conn, int bg,
                                                      int* __restrict__ parent) {
    const unsigned hs = (unsigned)(nty - 1) * (unsigned)W, vs = (unsigned)(ntx - 1) * (unsigned)H, per = hs + vs;   // <= H * W / 32
    const long total = (long)per * nimg, HW = (long)H * W;
    const int n = (int)HW;
    for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < total; k += (long)gridDim.x * 256) {
        const long img = k / per;
        unsigned j = (unsigned)(k - img * per);
        const int* lb = labels + img * HW;
        int* par = parent + img * HW;
        if (j < hs) {
            const int s = (int)(j / (unsigned)W), x = (int)(j - (unsigned)s * (unsigned)W), y = (s + 1) * 64, p = y * W + x;
            const int v = lb[p], c = cc_conn(v, conn, bg);
            if (c == 0) continue;
            if (lb[p - W] == v) cc_union(par, p, p - W, n);
            else if (c == 8) {
                if (x > 0 && lb[p - W - 1] == v) cc_union(par, p, p - W - 1, n);
                if (x + 1 < W && lb[p - W + 1] == v) cc_union(par, p, p - W + 1, n);
            }
        } else {
            j -= hs;
            const int s = (int)(j / (unsigned)H), y = (int)(j - (unsigned)s * (unsigned)H), x = (s + 1) * 64, p = y * W + x;
            const int v = lb[p], c = cc_conn(v, conn, bg);
            if (c == 0) continue;
            if (lb[p - 1] == v) cc_union(par, p, p - 1, n);
            else if (c == 8) {
                if (y > 0 && lb[p - W - 1] == v) cc_union(par, p, p - W - 1, n);
                if (y + 1 < H && lb[p + W - 1] == v) cc_union(par, p, p + W - 1, n);
            }
        }
    }
}

// ---- 3. flatten, count the roots of every block ---------------------------------------------------------------------------------------------
// Block b of image i covers pixels [4096 b, 4096 (b + 1)) of that image, thread t takes t, t + 256, ... (consecutive lanes, consecutive
// pixels).  A root is a pixel inside a component whose parent is itself; lowering the parents of the others changes no root.
__global__ __launch_bounds__(256) void cc_flatten_kernel(const int* __restrict__ labels, int nimg, int H, int W, int nbi, int conn, int bg,
                                                         int* __restrict__ parent, int* __restrict__ blocksum) {
    __shared__ int part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long nblk = (long)nbi * nimg, HW = (long)H * W;
    const int n = (int)HW;
    for (long b = blockIdx.x; b < nblk; b += gridDim.x) {
        const long img = b / nbi;
        const int p0 = (int)(b - img * nbi) * KG_CC_BLOCK;
        const int* lb = labels + img * HW;
        int* par = parent + img * HW;
        int cnt = 0;
        for (int k = 0; k < 16; ++k) {
            const long pl = (long)p0 + k * 256 + (int)threadIdx.x;
            if (pl >= HW) break;
            const int p = (int)pl;
            if (cc_conn(lb[p], conn, bg) == 0) continue;
            const int root = cc_find(par, p, n);
            if (root == p) ++cnt;
            else atomicMin(par + p, root);
        }
        cnt = kg_wave_sum(cnt);
        if (lane == 0) part[wave] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) blocksum[b] = part[0] + part[1] + part[2] + part[3];
        __syncthreads();
    }
}

// ---- 4. exclusive scan of the block counts of every image, in place; ncomp = the total --------------------------------------------------------
__global__ __launch_bounds__(256) void cc_scan_kernel(int* __restrict__ blocksum, int nimg, int nbi, int* __restrict__ ncomp) {
    __shared__ int wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int img = blockIdx.x; img < nimg; img += gridDim.x) {
        int* bs = blocksum + (long)img * nbi;
        int carry = 0;
        for (int j0 = 0; j0 < nbi; j0 += 256) {
            const int j = j0 + (int)threadIdx.x;
            const int v = j < nbi ? bs[j] : 0;
            int s = v;
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(s, o);
                if (lane >= o) s += t;
            }
            if (lane == 63) wsum[wave] = s;
            __syncthreads();
            int woff = 0;
            for (int w = 0; w < wave; ++w) woff += wsum[w];
            const int tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
            if (j < nbi) bs[j] = carry + woff + s - v;
            carry += tot;
            __syncthreads();
        }
        if (threadIdx.x == 0) ncomp[img] = carry;
    }
}

// ---- 5. number the roots ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cc_number_kernel(const int* __restrict__ labels, int nimg, int H, int W, int nbi, int conn, int bg,
                                                        const int* __restrict__ parent, const int* __restrict__ blockoff, int* __restrict__ comp) {
    __shared__ int wcnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long nblk = (long)nbi * nimg, HW = (long)H * W;
    for (long b = blockIdx.x; b < nblk; b += gridDim.x) {
        const long img = b / nbi, base = img * HW;
        const int p0 = (int)(b - img * nbi) * KG_CC_BLOCK;
        int running = blockoff[b];
        for (int k = 0; k < 16; ++k) {                                              // (uniform trip count: the barriers below)
            const long p = (long)p0 + k * 256 + (int)threadIdx.x;
            const bool live = p < HW;
            const int c = live ? cc_conn(labels[base + p], conn, bg) : 0;
            const bool root = c != 0 && parent[base + p] == (int)p;
            const unsigned long long m = __ballot(root);
            if (lane == 0) wcnt[wave] = __popcll(m);
            __syncthreads();
            int before = __popcll(m & ((1ull << lane) - 1ull));
            for (int w = 0; w < wave; ++w) before += wcnt[w];
            const int tot = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
            if (live && c == 0) comp[base + p] = 0;
            else if (root) comp[base + p] = running + before + 1;
            running += tot;
            __syncthreads();
        }
    }
}

// ---- 6. every other pixel takes the number of its root -----------------------------------------------------------------------------------------
// comp of a root was written by cc_number_kernel and is only read here; comp of every other pixel of a component is written here, once.
__global__ __launch_bounds__(256) void cc_spread_kernel(const int* __restrict__ labels, int nimg, int H, int W, int nbi, int conn, int bg,
                                                        int* __restrict__ parent, int* comp) {
    const long nblk = (long)nbi * nimg, HW = (long)H * W;
    const int n = (int)HW;
    for (long b = blockIdx.x; b < nblk; b += gridDim.x) {
        const long img = b / nbi, base = img * HW;
        const int p0 = (int)(b - img * nbi) * KG_CC_BLOCK;
        int* par = parent + base;
        for (int k = 0; k < 16; ++k) {
            const long pl = (long)p0 + k * 256 + (int)threadIdx.x;
            if (pl >= HW) break;
            const int p = (int)pl;
            if (cc_conn(labels[base + p], conn, bg) == 0) continue;
            const int root = cc_find(par, p, n);
            if (root != p) comp[base + p] = comp[base + root];
        }
    }
}

// ---- stats -------------------------------------------------------------------------------------------------------------------------------
// neutral elements of (max, add, min, min, max, max, or, min, max)
__global__ __launch_bounds__(256) void cc_stats_init_kernel(int* __restrict__ stats, int total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < (long)total * 9) {
        const int c = (int)(i % 9);
        stats[i] = c == 0 ? INT_MIN : (c == 2 || c == 3 || c == 7) ? INT_MAX : c == 8 ? INT_MIN : 0;
    }
}

// The nine cells of one stats row, updated by whoever holds a partial result for it.  min / max / or only move a cell one way, so a value
// that cannot move the cell as it reads NOW cannot move it later either: that atomic is skipped.
__device__ __forceinline__ void cc_stats_commit(int* st, int v, int area, int y1, int x1, int y2, int x2, bool border, int lo, int hi) {
    if (v > cc_peek(st + 0)) atomicMax(st + 0, v);
    atomicAdd(st + 1, area);
    if (y1 < cc_peek(st + 2)) atomicMin(st + 2, y1);
    if (x1 < cc_peek(st + 3)) atomicMin(st + 3, x1);
    if (y2 > cc_peek(st + 4)) atomicMax(st + 4, y2);
    if (x2 > cc_peek(st + 5)) atomicMax(st + 5, x2);
    if (border && cc_peek(st + 6) == 0) atomicOr(st + 6, 1);
    if (lo < cc_peek(st + 7)) atomicMin(st + 7, lo);
    if (hi > cc_peek(st + 8)) atomicMax(st + 8, hi);
}

// The run walk of kg_seg_run over the comp values of the images of one launch: one wave per 64-pixel segment of a row, the grid
// striding over the segments.  Every lane looks at its four neighbours in the image; the smallest and largest neighbouring value that differs from the lane's own are
// reduced over the lanes of the run by shuffles, and the head issues the run's integer atomics (max, add, min, max, or): arrival order
// cannot change the result.  The row index c - 1 is formed only inside (unsigned)(c - 1) < (unsigned)m.
// One component can own most segments (the background: measured, its runs' adds to ONE address were 3/4 of the kernel), so every wave
// carries ONE component along in wave-uniform registers -- the first valid one of a segment, replaced when a segment does not hold it --
// folds the pixels of that component into them by ballots instead of atomics, and commits them when it lets go: the same integers by
// the same associative operations.
__global__ __launch_bounds__(256) void cc_stats_kernel(const int* __restrict__ labels, const int* __restrict__ comp, int cnt, int H, int W, KgRanges rg,
                                                       int* __restrict__ stats) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long spr = (W + 63) >> 6, spi = (long)H * spr, nseg = spi * cnt, HW = (long)H * W;
    int hrow = -1, hval = INT_MIN, harea = 0, hy1 = INT_MAX, hx1 = INT_MAX, hy2 = 0, hx2 = 0, hlo = INT_MAX, hhi = INT_MIN;     // wave-uniform
    bool hborder = false;
    for (long s = (long)blockIdx.x * 4 + wave; s < nseg; s += (long)gridDim.x * 4) {
        const int img = (int)(s / spi);
        const long si = s - (long)img * spi;
        const int row0 = rg.start[img], m = rg.start[img + 1] - row0;
        const KgSegRun r = kg_seg_run(si, spr, W, comp + (long)img * HW);
        const int y = r.y, x = r.x, x0 = x - lane, c = r.v, end = r.end;
        const bool head = r.head;
        const long idx = (long)img * HW + r.p;
        const bool valid = r.live && (unsigned)c - 1u < (unsigned)m;
        const int row = valid ? row0 + (int)((unsigned)c - 1u) : -1;               // < total: the only index made from c
        int lo = INT_MAX, hi = INT_MIN;
        if (valid) {
            int nb[4];
            nb[0] = y > 0 ? comp[idx - W] : c;
            nb[1] = y + 1 < H ? comp[idx + W] : c;
            nb[2] = x > 0 ? comp[idx - 1] : c;
            nb[3] = x + 1 < W ? comp[idx + 1] : c;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (nb[q] != c) { lo = nb[q] < lo ? nb[q] : lo; hi = nb[q] > hi ? nb[q] : hi; }
        }
        // the component the wave carries along
        const unsigned long long anyvalid = __ballot(valid);
        unsigned long long mine = hrow >= 0 ? __ballot(valid && row == hrow) : 0ull;
        if (mine == 0ull && anyvalid != 0ull) {
            if (hrow >= 0 && lane == 0) cc_stats_commit(stats + (long)hrow * 9, hval, harea, hy1, hx1, hy2, hx2, hborder, hlo, hhi);
            hrow = __shfl(row, __builtin_ctzll(anyvalid));
            hval = INT_MIN; harea = 0; hy1 = INT_MAX; hx1 = INT_MAX; hy2 = 0; hx2 = 0; hlo = INT_MAX; hhi = INT_MIN; hborder = false;
            mine = __ballot(valid && row == hrow);
        }
        const bool carried = valid && row == hrow;
        if (mine != 0ull) {
            const int first = __builtin_ctzll(mine), xa = x0 + first, xb = x0 + 64 - __builtin_clzll(mine);
            const int v = __shfl(lane == first ? labels[idx] : 0, first);
            int l2 = carried ? lo : INT_MAX, h2 = carried ? hi : INT_MIN;
            for (int o = 32; o; o >>= 1) {
                const int a = __shfl_xor(l2, o), b = __shfl_xor(h2, o);
                l2 = a < l2 ? a : l2; h2 = b > h2 ? b : h2;
            }
            hval = v > hval ? v : hval; harea += __popcll(mine);
            hy1 = y < hy1 ? y : hy1; hx1 = xa < hx1 ? xa : hx1; hy2 = y + 1 > hy2 ? y + 1 : hy2; hx2 = xb > hx2 ? xb : hx2;
            hborder = hborder || y == 0 || y == H - 1 || xa == 0 || xb == W;
            hlo = l2 < hlo ? l2 : hlo; hhi = h2 > hhi ? h2 : hhi;
        }
        // every other run: its head commits it
        for (int o = 1; o < 64; o <<= 1) {
            const int lo2 = __shfl_down(lo, o), hi2 = __shfl_down(hi, o);
            if (lane + o < end) { lo = lo2 < lo ? lo2 : lo; hi = hi2 > hi ? hi2 : hi; }
        }
        if (head && valid && !carried) {
            const int len = end - lane;
            cc_stats_commit(stats + (long)row * 9, labels[idx], len, y, x, y + 1, x + len, y == 0 || y == H - 1 || x == 0 || x + len == W, lo, hi);
        }
    }
    if (hrow >= 0 && lane == 0) cc_stats_commit(stats + (long)hrow * 9, hval, harea, hy1, hx1, hy2, hx2, hborder, hlo, hhi);
}

// a row no pixel named: zeros; no differing neighbour: nb_min = nb_max = -1
__global__ __launch_bounds__(256) void cc_stats_finish_kernel(int* __restrict__ stats, int total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < total) {
        int* st = stats + i * 9;
        if (st[1] == 0) { st[0] = 0; st[2] = 0; st[3] = 0; }
        if (st[7] == INT_MAX) { st[7] = -1; st[8] = -1; }
    }
}

// ---- remap -------------------------------------------------------------------------------------------------------------------------------
// blockIdx.y = image of the launch; out = newval[comp_start[i] + c - 1] inside (unsigned)(c - 1) < (unsigned)m_i, else 0
__global__ __launch_bounds__(256) void cc_remap_kernel(const int* __restrict__ comp, int H, int W, KgRanges rg, const int* __restrict__ newval,
                                                       int* __restrict__ out) {
    const int img = blockIdx.y;
    const int row0 = rg.start[img], m = rg.start[img + 1] - row0;
    const long HW = (long)H * W, base = (long)img * HW;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < HW; p += (long)gridDim.x * 256) {
        const int c = comp[base + p];
        out[base + p] = (unsigned)c - 1u < (unsigned)m ? newval[(long)row0 + (long)((unsigned)c - 1u)] : 0;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------
static inline long cc_nbi(int H, int W) { return ((long)H * W + KG_CC_BLOCK - 1) / KG_CC_BLOCK; }
static inline unsigned cc_grid(long blocks) { return kg_grid_cap(blocks < 1 ? 1 : blocks); }

static int cc_check_size(const char* fn, int nimg, int H, int W) {
    KG_CHECK_ARG(nimg > 0 && H > 0 && W > 0, "%s: bad size (nimg %d, H %d, W %d)", fn, nimg, H, W);
    return kg_check_stack_size(fn, nimg, H, W);
}

static int cc_check_start(const char* fn, const int* comp_start, int nimg, int total) {
    KG_CHECK_ARG(comp_start, "%s: null pointer (comp_start)", fn);
    KG_CHECK_ARG(total >= 0 && (long)total * 9 <= 0x7fffffffL, "%s: bad total %d", fn, total);
    return kg_check_start(fn, "comp_start", comp_start, nimg, total, "total");
}

// parents (one int per pixel) followed by the block counts (one int per 4096-pixel block of every image)
extern "C" long kg_label_components_workspace_bytes(int nimg, int H, int W) {
    if (nimg <= 0 || H <= 0 || W <= 0 || (long)H * W > 0x7fffffffL || (long)H * W * nimg > 0x7fffffffL) return -1;
    return 4L * ((long)H * W * nimg + cc_nbi(H, W) * nimg);
}

extern "C" int kg_label_components(const int* labels, int nimg, int H, int W, int connectivity, int bg_connectivity, int* comp, int* ncomp,
                                   void* workspace, long workspace_bytes, void* stream) {
    KG_TRY(cc_check_size("kg_label_components", nimg, H, W));
    KG_CHECK_ARG(connectivity == 4 || connectivity == 8, "kg_label_components: connectivity %d is not 4 or 8", connectivity);
    KG_CHECK_ARG(bg_connectivity == 0 || bg_connectivity == 4 || bg_connectivity == 8, "kg_label_components: bg_connectivity %d is not 0, 4 or 8",
                 bg_connectivity);
    KG_CHECK_ARG(labels && comp && ncomp && workspace, "kg_label_components: null pointer (labels / comp / ncomp / workspace)");
    KG_CHECK_ARG(kg_aligned(labels, 3) && kg_aligned(comp, 3) && kg_aligned(ncomp, 3) && kg_aligned(workspace, 3), "kg_label_components: misaligned pointer");
    KG_CHECK_ARG(labels != comp, "kg_label_components: comp aliases labels");
    const long need = kg_label_components_workspace_bytes(nimg, H, W);
    KG_CHECK_ARG(workspace_bytes >= need, "kg_label_components: workspace of %ld bytes, %ld needed", workspace_bytes, need);
    const long HW = (long)H * W;
    const int ntx = (W + 63) / 64, nty = (H + 63) / 64, nbi = (int)cc_nbi(H, W);
    int* parent = (int*)workspace;
    int* blocksum = parent + HW * nimg;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cc_tile_kernel, dim3(cc_grid((long)ntx * nty * nimg)), dim3(256), 0, st, labels, nimg, H, W, ntx, nty, connectivity, bg_connectivity,
                       parent);
    KG_CHECK_LAUNCH("label_components_tile");
    const long seam = ((long)(nty - 1) * W + (long)(ntx - 1) * H) * nimg;
    hipLaunchKernelGGL(cc_seam_kernel, dim3(cc_grid((seam + 255) / 256)), dim3(256), 0, st, labels, nimg, H, W, ntx, nty, connectivity, bg_connectivity,
                       parent);
    KG_CHECK_LAUNCH("label_components_seam");
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(cc_grid((long)nbi * nimg)), dim3(256), 0, st, labels, nimg, H, W, nbi, connectivity, bg_connectivity, parent,
                       blocksum);
    KG_CHECK_LAUNCH("label_components_flatten");
    hipLaunchKernelGGL(cc_scan_kernel, dim3(cc_grid(nimg)), dim3(256), 0, st, blocksum, nimg, nbi, ncomp);
    KG_CHECK_LAUNCH("label_components_scan");
    hipLaunchKernelGGL(cc_number_kernel, dim3(cc_grid((long)nbi * nimg)), dim3(256), 0, st, labels, nimg, H, W, nbi, connectivity, bg_connectivity,
                       (const int*)parent, (const int*)blocksum, comp);
    KG_CHECK_LAUNCH("label_components_number");
    hipLaunchKernelGGL(cc_spread_kernel, dim3(cc_grid((long)nbi * nimg)), dim3(256), 0, st, labels, nimg, H, W, nbi, connectivity, bg_connectivity, parent,
                       comp);
    KG_CHECK_LAUNCH("label_components_spread");
    return KG_OK;
}

extern "C" int kg_component_stats(const int* labels, const int* comp, int nimg, int H, int W, const int* comp_start, int total, int* stats,
                                  void* stream) {
    KG_TRY(cc_check_size("kg_component_stats", nimg, H, W));
    KG_TRY(cc_check_start("kg_component_stats", comp_start, nimg, total));
    KG_CHECK_ARG(labels && comp, "kg_component_stats: null pointer (labels / comp)");
    KG_CHECK_ARG(stats || total == 0, "kg_component_stats: null pointer (stats)");
    KG_CHECK_ARG(kg_aligned(labels, 3) && kg_aligned(comp, 3) && kg_aligned(stats, 3), "kg_component_stats: misaligned pointer");
    const long HW = (long)H * W, cells = (long)total * 9;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cc_stats_init_kernel, dim3((unsigned)(cells ? kg_cdiv(cells, 256) : 1)), dim3(256), 0, st, stats, total);
    KG_CHECK_LAUNCH("component_stats_init");
    for (int i0 = 0; i0 < nimg; i0 += KG_MAX_IMAGES) {
        const int cnt = nimg - i0 < KG_MAX_IMAGES ? nimg - i0 : KG_MAX_IMAGES;
        KgRanges rg;
        kg_ranges(comp_start, i0, cnt, &rg);
        const long nseg = (long)H * ((W + 63) / 64) * cnt, nb = (nseg + 3) / 4;
        hipLaunchKernelGGL(cc_stats_kernel, dim3((unsigned)(nb < KG_CC_STATS_BLOCKS ? nb : KG_CC_STATS_BLOCKS)), dim3(256), 0, st, labels + HW * i0, comp + HW * i0, cnt, H, W, rg, stats);
        KG_CHECK_LAUNCH("component_stats");
    }
    hipLaunchKernelGGL(cc_stats_finish_kernel, dim3((unsigned)(total ? kg_cdiv(total, 256) : 1)), dim3(256), 0, st, stats, total);
    KG_CHECK_LAUNCH("component_stats_finish");
    return KG_OK;
}

extern "C" int kg_component_remap(const int* comp, int nimg, int H, int W, const int* comp_start, int total, const int* newval, int* out,
                                  void* stream) {
    KG_TRY(cc_check_size("kg_component_remap", nimg, H, W));
    KG_TRY(cc_check_start("kg_component_remap", comp_start, nimg, total));
    KG_CHECK_ARG(comp && out, "kg_component_remap: null pointer (comp / out)");
    KG_CHECK_ARG(newval || total == 0, "kg_component_remap: null pointer (newval)");
    KG_CHECK_ARG(kg_aligned(comp, 3) && kg_aligned(newval, 3) && kg_aligned(out, 3), "kg_component_remap: misaligned pointer");
    KG_CHECK_ARG(out != comp && (out != newval || total == 0), "kg_component_remap: out aliases an input");
    const long HW = (long)H * W;
    for (int i0 = 0; i0 < nimg; i0 += KG_MAX_IMAGES) {
        const int cnt = nimg - i0 < KG_MAX_IMAGES ? nimg - i0 : KG_MAX_IMAGES;
        KgRanges rg;
        kg_ranges(comp_start, i0, cnt, &rg);
        const long nb = (HW + 255) / 256;
        hipLaunchKernelGGL(cc_remap_kernel, dim3((unsigned)(nb < 65536 ? nb : 65536), (unsigned)cnt), dim3(256), 0, (hipStream_t)stream, comp + HW * i0, H, W, rg,
                           newval, out + HW * i0);
        KG_CHECK_LAUNCH("component_remap");
    }
    return KG_OK;
}
