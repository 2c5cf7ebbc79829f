// Spatial statistics of a slide's detections (wsi.spatial_stats, wsi.quantify_region(spatial_radii=...)): the cross-class pair counts
// within B radii, the eligible centres of the border rule, and the nearest neighbour of every row in every class -- what Ripley's K
// and L, the pair correlation g and the nearest-neighbour distribution G are made of on the host.
//
// THE PAIR RULE is stated in include/amyloid_yolo.h; tests/spatial_reference.py restates it on the CPU by brute force over all pairs.
//
// HOW.  The third user of the centre grid (ay_box_grid.h), and the first that searches a fixed radius: a partner within R_max of a
// centre lies in the 3 x 3 cells around the centre's as soon as the cell side is at least R_max.  So the grid comes from the
// ARGUMENTS (the slide's sides, R_max, the number of rows) and not from the data: S = R_max * 2^m quarter pixels, m the smallest for
// which the grid over the slide has at most grid_cell_cap(n_rows) cells.  No reduction, no host read: the call is kernel launches only.
//   1. pair_fill_kernel zeroes / fills every output and the two cell arrays.
//   2. pair_count_kernel, one lane per row: centre, flags, quarter-pixel position, border distance, the largest eligible k, the cell
//      histogram (grid_count); the statistics and the eligible centres go through LDS to one global atomic per workgroup and word.
//   3. the scan of the cell histogram in three levels (chunks of 2 048 cells in parallel, grid_scan_kernel over the chunk totals, the
//      offsets added back), then pair_scatter_kernel (grid_slot) into a structure of arrays: qx, qy, class, largest k, original index.
//   4. pair_search_kernel, persistent workgroups of 256 threads, a GROUP of 16 lanes per centre (sorted position p, strided over the
//      groups of the launch, so that the heavy centres of one dense cell are dealt round).  The three adjacent cells of a grid row are
//      one contiguous run of the sorted arrays; the lanes of the group stride over the partners of the up to three runs.  A lane finds
//      its partner's first bin (five steps of a binary search over the squared radii in LDS) and adds to the group's table [C][B] in
//      LDS; the nearest neighbour per class is a 64-bit LDS minimum of (d2 << 32) | j, tried only when it beats the word just read.
//      The group then sums its table over k and adds the entries with k <= kmax_i to the workgroup's table [C][C][B] (64-bit, LDS);
//      the workgroup flushes its non-zero entries once, at its end, with 64-bit global atomics.  A group in which no lane found a
//      partner within R_max skips the sums.  The 16 lanes of a group sit in one wavefront, which issues its LDS operations in order:
//      the group needs no barrier, only the compiler has to be told (pair_wave_sync).
//      Why 16 lanes and not the wavefront: a centre is a chain of dependent load latencies (its own words, the run bounds, the
//      partners) with 28 .. 440 partners to visit on the slide of profiles/spatial.txt; with every wavefront slot of the chip taken,
//      one centre per wavefront left the search at 178 us there (256 px), four per wavefront at 114.5 us.
// Integer sums and minima with an index tie-break only: the order inside a cell (the scatter's cursor) shows in no output byte, and
// any cell side >= R_max gives the same result.
//
// LDS: 128 B of squared radii + 16 x (C x B x 4 + C x 8) B of group tables + C x C x B x 8 B for the workgroup, sized per launch
// (dynamic): 2 944 B at C = 2, B = 16 and 33 920 B at the limits C = 8, B = 32.  A CU holds 8 workgroups of 4 wavefronts by its
// wavefront slots; 160 KiB / 2 944 B is far beyond that, so the usual call is not limited by LDS, and at the limits 160 KiB /
// 33 920 B = 4 workgroups per CU, half the slots: the price of the group tables where C x B is at its largest (32-bit workgroup sums
// would save 8 KiB there and could overflow on a dense slide).
//
// THE PAIR WINDOW RULE (ay_pair_counts_window; stated next to THE PAIR RULE, restated by tests/spatial_window_reference.py): the border
// distance of minus-sampling measured to the edge of a MASK on cells of mask_cell pixels, not only to the four lines of the ROI.  Two
// kernels in front of the count kernel, which takes their result as one more bound (wbd) and is otherwise the plain call's:
//   a. pair_window_bits_kernel, one lane per (chunk of 64 mask rows, mask column), coalesced across the columns: the OUT cells of the
//      chunk as the bits of one word, bits [ceil(Gy / 64)][Gx].  Every word is written, so nothing is reset.
//   b. pair_window_dist_kernel, a group of 16 lanes per row: the lanes stride over the mask columns within R_max of the row (and
//      the virtual columns -1 and Gx, wholly OUT); in a column every position has the same horizontal distance, so the nearest OUT
//      position of the column is dx and the vertical distance to the nearest OUT cell above or below (or the slide's edge).  That
//      comes from the column's words: count-leading / count-trailing zeros in the word of the row's own cell row, and where that word
//      has no OUT cell on a side, a walk over the next words of the column as far as R_max reaches (R_max / (64 Sc) + 1 words, 9 at
//      the limits).  Both offsets are capped at R_max + 1 <= 32 768, so dx^2 + dy^2 <= 2^31: UNSIGNED 32-bit.  The minimum goes
//      across the group by four shuffles; wbd = the largest d in -1 .. R_max with d^2 < the minimum, an integer square root (a float
//      estimate, corrected on integers).  wbd [M] is written for every row (-1 for rows not counted).
//   The decomposition first built kept, per mask cell, the nearest OUT row above and below (8 bytes a cell, one more kernel): on a
//   16-px mask writing them was the largest part of what the window added.  Reading the words in the distance kernel instead makes
//   the call faster at small radii and leaves it level at large ones, with 1/64 of the workspace (profiles/spatial_window.txt).
//
// RELABEL: THE RELABEL RULE (ay_pair_counts_relabel; stated in include/amyloid_yolo_spatial_sim.h, restated by tests/
// spatial_envelope_reference.py): the counts of THE PAIR RULE (or THE PAIR WINDOW RULE) under S labellings of the counted rows, given as
// a table uint8 [M][stride] in row order.  Positions, bd, eligibility and the pairs within every radius are those of one labelling, so
// the front end is the plain call's up to the scatter (steps 1 .. 3, with a, b in front when there is a mask; the count kernel's
// centres go to the workspace), the sorted arrays sqx, sqy, skmax, sorig are used as they are, and two kernels stand in for step 4.
// Both read the table only through sorig.
//   5. relabel_centres_kernel: per simulation and label the histogram of the rows' largest k (LDS, a lane per simulation), its suffix
//      sum = the eligible centres, and the rows with bd >= 0.
//   6. relabel_search_kernel: ONE pair walk for all simulations.  A wavefront per centre, its 64 lanes 64 simulations; the geometry
//      of a partner is wave-uniform, its 64 labels one read of 64 bytes; a lane books the pair in its own LDS column [la][lb][k] as
//      +1 at the first bin and -1 behind the centre's last, and the prefix sum over k at the flush goes to sim_pairs (64-bit atomics).
//      LDS: a column has A x C x B int32 entries, at most 256 = 64 KiB for one wavefront; relabel_plan says which shapes keep all C
//      centre labels in the column (C x C x B <= 256: C = 2 at every B, C = 3 up to B = 28, C = 4 up to B = 16, C = 8 up to B = 4)
//      and which walk the pairs in passes over the centre's label.  At C = 2, B = 16 a wavefront takes 16 KiB, a workgroup of four 64
//      KiB: two workgroups, eight wavefronts per CU of 160 KiB.  Cost: profiles/spatial_envelope.txt.
#include <limits.h>

#include "ay_box_grid.h"
#include "../../include/amyloid_yolo_spatial_sim.h"

namespace ay {

constexpr int PAIR_THREADS = 256;
constexpr int PAIR_GROUP = 16;                               // lanes that share a centre
constexpr int PAIR_GROUPS = PAIR_THREADS / PAIR_GROUP;       // centres a workgroup has in flight
constexpr int PAIR_SEARCH_BLOCKS = 2048;   // 256 CUs x 8 workgroups

struct PairRadii {
    int n;
    int r[AY_PAIR_MAX_RADII];   // quarter pixels, ascending; INT_MAX behind the last
};
struct PairGrid {
    int S, gx, gy;
    __host__ __device__ int n_cells() const { return gx * gy; }
};
struct PairWindow {
    int x1, y1, x2, y2, border;
};

// the grid of the arguments; false where it would not fit int32 cell indices
static inline bool pair_grid(int n_rows, int H, int W, int r_max, int cell_side, PairGrid* g) {
    const long long qw = 4ll * W, qh = 4ll * H;
    long long S = cell_side > 0 ? cell_side : r_max;
    for (;;) {
        const long long gx = (qw + S - 1) / S, gy = (qh + S - 1) / S;
        if (cell_side > 0 || (unsigned long long)(gx * gy) <= grid_cell_cap(n_rows)) {
            if (gx * gy > (1ll << 30)) return false;
            g->S = (int)S, g->gx = (int)gx, g->gy = (int)gy;
            return true;
        }
        S *= 2;   // (ends at S >= 4 max(H, W) = 2^23 at most: one cell)
    }
}

__global__ void __launch_bounds__(PAIR_THREADS) pair_fill_kernel(int32_t* __restrict__ cell_start, int32_t* __restrict__ cursor, int n_words,
                                                                  int64_t* __restrict__ pairs, int n_pairs, int32_t* __restrict__ centres,
                                                                  int n_centres, int32_t* __restrict__ stats, int n_stats,
                                                                  int32_t* __restrict__ nn, long long n_nn, int32_t* __restrict__ bd, int M) {
    const long long stride = (long long)gridDim.x * PAIR_THREADS, t0 = (long long)blockIdx.x * PAIR_THREADS + threadIdx.x;
    for (long long i = t0; i < n_nn; i += stride) nn[i] = -1;
    for (long long i = t0; i < M; i += stride) bd[i] = -1;
    for (long long i = t0; i < n_words; i += stride) cell_start[i] = 0, cursor[i] = 0;
    for (long long i = t0; i < n_pairs; i += stride) pairs[i] = 0;
    for (long long i = t0; i < n_centres; i += stride) centres[i] = 0;
    for (long long i = t0; i < n_stats; i += stride) stats[i] = 0;
}

__device__ __forceinline__ bool pair_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }   // false for NaN and +-inf

// quarter-pixel position of a finite centre coordinate: c * 4 is exact or overflows to +-inf, which the clamp takes; q_max = 4n - 1 is
// exact in fp32 (n <= 2^21)
__device__ __forceinline__ int pair_position(float c, int q_max) { return (int)floorf(fminf(fmaxf(c * 4.0f, 0.0f), (float)q_max)); }

// THE PAIR RULE's centre and tests of one row: 0 for a counted row (its class in *c), the flag bits of a flagged row, -1 for a row below
__device__ __forceinline__ int pair_row(const float* __restrict__ r, int C, float min_conf, float* cx, float* cy, int* c) {
    const float x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3], conf = r[4], label = r[6];
    *cx = (x1 + x2) * 0.5f, *cy = (y1 + y2) * 0.5f;
    int flags = 0;
    *c = -1;
    if (!(pair_finite(*cx) && pair_finite(*cy))) flags |= AY_BURDEN_FLAG_NONFINITE;
    if (label >= 0.0f && label < (float)C) {
        *c = (int)label;
        if ((float)*c != label) *c = -1;
    }
    if (*c < 0) flags |= AY_BURDEN_FLAG_CLASS;
    if (flags) return flags;
    return conf >= min_conf ? 0 : -1;
}

// one lane per row: THE PAIR RULE up to the position; row_q = (qx, qy), row_ck = class | (kmax + 1) << 8 for the scatter.  wbd: the
// mask's bound on the border distance per row (THE PAIR WINDOW RULE), NULL for the plain call
__global__ void __launch_bounds__(PAIR_THREADS) pair_count_kernel(const float* __restrict__ rows, int M, int C, int q_max_x, int q_max_y, float min_conf,
                                                                   PairRadii rad, PairWindow win, PairGrid g, const int32_t* __restrict__ wbd,
                                                                   int32_t* __restrict__ cell_of, int32_t* __restrict__ cell_start,
                                                                   int2* __restrict__ row_q, int32_t* __restrict__ row_ck, int32_t* __restrict__ bd,
                                                                   int32_t* __restrict__ centres, int32_t* __restrict__ stats) {
    __shared__ int sh[2 * AY_PAIR_MAX_CLASSES + 3];                  // counted per class, inside per class, below, flagged, flag bits
    __shared__ int cen[AY_PAIR_MAX_CLASSES * AY_PAIR_MAX_RADII];     // rows of class a whose largest eligible k is kmax
    const int B = rad.n;
    for (int k = threadIdx.x; k < 2 * C + 3; k += PAIR_THREADS) sh[k] = 0;
    for (int k = threadIdx.x; k < C * B; k += PAIR_THREADS) cen[k] = 0;
    __syncthreads();
    const long long i = (long long)blockIdx.x * PAIR_THREADS + threadIdx.x;
    if (i < M) {
        float cx, cy;
        int c;
        const int flags = pair_row(rows + (size_t)i * 7, C, min_conf, &cx, &cy, &c);
        if (flags > 0) {
            atomicAdd(&sh[2 * C + 1], 1);
            atomicOr(&sh[2 * C + 2], flags);
            cell_of[i] = -1;
        } else if (flags < 0) {
            atomicAdd(&sh[2 * C], 1);
            cell_of[i] = -1;
        } else {
            const int qx = pair_position(cx, q_max_x), qy = pair_position(cy, q_max_y);
            int d = min(min(qx - win.x1, win.x2 - qx), min(qy - win.y1, win.y2 - qy));
            if (wbd) d = min(d, wbd[i]);
            int kmax = -1;
            if (win.border) {   // the radii ascend: the eligible k are a prefix (INT_MAX behind the last radius)
#pragma unroll
                for (int k = 0; k < AY_PAIR_MAX_RADII; ++k) kmax += d >= rad.r[k];
            } else if (d >= 0) {
                kmax = B - 1;
            }
            bd[i] = d >= 0 ? d : -1;
            row_q[i] = make_int2(qx, qy);
            row_ck[i] = c | ((kmax + 1) << 8);
            atomicAdd(&sh[c], 1);
            if (d >= 0) atomicAdd(&sh[C + c], 1);
            if (kmax >= 0) atomicAdd(&cen[c * B + kmax], 1);
            grid_count((int)i, (qy / g.S) * g.gx + qx / g.S, cell_of, cell_start);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 2 * C + 3; k += PAIR_THREADS) {
        const int v = sh[k];
        if (v) {
            if (k == 2 * C + 2) atomicOr(&stats[k], v);
            else atomicAdd(&stats[k], v);
        }
    }
    for (int e = threadIdx.x; e < C * B; e += PAIR_THREADS) {   // eligible at k: every row whose largest k is k or more
        const int a = e / B, k = e - a * B;
        int v = 0;
        for (int kk = k; kk < B; ++kk) v += cen[a * B + kk];
        if (v) atomicAdd(&centres[e], v);
    }
}

// ---- THE PAIR WINDOW RULE: the two kernels in front of the count kernel (a, b at the top of this file)
constexpr int PAIR_WINDOW_CHUNK = 64;                                     // mask rows of one word of `bits`
constexpr int PAIR_WINDOW_GROUP = 16;                                     // lanes that share a row in pair_window_dist_kernel
constexpr int PAIR_WINDOW_ROWS = PAIR_THREADS / PAIR_WINDOW_GROUP;        // rows of a workgroup there

struct PairMask {
    int S, gx, gy;   // cell side in quarter pixels, cells across, cells down
    __host__ __device__ int n_chunks() const { return (gy + PAIR_WINDOW_CHUNK - 1) / PAIR_WINDOW_CHUNK; }
};

// the mask grid of the arguments; false where the call refuses them
static inline bool pair_mask_grid(int H, int W, int mask_cell, PairMask* m) {
    if (mask_cell < AY_PAIR_WINDOW_MIN_CELL || mask_cell > AY_PAIR_MAX_SIDE) return false;
    const long long gx = ((long long)W + mask_cell - 1) / mask_cell, gy = ((long long)H + mask_cell - 1) / mask_cell;
    if (gx * gy > AY_PAIR_WINDOW_MAX_CELLS) return false;
    m->S = 4 * mask_cell, m->gx = (int)gx, m->gy = (int)gy;
    return true;
}

// bits[c][g]: bit r is set iff mask cell (64 c + r, g) is OUT (zero); rows past Gy leave their bits clear
__global__ void __launch_bounds__(PAIR_THREADS) pair_window_bits_kernel(const uint8_t* __restrict__ mask, PairMask m, unsigned long long* __restrict__ bits) {
    const int t = blockIdx.x * PAIR_THREADS + threadIdx.x;
    if (t >= m.n_chunks() * m.gx) return;
    const int c = t / m.gx, g = t - c * m.gx, y0 = c * PAIR_WINDOW_CHUNK, n = min(PAIR_WINDOW_CHUNK, m.gy - y0);
    unsigned long long w = 0;
#pragma unroll 8
    for (int r = 0; r < n; ++r) w |= (unsigned long long)(mask[(y0 + r) * m.gx + g] == 0) << r;   // (the loads are independent of w)
    bits[t] = w;
}

// floor(sqrt(v)) for v < 2^31: a float estimate, corrected on integers (s <= 46 341, so the squares fit 32 bits unsigned)
__device__ __forceinline__ unsigned pair_isqrt(unsigned v) {
    unsigned s = (unsigned)sqrtf((float)v);
    while (s * s > v) --s;
    while ((s + 1) * (s + 1) <= v) ++s;
    return s;
}

// the vertical distance (capped at `cap`) from position qy of mask row cy0 to the nearest OUT position of column g: 0 in an OUT cell,
// else to the nearest OUT cell above and below from the column's words, or to the slide's edge.  A walk over the words ends where the
// next word's nearest row is beyond `cap`: what lies further, the slide's edge included, is capped anyway.
__device__ __forceinline__ int pair_window_dy(const unsigned long long* __restrict__ bits, const PairMask& m, int g, int cy0, int qy, int qh, int cap) {
    const int c0 = cy0 / PAIR_WINDOW_CHUNK, r = cy0 % PAIR_WINDOW_CHUNK, n_chunks = m.n_chunks();
    const unsigned long long w = bits[c0 * m.gx + g];
    if ((w >> r) & 1) return 0;
    unsigned long long a = w & (~0ull >> (63 - r)), b = w >> r;   // the OUT rows above and below cy0 in its word
    int ca = c0, cb = c0;
    while (!a && ca > 0 && qy - (ca * PAIR_WINDOW_CHUNK * m.S - 1) <= cap) a = bits[--ca * m.gx + g];
    while (!b && cb + 1 < n_chunks && (cb + 1) * PAIR_WINDOW_CHUNK * m.S - qy <= cap) b = bits[++cb * m.gx + g];
    const int up = a ? ca * PAIR_WINDOW_CHUNK + 63 - __clzll((long long)a) : -1;                                          // -1: the slide's upper edge
    const int down = b ? (cb == c0 ? cy0 : cb * PAIR_WINDOW_CHUNK) + __ffsll((long long)b) - 1 : m.gy;                     // Gy: its lower edge
    const int above = qy - ((up + 1) * m.S - 1), below = down >= m.gy ? qh - qy : down * m.S - qy;
    return min(min(above, below), cap);
}

// a group of PAIR_WINDOW_GROUP lanes per row: wbd[i] = the largest d in -1 .. r_max with d^2 < the squared distance from row i's
// position to the nearest OUT position (outside the slide, or in a zero cell of the mask); -1 for rows that are not counted.
// dx^2 + dy^2 is UNSIGNED 32-bit: both offsets are capped at r_max + 1 <= 32 768, the sum reaches 2^31.
__global__ void __launch_bounds__(PAIR_THREADS) pair_window_dist_kernel(const float* __restrict__ rows, int M, int C, int q_max_x, int q_max_y, float min_conf,
                                                                         int r_max, PairMask m, const unsigned long long* __restrict__ bits,
                                                                         int32_t* __restrict__ wbd) {
    const int lane = threadIdx.x & (PAIR_WINDOW_GROUP - 1);
    const long long i = (long long)blockIdx.x * PAIR_WINDOW_ROWS + threadIdx.x / PAIR_WINDOW_GROUP;
    const int cap = r_max + 1, qw = q_max_x + 1, qh = q_max_y + 1;
    unsigned best = (unsigned)cap * (unsigned)cap;   // no OUT position within r_max
    bool counted = false;
    if (i < M) {
        float cx, cy;
        int c;
        counted = pair_row(rows + (size_t)i * 7, C, min_conf, &cx, &cy, &c) == 0;
        if (counted) {
            const int qx = pair_position(cx, q_max_x), qy = pair_position(cy, q_max_y), cy0 = qy / m.S;
            // the columns within r_max of qx; -1 and Gx are the half-planes left and right of the slide
            const int g_lo = qx >= r_max ? (qx - r_max) / m.S : -1, g_hi = qx + r_max >= qw ? m.gx : (qx + r_max) / m.S;
            for (int g = g_lo + lane; g <= g_hi; g += PAIR_WINDOW_GROUP) {
                int dx, dy = 0;
                if (g < 0) {
                    dx = qx + 1;
                } else if (g >= m.gx) {
                    dx = qw - qx;
                } else {
                    const int x0 = g * m.S, x1 = min(x0 + m.S, qw) - 1;   // (the last cell of a row is cut by the slide)
                    dx = max(max(x0 - qx, qx - x1), 0);
                    dy = pair_window_dy(bits, m, g, cy0, qy, qh, cap);
                }
                dx = min(dx, cap);
                best = min(best, (unsigned)(dx * dx) + (unsigned)(dy * dy));
            }
        }
    }
#pragma unroll
    for (int o = PAIR_WINDOW_GROUP / 2; o > 0; o >>= 1) best = min(best, (unsigned)__shfl_xor((int)best, o, PAIR_WINDOW_GROUP));
    if (i < M && lane == 0) wbd[i] = counted && best ? (int)min(pair_isqrt(best - 1), (unsigned)r_max) : -1;
}

// ---- the scan of the cell histogram in three levels.  grid_scan_kernel is ONE workgroup: right for the grids of the seam merge and the
// slide match, whose searches get cheaper with smaller cells, but here the grid is as fine as the cell cap allows and the scan
// pays for every cell (profiles/spatial.txt).  So: every workgroup scans a chunk of PAIR_SCAN_CHUNK cells in place and leaves its
// total, grid_scan_kernel scans the totals, and a last pass adds a chunk's offset to its cells.
constexpr int PAIR_SCAN_PER_THREAD = 8;
constexpr int PAIR_SCAN_CHUNK = PAIR_THREADS * PAIR_SCAN_PER_THREAD;

__global__ void __launch_bounds__(PAIR_THREADS) pair_scan_chunks_kernel(int32_t* __restrict__ a, int n, int32_t* __restrict__ chunk_sum) {
    __shared__ int wave_sum[PAIR_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long base = (long long)blockIdx.x * PAIR_SCAN_CHUNK + tid * PAIR_SCAN_PER_THREAD;
    int v[PAIR_SCAN_PER_THREAD], run = 0;
#pragma unroll
    for (int u = 0; u < PAIR_SCAN_PER_THREAD; ++u) v[u] = base + u < n ? a[base + u] : 0;
#pragma unroll
    for (int u = 0; u < PAIR_SCAN_PER_THREAD; ++u) {   // exclusive inside the thread; run = the thread's total
        const int t = v[u];
        v[u] = run;
        run += t;
    }
    int inc = run;   // inclusive over the wavefront
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    int off = inc - run;
    for (int w = 0; w < wave; ++w) off += wave_sum[w];
#pragma unroll
    for (int u = 0; u < PAIR_SCAN_PER_THREAD; ++u)
        if (base + u < n) a[base + u] = v[u] + off;
    if (tid == PAIR_THREADS - 1) chunk_sum[blockIdx.x] = off + run;
}

// a[i] += the offset of i's chunk; a[n] = the total (chunk_sum is scanned: chunk_sum[n_chunks] holds it)
__global__ void __launch_bounds__(PAIR_THREADS) pair_scan_add_kernel(int32_t* __restrict__ a, int n, const int32_t* __restrict__ chunk_sum, int n_chunks) {
    const long long stride = (long long)gridDim.x * PAIR_THREADS;
    for (long long i = (long long)blockIdx.x * PAIR_THREADS + threadIdx.x; i < n; i += stride) a[i] += chunk_sum[i / PAIR_SCAN_CHUNK];
    if (blockIdx.x == 0 && threadIdx.x == 0) a[n] = chunk_sum[n_chunks];
}

__global__ void __launch_bounds__(PAIR_THREADS) pair_scatter_kernel(int M, const int32_t* __restrict__ cell_of, const int32_t* __restrict__ cell_start,
                                                                     int32_t* __restrict__ cursor, const int2* __restrict__ row_q,
                                                                     const int32_t* __restrict__ row_ck, int32_t* __restrict__ sqx,
                                                                     int32_t* __restrict__ sqy, uint8_t* __restrict__ scls,
                                                                     int8_t* __restrict__ skmax, int32_t* __restrict__ sorig) {
    const long long i = (long long)blockIdx.x * PAIR_THREADS + threadIdx.x;
    if (i >= M) return;
    const int c = cell_of[i];
    if (c < 0) return;
    const int p = grid_slot(c, cell_start, cursor);
    const int2 q = row_q[i];
    const int ck = row_ck[i];
    sqx[p] = q.x, sqy[p] = q.y, scls[p] = (uint8_t)(ck & 255), skmax[p] = (int8_t)((ck >> 8) - 1), sorig[p] = (int)i;
}

// the lanes of a wavefront (so those of a group) see each other's LDS writes from here on: one wavefront issues its LDS operations
// in order, only the compiler has to be told
__device__ __forceinline__ void pair_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

static inline size_t pair_search_lds(int C, int B) {
    return sizeof(unsigned long long) * ((size_t)C * C * B + (size_t)PAIR_GROUPS * C) + sizeof(int) * (AY_PAIR_MAX_RADII + (size_t)PAIR_GROUPS * C * B);
}

// (at most 96 SGPRs: the 33 words of the radii otherwise take the kernel to 106 and the SIMD from 8 wavefronts to 7)
__global__ void __launch_bounds__(PAIR_THREADS) __attribute__((amdgpu_num_sgpr(96))) pair_search_kernel(PairRadii rad, int r_max, int C, PairGrid g, const int32_t* __restrict__ cell_start,
                                                                    const int32_t* __restrict__ sqx, const int32_t* __restrict__ sqy,
                                                                    const uint8_t* __restrict__ scls, const int8_t* __restrict__ skmax,
                                                                    const int32_t* __restrict__ sorig, int64_t* __restrict__ pairs,
                                                                    int32_t* __restrict__ nn) {
    extern __shared__ unsigned long long pair_lds[];
    const int B = rad.n, CB = C * B, tid = threadIdx.x, lane = tid & (PAIR_GROUP - 1), grp = tid / PAIR_GROUP;
    const int shift = (tid & 63) - lane;                                 // the group's first lane in its wavefront
    unsigned long long* wg = pair_lds;                                   // [C][C][B]
    unsigned long long* wnn = wg + (size_t)C * CB + grp * C;             // [C] of this group
    int* r2 = (int*)(pair_lds + (size_t)C * CB + PAIR_GROUPS * C);       // [32] squared radii, INT_MAX behind the last
    unsigned* wtab = (unsigned*)(r2 + AY_PAIR_MAX_RADII) + grp * CB;      // [C][B] of this group
    for (int e = tid; e < C * CB; e += PAIR_THREADS) wg[e] = 0;
    if (lane < C) wnn[lane] = ~0ull;
    for (int e = lane; e < CB; e += PAIR_GROUP) wtab[e] = 0;
#pragma unroll
    for (int k = 0; k < AY_PAIR_MAX_RADII; ++k)   // (constant indices into the kernel arguments: no scratch copy of them)
        if (tid == k) r2[k] = rad.r[k] <= AY_PAIR_MAX_RADIUS_Q ? rad.r[k] * rad.r[k] : INT_MAX;
    __syncthreads();
    const int n_cells = g.n_cells(), n = cell_start[n_cells];   // the counted rows
    const int r2_max = r_max * r_max;
    for (int p = blockIdx.x * PAIR_GROUPS + grp; p < n; p += gridDim.x * PAIR_GROUPS) {
        const int qxi = sqx[p], qyi = sqy[p], a = scls[p], kmax = skmax[p], i = sorig[p];
        const int cx = qxi / g.S, cy = qyi / g.S;
        const int xa = max(cx - 1, 0), xb = min(cx + 1, g.gx - 1);
        // the bounds of the three runs first, then per partner its four words at once: the time of a centre is a chain of load
        // latencies (profiles/spatial.txt), so nothing is loaded behind a test that an earlier load feeds
        int lo[3], hi[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int y = cy - 1 + r;
            const bool in = y >= 0 && y < g.gy;
            lo[r] = in ? cell_start[y * g.gx + xa] : 0;
            hi[r] = in ? cell_start[y * g.gx + xb + 1] : 0;
        }
        bool found = false;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            for (int q = lo[r] + lane; q < hi[r]; q += PAIR_GROUP) {
                const int dx = sqx[q] - qxi, dy = sqy[q] - qyi, b = scls[q], j = sorig[q];
                if (q == p || abs(dx) > r_max || abs(dy) > r_max) continue;   // (then both squares fit int32)
                const int d2 = dx * dx + dy * dy;
                if (d2 > r2_max) continue;
                int k = 0;   // the number of radii with R_k^2 < d2: the partner's first bin
#pragma unroll
                for (int s = AY_PAIR_MAX_RADII / 2; s > 0; s >>= 1) k += r2[k + s - 1] < d2 ? s : 0;
                atomicAdd(&wtab[b * B + k], 1u);
                const unsigned long long key = ((unsigned long long)(unsigned)d2 << 32) | (unsigned)j;
                if (key < __atomic_load_n(&wnn[b], __ATOMIC_RELAXED)) atomicMin(&wnn[b], key);
                found = true;
            }
        }
        // (group-uniform) nobody within r_max: the tables are as they were, nn keeps its -1
        if (((__ballot(found) >> shift) & ((1ull << PAIR_GROUP) - 1)) == 0) continue;
        pair_wave_sync();
        for (int e = lane; e < CB; e += PAIR_GROUP) {   // cumulative over k; the centre counts where it is eligible
            const int b = e / B, k = e - b * B;
            unsigned sum = 0;
#pragma unroll 8
            for (int kk = 0; kk < B; ++kk) sum += kk <= k ? wtab[b * B + kk] : 0u;   // (independent reads: several in flight)
            if (k <= kmax && sum) atomicAdd(&wg[(size_t)(a * C + b) * B + k], (unsigned long long)sum);
        }
        if (lane < C) {
            const unsigned long long key = wnn[lane];
            if (key != ~0ull) {
                int32_t* o = nn + ((size_t)i * C + lane) * 2;
                o[0] = (int)(key >> 32), o[1] = (int)(unsigned)key;
            }
        }
        pair_wave_sync();
        for (int e = lane; e < CB; e += PAIR_GROUP) wtab[e] = 0;
        if (lane < C) wnn[lane] = ~0ull;
        pair_wave_sync();
    }
    __syncthreads();
    for (int e = tid; e < C * CB; e += PAIR_THREADS) {
        const unsigned long long v = wg[e];
        if (v) atomicAdd((unsigned long long*)pairs + e, v);
    }
}

// ---- THE RELABEL RULE (ay_pair_counts_relabel; the header of this file, RELABEL): the two kernels behind the scatter
constexpr int RELABEL_LANES = 64;            // the simulations of a chunk: the lanes of a wavefront
constexpr int RELABEL_COLUMN = 256;          // the int32 entries of one lane's column that 64 KiB of LDS hold for one wavefront
constexpr int RELABEL_LDS = RELABEL_COLUMN * RELABEL_LANES * 4;
constexpr int RELABEL_WAVES = PAIR_THREADS / 64;
constexpr int RELABEL_UNROLL = 4;            // partner label reads in flight per wavefront
constexpr int RELABEL_ROWS = 1024;           // sorted rows of one workgroup of relabel_centres_kernel
constexpr int RELABEL_FLUSH = 1 << 30;       // pairs a wavefront books between two flushes (see relabel_search_kernel)
constexpr int RELABEL_BLOCKS = 1024;         // the search's workgroups, all chunks and passes together: 256 CUs x 4

struct PairRelabel {
    const uint8_t* labels;
    int S, stride;
    int64_t* sim_pairs;
    int32_t *sim_centres, *sim_inside;
};

// which shapes take which path.  A lane's column holds [A][C][B] entries, A the centre classes of one pass: A = C (one pass, every
// pair walked once) where C * C * B <= 256, else the largest A with A * C * B <= 256 and ceil(C / A) passes over the pair walk, each
// booking the centres labelled a0 .. a0 + A - 1 (A = 1 at C = 8, B = 32: eight passes, a column of exactly 256 entries).  C * B <=
// 256 always, so every legal shape has a plan.  A workgroup has as many wavefronts (1 .. 4) as 64 KiB hold columns for.
struct RelabelPlan {
    int A, passes, cols, waves, chunks;   // cols = A * C * B entries of a lane's column
    size_t lds() const { return (size_t)waves * cols * RELABEL_LANES * 4; }
};
static inline RelabelPlan relabel_plan(int C, int B, int S) {
    RelabelPlan p;
    p.A = RELABEL_COLUMN / (C * B) < C ? RELABEL_COLUMN / (C * B) : C;
    p.passes = (C + p.A - 1) / p.A;
    p.cols = p.A * C * B;
    p.waves = RELABEL_COLUMN / p.cols < RELABEL_WAVES ? RELABEL_COLUMN / p.cols : RELABEL_WAVES;
    p.chunks = (S + RELABEL_LANES - 1) / RELABEL_LANES;
    return p;
}
// the simulations of one workgroup of relabel_centres_kernel: its table [C][B + 1][SL] must fit 64 KiB (not at C = 8, B = 32 with 64)
static inline int relabel_centres_sims(int C, int B) { return C * (B + 1) * RELABEL_LANES * 4 <= RELABEL_LDS ? RELABEL_LANES : RELABEL_LANES / 2; }

// per simulation s and class a: the counted rows labelled a that are eligible at k (a histogram over the rows' largest k in LDS, a
// suffix sum at the end) and those with bd >= 0.  A workgroup takes RELABEL_ROWS sorted rows and SL simulations; a lane is a
// simulation (with SL = 32 the two halves of a wavefront take two rows).  A row with kmax >= 0 has bd >= R_0 > 0 under the border
// rule and bd >= 0 without it, so `inside` is the histogram's total plus the rows with kmax < 0 and bd >= 0 (slot B).  A label >= C
// on a counted row books nothing and sets AY_PAIR_RELABEL_FLAG_LABEL.
__global__ void __launch_bounds__(PAIR_THREADS) relabel_centres_kernel(int C, int B, int SL, const int32_t* __restrict__ cell_start, int n_cells,
                                                                        const int8_t* __restrict__ skmax, const int32_t* __restrict__ sorig,
                                                                        const int32_t* __restrict__ bd, const uint8_t* __restrict__ labels, int S,
                                                                        int stride, int32_t* __restrict__ sim_centres, int32_t* __restrict__ sim_inside,
                                                                        int32_t* __restrict__ stats) {
    extern __shared__ int relabel_tab[];   // [C][B + 1][SL]
    __shared__ int bad;
    const int n = cell_start[n_cells], base = blockIdx.x * RELABEL_ROWS, end = min(base + RELABEL_ROWS, n);
    if (base >= n) return;
    const int tid = threadIdx.x, per_wave = RELABEL_LANES / SL, sl = tid & (SL - 1), s = blockIdx.y * SL + sl;
    for (int e = tid; e < C * (B + 1) * SL; e += PAIR_THREADS) relabel_tab[e] = 0;
    if (tid == 0) bad = 0;
    __syncthreads();
    if (s < S) {
        for (int p = base + (tid >> 6) * per_wave + (tid & 63) / SL; p < end; p += RELABEL_WAVES * per_wave) {
            const int kmax = skmax[p], i = sorig[p];
            const int la = labels[(size_t)i * stride + s];
            if (la >= C) atomicOr(&bad, 1);
            else if (kmax >= 0) atomicAdd(&relabel_tab[(la * (B + 1) + kmax) * SL + sl], 1);
            else if (bd[i] >= 0) atomicAdd(&relabel_tab[(la * (B + 1) + B) * SL + sl], 1);
        }
    }
    __syncthreads();
    for (int e = tid; e < SL * C; e += PAIR_THREADS) {   // (the simulation moves fastest: the reads of a wavefront take 64 banks)
        const int l = e & (SL - 1), a = e / SL, sim = blockIdx.y * SL + l;
        if (sim >= S) continue;
        int run = 0;
        for (int k = B - 1; k >= 0; --k) {   // eligible at k: every row whose largest k is k or more
            run += relabel_tab[(a * (B + 1) + k) * SL + l];
            if (run) atomicAdd(&sim_centres[((size_t)sim * C + a) * B + k], run);
        }
        run += relabel_tab[(a * (B + 1) + B) * SL + l];
        if (run) atomicAdd(&sim_inside[(size_t)sim * C + a], run);
    }
    if (tid == 0 && bad) atomicOr(&stats[2 * C + 2], AY_PAIR_RELABEL_FLAG_LABEL);
}

// a lane's column: prefix sums over k of every [slot][b], added to the simulation's pairs with 64-bit atomics, and zeroed
__device__ __forceinline__ void relabel_flush(int* __restrict__ acc, int lane, int A, int a0, int C, int B, bool live, int s, int64_t* __restrict__ sim_pairs) {
    for (int slot = 0; slot < A && a0 + slot < C; ++slot)
        for (int b = 0; b < C; ++b) {
            int run = 0;
            unsigned long long* out = (unsigned long long*)sim_pairs + (((size_t)s * C + (a0 + slot)) * C + b) * B;
            for (int k = 0; k < B; ++k) {
                const int e = ((slot * C + b) * B + k) * RELABEL_LANES + lane;
                run += acc[e];
                acc[e] = 0;
                if (live && run) atomicAdd(out + k, (unsigned long long)run);
            }
        }
}

// the pair walk of pair_search_kernel with a WAVEFRONT per centre and a simulation per lane (chunk blockIdx.y of 64 simulations, pass
// blockIdx.z over the centre's label: relabel_plan).  The partners of a run are taken 64 at a time, a lane each: d2 on integers and
// the first bin k as the number of squared radii below d2 (32 compares against kernel arguments: no table, the LDS is the columns').
// The partners with k <= kmax of the centre are then walked one by one, wave-uniform (ballot, readlane): a partner's 64 labels are
// one coalesced read of 64 bytes, RELABEL_UNROLL partners in flight.  Lane s adds +1 at [la - a0][lb][k] and -1 at [..][kmax + 1]
// (nothing behind the last bin) of ITS OWN column acc[entry][lane] in LDS: the prefix sum over k at the flush is the pair's share of
// the bins k .. kmax.  No lane reads another's words, so there is no barrier, and with the lane as the fastest index no bank
// conflict; the adds are LDS add instructions without a result, not read-modify-write chains.
// NO COUNTER WRAPS.  Every booked pair moves one entry of a column by +1 and at most one by -1, so after n pairs every entry and every
// prefix sum lies in -n .. n.  `booked` counts the partners a wavefront walked since its last flush (wave-uniform, an upper bound for
// every lane); it is tested after every 64 partners, so a wavefront flushes before it passes RELABEL_FLUSH + 64 + RELABEL_UNROLL < 2^31,
// and once more at its end.
__global__ void __launch_bounds__(PAIR_THREADS) relabel_search_kernel(PairRadii rad, int r_max, int C, int A, PairGrid g, const int32_t* __restrict__ cell_start,
                                                                       const int32_t* __restrict__ sqx, const int32_t* __restrict__ sqy,
                                                                       const int8_t* __restrict__ skmax, const int32_t* __restrict__ sorig,
                                                                       const uint8_t* __restrict__ labels, int S, int stride,
                                                                       int64_t* __restrict__ sim_pairs) {
    extern __shared__ int relabel_acc[];   // [waves][A][C][B][64]
    const int B = rad.n, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), waves = blockDim.x >> 6;
    const int cols = A * C * B, a0 = blockIdx.z * A, s = blockIdx.y * RELABEL_LANES + lane;
    const bool live = s < S;
    int* acc = relabel_acc + (size_t)wave * cols * RELABEL_LANES;
    for (int e = 0; e < cols; ++e) acc[e * RELABEL_LANES + lane] = 0;
    const int n = cell_start[g.n_cells()];   // the counted rows
    int booked = 0;
    for (int p = blockIdx.x * waves + wave; p < n; p += gridDim.x * waves) {
        const int kmax = skmax[p];
        if (kmax < 0) continue;   // (wave-uniform) eligible nowhere: no centre
        const int qxi = sqx[p], qyi = sqy[p], i = sorig[p];
        const int la = live ? labels[(size_t)i * stride + s] : 255;
        const int slot = la - a0;
        const bool mine = la < C && slot >= 0 && slot < A;   // (a label >= C: no centre in this simulation)
        if (__ballot(mine) == 0) continue;                   // no simulation of the chunk has this centre in the pass
        const int cx = qxi / g.S, cy = qyi / g.S;
        const int xa = max(cx - 1, 0), xb = min(cx + 1, g.gx - 1);
        int lo[3], hi[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int y = cy - 1 + r;
            const bool in = y >= 0 && y < g.gy;
            lo[r] = in ? cell_start[y * g.gx + xa] : 0;
            hi[r] = in ? cell_start[y * g.gx + xb + 1] : 0;
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            for (int q0 = lo[r]; q0 < hi[r]; q0 += RELABEL_LANES) {
                const int q = q0 + lane;
                int dx = 0, dy = 0, j = 0;
                bool hit = q < hi[r] && q != p;
                if (hit) dx = sqx[q] - qxi, dy = sqy[q] - qyi, j = sorig[q];
                hit = hit && abs(dx) <= r_max && abs(dy) <= r_max;   // (then both squares fit int32)
                const int d2 = hit ? dx * dx + dy * dy : 0;
                int k = 0;   // the number of radii with R_k^2 < d2: the partner's first bin (B beyond the largest radius)
#pragma unroll
                for (int t = 0; t < AY_PAIR_MAX_RADII; ++t) k += (rad.r[t] <= AY_PAIR_MAX_RADIUS_Q ? rad.r[t] * rad.r[t] : INT_MAX) < d2 ? 1 : 0;
                unsigned long long m = __ballot(hit && k <= kmax);
                while (m) {   // (wave-uniform)
                    int jj[RELABEL_UNROLL], kk[RELABEL_UNROLL], lb[RELABEL_UNROLL];
                    bool valid[RELABEL_UNROLL];
                    int l = 0;
#pragma unroll
                    for (int u = 0; u < RELABEL_UNROLL; ++u) {
                        valid[u] = m != 0;
                        if (m) l = __builtin_ctzll(m), m &= m - 1;
                        jj[u] = __builtin_amdgcn_readlane(j, l), kk[u] = __builtin_amdgcn_readlane(k, l);   // (past the last: the one before again)
                    }
#pragma unroll
                    for (int u = 0; u < RELABEL_UNROLL; ++u) lb[u] = live ? labels[(size_t)jj[u] * stride + s] : 255;
#pragma unroll
                    for (int u = 0; u < RELABEL_UNROLL; ++u) {
                        if (valid[u] && mine && lb[u] < C) {   // (a label >= C: no partner in this simulation)
                            int* col = acc + (size_t)((slot * C + lb[u]) * B) * RELABEL_LANES + lane;
                            __hip_atomic_fetch_add(col + kk[u] * RELABEL_LANES, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            if (kmax + 1 < B) __hip_atomic_fetch_add(col + (kmax + 1) * RELABEL_LANES, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
                    }
                    booked += RELABEL_UNROLL;
                }
                if (booked >= RELABEL_FLUSH) {   // (wave-uniform; between two partners, each booked whole)
                    relabel_flush(acc, lane, A, a0, C, B, live, s, sim_pairs);
                    booked = 0;
                }
            }
        }
    }
    relabel_flush(acc, lane, A, a0, C, B, live, s, sim_pairs);
}

struct PairWs {
    int32_t *cell_of, *row_ck, *sqx, *sqy, *sorig, *cell_start, *cursor, *chunk_sum, *wbd, *obs_centres;
    int2* row_q;
    unsigned long long* bits;
    uint8_t* scls;
    int8_t* skmax;
    size_t bytes;
};

// mask: the mask grid of the window call, NULL for the plain call (whose workspace is then what it was)
static PairWs pair_carve(void* ws, int n_rows, size_t n_cells, const PairMask* mask, bool relabel = false) {
    PairWs w;
    WsCarver cv(ws);
    const size_t m = (size_t)(n_rows > 0 ? n_rows : 1);
    w.cell_of = cv.take<int32_t>(m);
    w.row_q = cv.take<int2>(m);
    w.row_ck = cv.take<int32_t>(m);
    w.sqx = cv.take<int32_t>(m);
    w.sqy = cv.take<int32_t>(m);
    w.sorig = cv.take<int32_t>(m);
    w.scls = cv.take<uint8_t>(m);
    w.skmax = cv.take<int8_t>(m);
    w.cell_start = cv.take<int32_t>(n_cells + 2);
    w.cursor = cv.take<int32_t>(n_cells + 2);
    w.chunk_sum = cv.take<int32_t>((n_cells + PAIR_SCAN_CHUNK - 1) / PAIR_SCAN_CHUNK + 2);
    w.wbd = nullptr, w.bits = nullptr;
    if (mask) {
        w.wbd = cv.take<int32_t>(m);
        w.bits = cv.take<unsigned long long>((size_t)mask->gx * mask->n_chunks());
    }
    w.obs_centres = relabel ? cv.take<int32_t>(AY_PAIR_MAX_CLASSES * AY_PAIR_MAX_RADII) : nullptr;   // the count kernel's centres [C][B]
    w.bytes = cv.bytes();
    return w;
}

static inline bool pair_dims_ok(int n_rows, int H, int W, int r_max, int cell_side) {
    return n_rows >= 0 && H >= 1 && W >= 1 && H <= AY_PAIR_MAX_SIDE && W <= AY_PAIR_MAX_SIDE && r_max >= 1 && r_max <= AY_PAIR_MAX_RADIUS_Q &&
           (cell_side <= 0 || cell_side >= r_max);
}

static inline unsigned pair_blocks(long long n, long long cap) {
    const long long b = (n + PAIR_THREADS - 1) / PAIR_THREADS;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

static size_t pair_workspace_bytes(int n_rows, int H, int W, int r_max, int cell_side, bool windowed, int mask_cell, bool relabel = false) {
    PairGrid g;
    PairMask mg;
    if (!pair_dims_ok(n_rows, H, W, r_max, cell_side) || !pair_grid(n_rows, H, W, r_max, cell_side, &g)) return 0;
    if (windowed && !pair_mask_grid(H, W, mask_cell, &mg)) return 0;
    return pair_carve(nullptr, n_rows, (size_t)g.n_cells(), windowed ? &mg : nullptr, relabel).bytes;
}

// the three entry points: `who` names the one in the messages; windowed adds the two kernels of THE PAIR WINDOW RULE and hands their
// wbd to the count kernel.  With `rl` (ay_pair_counts_relabel) pairs, centres and nn are NULL: the front end is the same up to the
// scatter (the count kernel's centres go to the workspace), and the two relabel kernels stand in for pair_search_kernel.
static int pair_counts_run(const char* who, bool windowed, const float* rows, int n_rows, int num_classes, int slide_h, int slide_w, float min_conf,
                           const int32_t* radii_q, int n_radii, const int32_t* roi_q, int border, int cell_side_q, const uint8_t* mask, int mask_cell,
                           int64_t* pairs, int32_t* centres, int32_t* nn, int32_t* bd, int32_t* stats, void* workspace, size_t workspace_bytes,
                           ay_stream_t stream, const PairRelabel* rl = nullptr) {
    const int M = n_rows, C = num_classes, B = n_radii, H = slide_h, W = slide_w;
    AY_CHECK_ARG(M >= 0 && (M == 0 || rows), "%s: n_rows %d%s", who, M, rows ? "" : " with null rows");
    AY_CHECK_ARG(C >= 1 && C <= AY_PAIR_MAX_CLASSES, "%s: num_classes %d outside 1 .. %d", who, C, AY_PAIR_MAX_CLASSES);
    AY_CHECK_ARG(H >= 1 && W >= 1 && H <= AY_PAIR_MAX_SIDE && W <= AY_PAIR_MAX_SIDE, "%s: slide %d x %d outside 1 .. %d", who, H, W, AY_PAIR_MAX_SIDE);
    AY_CHECK_ARG(radii_q && B >= 1 && B <= AY_PAIR_MAX_RADII, "%s: n_radii %d outside 1 .. %d", who, B, AY_PAIR_MAX_RADII);
    PairRadii rad;
    rad.n = B;
    for (int k = 0; k < AY_PAIR_MAX_RADII; ++k) rad.r[k] = k < B ? radii_q[k] : INT_MAX;
    for (int k = 0; k < B; ++k)
        AY_CHECK_ARG(rad.r[k] >= 1 && rad.r[k] <= AY_PAIR_MAX_RADIUS_Q && (k == 0 || rad.r[k] > rad.r[k - 1]),
                     "%s: radii[%d] = %d: the radii ascend strictly inside 1 .. %d quarter pixels", who, k, rad.r[k], AY_PAIR_MAX_RADIUS_Q);
    const int r_max = rad.r[B - 1];
    PairWindow win = {0, 0, 4 * W - 1, 4 * H - 1, border ? 1 : 0};
    if (roi_q) win.x1 = roi_q[0], win.y1 = roi_q[1], win.x2 = roi_q[2], win.y2 = roi_q[3];
    AY_CHECK_ARG(win.x1 <= win.x2 && win.y1 <= win.y2, "%s: roi (%d, %d, %d, %d) is empty", who, win.x1, win.y1, win.x2, win.y2);
    // (the border distance subtracts a position in 0 .. 2^23 from a bound: keep the bounds where that cannot overflow)
    AY_CHECK_ARG(win.x1 >= -(1 << 30) && win.y1 >= -(1 << 30) && win.x2 <= (1 << 30) && win.y2 <= (1 << 30), "%s: roi beyond +-2^30", who);
    AY_CHECK_ARG(cell_side_q <= 0 || cell_side_q >= r_max, "%s: cell_side %d below the largest radius %d", who, cell_side_q, r_max);
    PairGrid g;
    AY_CHECK_ARG(pair_grid(M, H, W, r_max, cell_side_q, &g), "%s: cell_side %d gives more than 2^30 cells", who, cell_side_q);
    PairMask mg = {0, 0, 0};
    if (windowed) {
        AY_CHECK_ARG(mask, "%s: null mask", who);
        AY_CHECK_ARG(mask_cell >= AY_PAIR_WINDOW_MIN_CELL && mask_cell <= AY_PAIR_MAX_SIDE, "%s: mask_cell %d outside %d .. %d", who, mask_cell,
                     AY_PAIR_WINDOW_MIN_CELL, AY_PAIR_MAX_SIDE);
        AY_CHECK_ARG(pair_mask_grid(H, W, mask_cell, &mg), "%s: mask_cell %d gives more than 2^26 mask cells on a %d x %d slide", who, mask_cell, H, W);
    }
    if (rl) {
        AY_CHECK_ARG(rl->S >= 1 && rl->S <= AY_PAIR_RELABEL_MAX_SIMS, "%s: n_sims %d outside 1 .. %d", who, rl->S, AY_PAIR_RELABEL_MAX_SIMS);
        AY_CHECK_ARG(rl->stride >= rl->S, "%s: label_stride %d below n_sims %d", who, rl->stride, rl->S);
        AY_CHECK_ARG(M == 0 || rl->labels, "%s: null labels", who);
        AY_CHECK_ARG(rl->sim_pairs && rl->sim_centres && rl->sim_inside && stats && workspace && (M == 0 || bd), "%s: null output or workspace", who);
    } else {
        AY_CHECK_ARG(pairs && centres && stats && workspace && (M == 0 || (nn && bd)), "%s: null output or workspace", who);
    }
    const int n_cells = g.n_cells();
    const PairWs w = pair_carve(workspace, M, (size_t)n_cells, windowed ? &mg : nullptr, rl != nullptr);
    AY_CHECK_ARG(workspace_bytes >= w.bytes, "%s: workspace %zu < %zu bytes", who, workspace_bytes, w.bytes);
    AY_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "%s: workspace not 16-byte aligned", who);
    hipStream_t st = S(stream);
    long long n_nn = (long long)M * C * 2;
    int n_pairs = C * C * B;
    if (rl) {   // the simulations' pairs are zeroed where the plain call zeroes its own; the other two outputs by a second launch
        pairs = rl->sim_pairs, n_pairs *= rl->S, centres = w.obs_centres, nn = nullptr, n_nn = 0;
        hipLaunchKernelGGL(pair_fill_kernel, dim3(pair_blocks((long long)rl->S * C * B, 4096)), dim3(PAIR_THREADS), 0, st, (int32_t*)nullptr,
                           (int32_t*)nullptr, 0, (int64_t*)nullptr, 0, rl->sim_centres, rl->S * C * B, rl->sim_inside, rl->S * C, (int32_t*)nullptr, 0ll,
                           (int32_t*)nullptr, 0);
        AY_CHECK_LAUNCH("pair_fill_kernel");
    }
    const long long cells_or_rows = (long long)M > n_cells + 2 ? (long long)M : n_cells + 2;
    const long long most = rl ? (n_pairs > cells_or_rows ? n_pairs : cells_or_rows) : (n_nn > n_cells + 2 ? n_nn : n_cells + 2);
    hipLaunchKernelGGL(pair_fill_kernel, dim3(pair_blocks(most, 4096)), dim3(PAIR_THREADS), 0, st, w.cell_start, w.cursor, n_cells + 2, pairs, n_pairs,
                       centres, C * B, stats, 2 * C + 3, nn, n_nn, bd, M);
    AY_CHECK_LAUNCH("pair_fill_kernel");
    if (M > 0) {
        const unsigned rblocks = (unsigned)(((long long)M + PAIR_THREADS - 1) / PAIR_THREADS);
        if (windowed) {
            const unsigned cblocks = pair_blocks((long long)mg.n_chunks() * mg.gx, INT_MAX);
            hipLaunchKernelGGL(pair_window_bits_kernel, dim3(cblocks), dim3(PAIR_THREADS), 0, st, mask, mg, w.bits);
            AY_CHECK_LAUNCH("pair_window_bits_kernel");
            hipLaunchKernelGGL(pair_window_dist_kernel, dim3((unsigned)(((long long)M + PAIR_WINDOW_ROWS - 1) / PAIR_WINDOW_ROWS)), dim3(PAIR_THREADS), 0, st,
                               rows, M, C, 4 * W - 1, 4 * H - 1, min_conf, r_max, mg, (const unsigned long long*)w.bits, w.wbd);
            AY_CHECK_LAUNCH("pair_window_dist_kernel");
        }
        hipLaunchKernelGGL(pair_count_kernel, dim3(rblocks), dim3(PAIR_THREADS), 0, st, rows, M, C, 4 * W - 1, 4 * H - 1, min_conf, rad, win, g,
                           (const int32_t*)w.wbd, w.cell_of, w.cell_start, w.row_q, w.row_ck, bd, centres, stats);
        AY_CHECK_LAUNCH("pair_count_kernel");
        const int n_chunks = (n_cells + PAIR_SCAN_CHUNK - 1) / PAIR_SCAN_CHUNK;
        hipLaunchKernelGGL(pair_scan_chunks_kernel, dim3(n_chunks), dim3(PAIR_THREADS), 0, st, w.cell_start, n_cells, w.chunk_sum);
        AY_CHECK_LAUNCH("pair_scan_chunks_kernel");
        hipLaunchKernelGGL(grid_scan_kernel, dim3(1), dim3(1024), 0, st, w.chunk_sum, n_chunks);
        AY_CHECK_LAUNCH("grid_scan_kernel");
        hipLaunchKernelGGL(pair_scan_add_kernel, dim3(pair_blocks(n_cells, 4096)), dim3(PAIR_THREADS), 0, st, w.cell_start, n_cells,
                           (const int32_t*)w.chunk_sum, n_chunks);
        AY_CHECK_LAUNCH("pair_scan_add_kernel");
        hipLaunchKernelGGL(pair_scatter_kernel, dim3(rblocks), dim3(PAIR_THREADS), 0, st, M, (const int32_t*)w.cell_of, (const int32_t*)w.cell_start,
                           w.cursor, (const int2*)w.row_q, (const int32_t*)w.row_ck, w.sqx, w.sqy, w.scls, w.skmax, w.sorig);
        AY_CHECK_LAUNCH("pair_scatter_kernel");
        if (rl) {
            const int SL = relabel_centres_sims(C, B);
            hipLaunchKernelGGL(relabel_centres_kernel, dim3((unsigned)(((long long)M + RELABEL_ROWS - 1) / RELABEL_ROWS), (unsigned)((rl->S + SL - 1) / SL)),
                               dim3(PAIR_THREADS), (size_t)C * (B + 1) * SL * 4, st, C, B, SL, (const int32_t*)w.cell_start, n_cells, (const int8_t*)w.skmax,
                               (const int32_t*)w.sorig, (const int32_t*)bd, rl->labels, rl->S, rl->stride, rl->sim_centres, rl->sim_inside, stats);
            AY_CHECK_LAUNCH("relabel_centres_kernel");
            const RelabelPlan pl = relabel_plan(C, B, rl->S);
            const long long want = ((long long)M + pl.waves - 1) / pl.waves, cap = RELABEL_BLOCKS / (pl.chunks * pl.passes);
            const unsigned bx = (unsigned)(want < 1 ? 1 : (want > cap ? (cap < 1 ? 1 : cap) : want));
            hipLaunchKernelGGL(relabel_search_kernel, dim3(bx, (unsigned)pl.chunks, (unsigned)pl.passes), dim3(64 * pl.waves), pl.lds(), st, rad, r_max, C,
                               pl.A, g, (const int32_t*)w.cell_start, (const int32_t*)w.sqx, (const int32_t*)w.sqy, (const int8_t*)w.skmax,
                               (const int32_t*)w.sorig, rl->labels, rl->S, rl->stride, rl->sim_pairs);
            AY_CHECK_LAUNCH("relabel_search_kernel");
            return AY_OK;
        }
        hipLaunchKernelGGL(pair_search_kernel, dim3(pair_blocks((long long)M * PAIR_GROUP, PAIR_SEARCH_BLOCKS)), dim3(PAIR_THREADS), pair_search_lds(C, B), st, rad,
                           r_max, C, g, (const int32_t*)w.cell_start, (const int32_t*)w.sqx, (const int32_t*)w.sqy, (const uint8_t*)w.scls,
                           (const int8_t*)w.skmax, (const int32_t*)w.sorig, pairs, nn);
        AY_CHECK_LAUNCH("pair_search_kernel");
    }
    return AY_OK;
}

}  // namespace ay

extern "C" size_t ay_pair_counts_workspace_bytes(int n_rows, int slide_h, int slide_w, int r_max_q, int cell_side_q) {
    return ay::pair_workspace_bytes(n_rows, slide_h, slide_w, r_max_q, cell_side_q, false, 0);
}

extern "C" int ay_pair_counts(const float* rows, int n_rows, int num_classes, int slide_h, int slide_w, float min_conf, const int32_t* radii_q,
                              int n_radii, const int32_t* roi_q, int border, int cell_side_q, int64_t* pairs, int32_t* centres, int32_t* nn,
                              int32_t* bd, int32_t* stats, void* workspace, size_t workspace_bytes, ay_stream_t stream) {
    return ay::pair_counts_run("ay_pair_counts", false, rows, n_rows, num_classes, slide_h, slide_w, min_conf, radii_q, n_radii, roi_q, border,
                               cell_side_q, nullptr, 0, pairs, centres, nn, bd, stats, workspace, workspace_bytes, stream);
}

extern "C" size_t ay_pair_counts_window_workspace_bytes(int n_rows, int slide_h, int slide_w, int r_max_q, int cell_side_q, int mask_cell) {
    return ay::pair_workspace_bytes(n_rows, slide_h, slide_w, r_max_q, cell_side_q, true, mask_cell);
}

extern "C" int ay_pair_counts_window(const float* rows, int n_rows, int num_classes, int slide_h, int slide_w, float min_conf, const int32_t* radii_q,
                                     int n_radii, const int32_t* roi_q, int border, int cell_side_q, const uint8_t* mask, int mask_cell,
                                     int64_t* pairs, int32_t* centres, int32_t* nn, int32_t* bd, int32_t* stats, void* workspace,
                                     size_t workspace_bytes, ay_stream_t stream) {
    return ay::pair_counts_run("ay_pair_counts_window", true, rows, n_rows, num_classes, slide_h, slide_w, min_conf, radii_q, n_radii, roi_q, border,
                               cell_side_q, mask, mask_cell, pairs, centres, nn, bd, stats, workspace, workspace_bytes, stream);
}

extern "C" size_t ay_pair_counts_relabel_workspace_bytes(int n_rows, int num_classes, int n_radii, int slide_h, int slide_w, int r_max_q,
                                                         int cell_side_q, int mask_cell, int n_sims) {
    if (num_classes < 1 || num_classes > AY_PAIR_MAX_CLASSES || n_radii < 1 || n_radii > AY_PAIR_MAX_RADII || n_sims < 1 ||
        n_sims > AY_PAIR_RELABEL_MAX_SIMS)
        return 0;
    return ay::pair_workspace_bytes(n_rows, slide_h, slide_w, r_max_q, cell_side_q, mask_cell != 0, mask_cell, true);
}

extern "C" int ay_pair_counts_relabel(const float* rows, int n_rows, int num_classes, int slide_h, int slide_w, float min_conf,
                                      const int32_t* radii_q, int n_radii, const int32_t* roi_q, int border, int cell_side_q, const uint8_t* mask,
                                      int mask_cell, const uint8_t* labels, int n_sims, int label_stride, int64_t* sim_pairs, int32_t* sim_centres,
                                      int32_t* sim_inside, int32_t* bd, int32_t* stats, void* workspace, size_t workspace_bytes, ay_stream_t stream) {
    const ay::PairRelabel rl = {labels, n_sims, label_stride, sim_pairs, sim_centres, sim_inside};
    return ay::pair_counts_run("ay_pair_counts_relabel", mask != nullptr, rows, n_rows, num_classes, slide_h, slide_w, min_conf, radii_q, n_radii, roi_q,
                               border, cell_side_q, mask, mask_cell, nullptr, nullptr, nullptr, bd, stats, workspace, workspace_bytes, stream, &rl);
}
