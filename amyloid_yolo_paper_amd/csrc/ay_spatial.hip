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
#include <limits.h>

#include "ay_box_grid.h"

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

// one lane per row: THE PAIR RULE up to the position; row_q = (qx, qy), row_ck = class | (kmax + 1) << 8 for the scatter
__global__ void __launch_bounds__(PAIR_THREADS) pair_count_kernel(const float* __restrict__ rows, int M, int C, int q_max_x, int q_max_y, float min_conf,
                                                                   PairRadii rad, PairWindow win, PairGrid g, int32_t* __restrict__ cell_of,
                                                                   int32_t* __restrict__ cell_start, int2* __restrict__ row_q,
                                                                   int32_t* __restrict__ row_ck, int32_t* __restrict__ bd,
                                                                   int32_t* __restrict__ centres, int32_t* __restrict__ stats) {
    __shared__ int sh[2 * AY_PAIR_MAX_CLASSES + 3];                  // counted per class, inside per class, below, flagged, flag bits
    __shared__ int cen[AY_PAIR_MAX_CLASSES * AY_PAIR_MAX_RADII];     // rows of class a whose largest eligible k is kmax
    const int B = rad.n;
    for (int k = threadIdx.x; k < 2 * C + 3; k += PAIR_THREADS) sh[k] = 0;
    for (int k = threadIdx.x; k < C * B; k += PAIR_THREADS) cen[k] = 0;
    __syncthreads();
    const long long i = (long long)blockIdx.x * PAIR_THREADS + threadIdx.x;
    if (i < M) {
        const float* r = rows + (size_t)i * 7;
        const float x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3], conf = r[4], label = r[6];
        const float cx = (x1 + x2) * 0.5f, cy = (y1 + y2) * 0.5f;
        int flags = 0, c = -1;
        if (!(pair_finite(cx) && pair_finite(cy))) flags |= AY_BURDEN_FLAG_NONFINITE;
        if (label >= 0.0f && label < (float)C) {
            c = (int)label;
            if ((float)c != label) c = -1;
        }
        if (c < 0) flags |= AY_BURDEN_FLAG_CLASS;
        if (flags) {
            atomicAdd(&sh[2 * C + 1], 1);
            atomicOr(&sh[2 * C + 2], flags);
            cell_of[i] = -1;
        } else if (!(conf >= min_conf)) {
            atomicAdd(&sh[2 * C], 1);
            cell_of[i] = -1;
        } else {
            const int qx = pair_position(cx, q_max_x), qy = pair_position(cy, q_max_y);
            const int d = min(min(qx - win.x1, win.x2 - qx), min(qy - win.y1, win.y2 - qy));
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

struct PairWs {
    int32_t *cell_of, *row_ck, *sqx, *sqy, *sorig, *cell_start, *cursor, *chunk_sum;
    int2* row_q;
    uint8_t* scls;
    int8_t* skmax;
    size_t bytes;
};

static PairWs pair_carve(void* ws, int n_rows, size_t n_cells) {
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

}  // namespace ay

extern "C" size_t ay_pair_counts_workspace_bytes(int n_rows, int slide_h, int slide_w, int r_max_q, int cell_side_q) {
    ay::PairGrid g;
    if (!ay::pair_dims_ok(n_rows, slide_h, slide_w, r_max_q, cell_side_q) || !ay::pair_grid(n_rows, slide_h, slide_w, r_max_q, cell_side_q, &g)) return 0;
    return ay::pair_carve(nullptr, n_rows, (size_t)g.n_cells()).bytes;
}

extern "C" int ay_pair_counts(const float* rows, int n_rows, int num_classes, int slide_h, int slide_w, float min_conf, const int32_t* radii_q,
                              int n_radii, const int32_t* roi_q, int border, int cell_side_q, int64_t* pairs, int32_t* centres, int32_t* nn,
                              int32_t* bd, int32_t* stats, void* workspace, size_t workspace_bytes, ay_stream_t stream) {
    using namespace ay;
    const int M = n_rows, C = num_classes, B = n_radii, H = slide_h, W = slide_w;
    AY_CHECK_ARG(M >= 0 && (M == 0 || rows), "ay_pair_counts: n_rows %d%s", M, rows ? "" : " with null rows");
    AY_CHECK_ARG(C >= 1 && C <= AY_PAIR_MAX_CLASSES, "ay_pair_counts: num_classes %d outside 1 .. %d", C, AY_PAIR_MAX_CLASSES);
    AY_CHECK_ARG(H >= 1 && W >= 1 && H <= AY_PAIR_MAX_SIDE && W <= AY_PAIR_MAX_SIDE, "ay_pair_counts: slide %d x %d outside 1 .. %d", H, W,
                 AY_PAIR_MAX_SIDE);
    AY_CHECK_ARG(radii_q && B >= 1 && B <= AY_PAIR_MAX_RADII, "ay_pair_counts: n_radii %d outside 1 .. %d", B, AY_PAIR_MAX_RADII);
    PairRadii rad;
    rad.n = B;
    for (int k = 0; k < AY_PAIR_MAX_RADII; ++k) rad.r[k] = k < B ? radii_q[k] : INT_MAX;
    for (int k = 0; k < B; ++k)
        AY_CHECK_ARG(rad.r[k] >= 1 && rad.r[k] <= AY_PAIR_MAX_RADIUS_Q && (k == 0 || rad.r[k] > rad.r[k - 1]),
                     "ay_pair_counts: radii[%d] = %d: the radii ascend strictly inside 1 .. %d quarter pixels", k, rad.r[k], AY_PAIR_MAX_RADIUS_Q);
    const int r_max = rad.r[B - 1];
    PairWindow win = {0, 0, 4 * W - 1, 4 * H - 1, border ? 1 : 0};
    if (roi_q) win.x1 = roi_q[0], win.y1 = roi_q[1], win.x2 = roi_q[2], win.y2 = roi_q[3];
    AY_CHECK_ARG(win.x1 <= win.x2 && win.y1 <= win.y2, "ay_pair_counts: roi (%d, %d, %d, %d) is empty", win.x1, win.y1, win.x2, win.y2);
    // (the border distance subtracts a position in 0 .. 2^23 from a bound: keep the bounds where that cannot overflow)
    AY_CHECK_ARG(win.x1 >= -(1 << 30) && win.y1 >= -(1 << 30) && win.x2 <= (1 << 30) && win.y2 <= (1 << 30), "ay_pair_counts: roi beyond +-2^30");
    AY_CHECK_ARG(cell_side_q <= 0 || cell_side_q >= r_max, "ay_pair_counts: cell_side %d below the largest radius %d", cell_side_q, r_max);
    PairGrid g;
    AY_CHECK_ARG(pair_grid(M, H, W, r_max, cell_side_q, &g), "ay_pair_counts: cell_side %d gives more than 2^30 cells", cell_side_q);
    AY_CHECK_ARG(pairs && centres && stats && workspace && (M == 0 || (nn && bd)), "ay_pair_counts: null output or workspace");
    const int n_cells = g.n_cells();
    const PairWs w = pair_carve(workspace, M, (size_t)n_cells);
    AY_CHECK_ARG(workspace_bytes >= w.bytes, "ay_pair_counts: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
    AY_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "ay_pair_counts: workspace not 16-byte aligned");
    hipStream_t st = S(stream);
    const long long n_nn = (long long)M * C * 2;
    const long long most = n_nn > n_cells + 2 ? n_nn : n_cells + 2;
    hipLaunchKernelGGL(pair_fill_kernel, dim3(pair_blocks(most, 4096)), dim3(PAIR_THREADS), 0, st, w.cell_start, w.cursor, n_cells + 2, pairs, C * C * B,
                       centres, C * B, stats, 2 * C + 3, nn, n_nn, bd, M);
    AY_CHECK_LAUNCH("pair_fill_kernel");
    if (M > 0) {
        const unsigned rblocks = (unsigned)(((long long)M + PAIR_THREADS - 1) / PAIR_THREADS);
        hipLaunchKernelGGL(pair_count_kernel, dim3(rblocks), dim3(PAIR_THREADS), 0, st, rows, M, C, 4 * W - 1, 4 * H - 1, min_conf, rad, win, g, w.cell_of,
                           w.cell_start, w.row_q, w.row_ck, bd, centres, stats);
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
        hipLaunchKernelGGL(pair_search_kernel, dim3(pair_blocks((long long)M * PAIR_GROUP, PAIR_SEARCH_BLOCKS)), dim3(PAIR_THREADS), pair_search_lds(C, B), st, rad,
                           r_max, C, g, (const int32_t*)w.cell_start, (const int32_t*)w.sqx, (const int32_t*)w.sqy, (const uint8_t*)w.scls,
                           (const int8_t*)w.skmax, (const int32_t*)w.sorig, pairs, nn);
        AY_CHECK_LAUNCH("pair_search_kernel");
    }
    return AY_OK;
}
