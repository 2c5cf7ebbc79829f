// The centre grid of the slide-level box passes (ay_seam.hip over the detection rows, ay_slidematch.hip over the annotated targets),
// and the 256-byte workspace carver they share with ay_burden.hip.
//
// The work of those passes is local (a box only meets boxes near it), so the items are binned by the grid cell of their centre
// (counting sort: histogram, one-workgroup scan, scatter) and a search reads the cells around its own.  The cell side c comes from
// the data: a geometry reduction takes the min / max of the centres and a histogram of ceil(log2(side)); grid_choose takes the
// smallest power of two that all but a handful of items fit into.  Every item its user calls "regular" for that c lies in the
// cell of its centre; all others (larger than a cell, or not finite) form the OVERSIZE list, cell n_cells, the last segment of the
// sorted array.  What is regular, and which cells a search must then read, is the user's: the seam merge and the slide match
// state two different fp32 predicates and each proves its own.  Any cell side gives the same result; the choice is about work.
//
// Templates and helpers only, in the manner of ay_slide_pass.h.  An item policy says how the reduction and the count see an item:
//   float4 box(int i) const             (x1, y1, x2, y2) of item i
//   bool live(float4 b) const           false: the item takes no part (the slide match's ROI)
//   static float extent(lo, hi)         the width / height whose finiteness is tested and whose maximum is binned
//   static float side(w, h)             the value >= 1 whose ceil(log2) is binned
//   static bool regular(float4 b, c)    the item lies in the cell of its centre (else: on the oversize list)
#pragma once
#include <math.h>
#include <string.h>

#include "ay_box.h"
#include "ay_common.h"

namespace ay {

constexpr int GRID_STATS_BLOCKS = 256;   // per-block partials of the geometry reduction (finished on the host)
constexpr int GRID_SIDE_BINS = 32;
constexpr int GRID_STATS_WORDS = 4 + GRID_SIDE_BINS;

struct BoxGrid {
    float x0, y0, c;
    int gx, gy;
    __host__ __device__ int n_cells() const { return gx * gy; }
};

// cell index of a cell coordinate, clamped into 0 .. n - 1.  The last step is on integers: (float)(n - 1) rounds up to n for some
// n above 2^24, and an index n would be the first cell of the next grid row.
__device__ __forceinline__ int grid_clamp_cell(float f, int n) { return min((int)fminf(fmaxf(f, 0.0f), (float)(n - 1)), n - 1); }

// cell coordinate of the position v on one axis: floor((v - x0) / c), clamped.  Every step is monotone in v (the library is built
// with -ffp-contract=off, so the steps are the ones written here: do not reorder them).  The slide match rests on that: a row's
// cell bounds go through this expression as a target's centre does, so a centre inside an interval cannot land in a cell outside
// the cells of the interval's ends.
__device__ __forceinline__ int grid_cell_coord(float v, float x0, float c, int n) { return grid_clamp_cell(floorf((v - x0) / c), n); }

__device__ __forceinline__ int grid_cell_of_centre(float x1, float y1, float x2, float y2, const BoxGrid g) {
    return grid_cell_coord((y1 + y2) * 0.5f, g.y0, g.c, g.gy) * g.gx + grid_cell_coord((x1 + x2) * 0.5f, g.x0, g.c, g.gx);
}

// sum of v over the 256 threads of the workgroup; every thread calls it (two barriers), from a workgroup-uniform place
__device__ __forceinline__ int block_sum_256(int v, int* red /* [4] */) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// per-block partials over the live items with finite coordinates: min / max of the centres (4 floats) and a histogram of the sides
// (GRID_SIDE_BINS ints; bin k counts the items with 2^(k-1) < side <= 2^k).  Integer counts and min / max: the partials are the
// same bytes in every run.
template <typename Items>
__global__ void __launch_bounds__(256) grid_stats_kernel(Items items, int n, float* __restrict__ partials) {
    __shared__ float sh[256];
    __shared__ int hist[GRID_SIDE_BINS];
    if (threadIdx.x < GRID_SIDE_BINS) hist[threadIdx.x] = 0;
    __syncthreads();
    float mnx = 3.0e38f, mxx = -3.0e38f, mny = 3.0e38f, mxy = -3.0e38f;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += GRID_STATS_BLOCKS * 256) {
        const float4 b = items.box(i);
        const float x1 = b.x, y1 = b.y, x2 = b.z, y2 = b.w;
        const float w = Items::extent(x1, x2), h = Items::extent(y1, y2);
        if (!items.live(b)) continue;
        if (!(finite_f(x1) && finite_f(y1) && finite_f(x2) && finite_f(y2) && finite_f(w) && finite_f(h))) continue;
        const float cx = (x1 + x2) * 0.5f, cy = (y1 + y2) * 0.5f;
        mnx = fminf(mnx, cx), mxx = fmaxf(mxx, cx), mny = fminf(mny, cy), mxy = fmaxf(mxy, cy);
        const int bits = __float_as_int(Items::side(w, h));                    // >= 1: exponent >= 0
        const int bin = ((bits >> 23) & 255) - 127 + ((bits & 0x7fffff) != 0);  // ceil(log2(side))
        atomicAdd(&hist[min(bin, GRID_SIDE_BINS - 1)], 1);
    }
    float v[4] = {mnx, mxx, mny, mxy};
    for (int q = 0; q < 4; ++q) {
        __syncthreads();
        sh[threadIdx.x] = v[q];
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (threadIdx.x < o) {
                const float a = sh[threadIdx.x], b = sh[threadIdx.x + o];
                sh[threadIdx.x] = (q & 1) ? fmaxf(a, b) : fminf(a, b);
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) partials[blockIdx.x * GRID_STATS_WORDS + q] = sh[0];
    }
    if (threadIdx.x < GRID_SIDE_BINS) partials[blockIdx.x * GRID_STATS_WORDS + 4 + threadIdx.x] = __int_as_float(hist[threadIdx.x]);
}

// ---- the counting sort: count, scan, scatter.  cell_start and cursor hold n_cells + 2 words, zeroed before the count.
template <typename Items>
__device__ __forceinline__ int grid_cell(const float4 b, const BoxGrid g) {   // the cell of a live item; n_cells: the oversize list
    return Items::regular(b, g.c) ? grid_cell_of_centre(b.x, b.y, b.z, b.w, g) : g.n_cells();
}
__device__ __forceinline__ void grid_count(int i, int c, int32_t* __restrict__ cell_of, int32_t* __restrict__ cell_start) {
    cell_of[i] = c;
    atomicAdd(&cell_start[c], 1);
}
// place of the next item of cell c in the sorted array (an integer atomic: the order inside a cell is any)
__device__ __forceinline__ int grid_slot(int c, const int32_t* __restrict__ cell_start, int32_t* __restrict__ cursor) {
    return cell_start[c] + atomicAdd(&cursor[c], 1);
}

// exclusive scan of a[0 .. n) in place, a[n] = total; one workgroup of 1024, a contiguous chunk per thread
static __global__ void __launch_bounds__(1024) grid_scan_kernel(int32_t* __restrict__ a, int n) {
    __shared__ int sums[1024];
    const int chunk = (n + 1023) / 1024;
    const int lo = min(threadIdx.x * chunk, n), hi = min(lo + chunk, n);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += a[i];
    sums[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {   // Hillis-Steele inclusive scan of the 1024 chunk sums
        const int v = threadIdx.x >= o ? sums[threadIdx.x - o] : 0;
        __syncthreads();
        sums[threadIdx.x] += v;
        __syncthreads();
    }
    int run = sums[threadIdx.x] - s;
    for (int i = lo; i < hi; ++i) {
        const int v = a[i];
        a[i] = run;
        run += v;
    }
    if (threadIdx.x == 1023) a[n] = sums[1023];
}

// cells of the grid at most (cell indices stay in int32)
static inline size_t grid_cell_cap(int n) {
    const size_t want = (size_t)(n > 2048 ? n : 2048) * 2;
    return want < ((size_t)1 << 30) ? want : ((size_t)1 << 30);
}

// Cell side and grid from the reduction's partials over n items.  Without a caller's cell_side (<= 0): the smallest power of two
// (>= 8) that leaves at most max(16, n / 4096) items oversize: a handful of outliers (a box as large as a tile) must not blow the
// cells up for everyone, and the oversize list, which every search reads in full, stays a vanishing share of the items.  (An
// estimate of pair tests, 9 c^2 n / area per regular item + the oversize list, minimised over c, was measured against this rule on
// a slide with a heavy tail of large boxes: 61 ms against 31 ms of seam round kernels.)  unbinned_oversize: the items the
// reduction left out count as oversize whatever the cell (the seam merge's rows that are not finite); false where they are on no
// list at all (the slide match's ignored targets).  The side is then doubled until the grid over the centres' extent fits
// cell_cap cells: one item far from all others costs larger cells, never an unbounded grid.
static inline BoxGrid grid_choose(const float* partials, int n, bool unbinned_oversize, size_t cell_cap, float cell_side) {
    double mnx = 3.0e38, mxx = -3.0e38, mny = 3.0e38, mxy = -3.0e38;
    long long hist[GRID_SIDE_BINS] = {0}, cnt = 0;
    for (int b = 0; b < GRID_STATS_BLOCKS; ++b) {
        const float* v = partials + b * GRID_STATS_WORDS;
        mnx = fmin(mnx, v[0]), mxx = fmax(mxx, v[1]), mny = fmin(mny, v[2]), mxy = fmax(mxy, v[3]);
        for (int k = 0; k < GRID_SIDE_BINS; ++k) {
            int32_t m;
            memcpy(&m, v + 4 + k, sizeof(m));
            hist[k] += m, cnt += m;
        }
    }
    BoxGrid g = {0.0f, 0.0f, cell_side > 0.0f ? cell_side : 8.0f, 1, 1};
    if (cnt < 1) return g;   // nothing binned: one cell, possibly an oversize list
    double c = cell_side;
    if (!(cell_side > 0.0f)) {
        const long long allowed = n / 4096 > 16 ? n / 4096 : 16;
        int bin = GRID_SIDE_BINS - 2;   // (the last bin is open-ended: never taken for "fits")
        long long above = hist[GRID_SIDE_BINS - 1] + (unbinned_oversize ? (long long)n - cnt : 0);
        while (bin > 3 && above + hist[bin] <= allowed) above += hist[bin--];
        c = ldexp(1.0, bin);
    }
    for (;;) {
        const double nx = floor((mxx - mnx) / c) + 1.0, ny = floor((mxy - mny) / c) + 1.0;
        if (nx * ny <= (double)cell_cap) {
            g.x0 = (float)mnx, g.y0 = (float)mny, g.c = (float)c, g.gx = (int)nx, g.gy = (int)ny;
            return g;
        }
        c *= 2.0;
    }
}

// ---- a workspace handed out in pieces that start on multiples of 256 bytes; base may be null where only bytes() is wanted
struct WsCarver {
    char* base;
    size_t off;
    explicit WsCarver(void* ws) : base((char*)ws), off(0) {}
    template <typename T>
    T* take(size_t count) {
        T* p = (T*)(base + off);
        off += (sizeof(T) * count + 255) & ~(size_t)255;
        return p;
    }
    size_t bytes() const { return off; }
};

}  // namespace ay
