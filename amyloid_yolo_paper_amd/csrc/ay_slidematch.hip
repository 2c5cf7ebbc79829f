// Slide-level matching of detections against annotations (stats.match_slide, wsi.evaluate_region): the true-positive rule of
// get_batch_statistics (utils/utils.py:154-190) for ONE image of any size -- a whole slide with 10^4 .. 10^5 annotated objects and
// a few 10^5 detection rows -- where ay_match_detections (one wavefront per image, 2048 targets in LDS) cannot go.
//
// THE SLIDE MATCH RULE is stated in include/amyloid_yolo.h; tests/slide_match_reference.py restates it on the CPU as the reference
// writes it (sort, then a sequential walk with a claimed set).
//
// HOW.  The walk only looks sequential.  A row's candidate is its own first-maximum IoU target whatever earlier rows did; rows are
// coupled only through which of them reaches a target first.  So the rule is an argmax per row and a minimum per target:
//   1. the non-ignored targets are binned by the grid cell of their centre (counting sort: histogram, one-workgroup scan, scatter;
//      the original index travels with the box, the tie-break needs it).  A target with x2 - x1 or y2 - y1 above c - 2 (c = the cell
//      side), or with a coordinate that is not finite, goes to the OVERSIZE list behind the last cell.
//   2. one lane per row scans the cells that can hold the centre of a regular target sharing a pixel with the row, plus the oversize
//      list, and keeps the maximum by (IoU descending, original index ascending): torch's first maximum.  A target shares a pixel
//      with the row only if tx2 > rx1 - 1 and tx1 < rx2 + 1; with a width of at most c - 2 its centre then lies inside
//      (rx1 - c / 2, rx2 + c / 2).  The scanned interval is wider by a slack of 2 px + 2^-20 of the magnitudes involved, which
//      covers every fp32 rounding on the way, and the row's cell bounds go through the same expression floor((v - x0) / c) as the
//      target's cell -- every step of it is monotone in v, so a centre inside the interval cannot land in a cell outside the range.
//      Both are clamped into the grid the same way.  A row whose range exceeds SLIDE_WIDE_CELLS cells (a box over half the slide) is
//      scanned by its whole wavefront instead of one lane.
//      Whatever the cell side, the cells scanned hold every target with a positive IoU, so the result does not depend on it.
//   3. an eligible row takes part in claim_key[k][best_target] = min over ((0xFFFFFFFF - score bits) << 32 | row index): one 64-bit
//      vector atomic per row and threshold.  The minimum is the first eligible row in rank order (scores are >= +0, so their bits
//      order like the values).
//   4. a last kernel turns the keys into claim / tp and counts.
// Integer atomics and min / max only: the same bytes on every run, whatever order the threads or the scatter's cursor take.
#include <math.h>
#include <string.h>

#include "ay_box.h"
#include "ay_common.h"

namespace ay {

constexpr int SLIDE_STATS_BLOCKS = 256;   // per-block partials of the geometry reduction (finished on the host)
constexpr int SLIDE_SIDE_BINS = 32;
constexpr int SLIDE_STATS_WORDS = 4 + SLIDE_SIDE_BINS;
constexpr int SLIDE_WIDE_CELLS = 32;      // a row whose cell range is larger is scanned by its wavefront

struct SlideGrid {
    float x0, y0, c;
    int gx, gy;
};
struct SlideRoi {
    int on;
    float x1, y1, x2, y2;
};
struct SlideThres {
    int n;
    float v[AY_SLIDE_MAX_THRES];
};

// ROI: ignored iff the centre lies outside the closed rectangle (a NaN centre is outside)
__device__ __forceinline__ bool slide_ignored(const SlideRoi roi, float x1, float y1, float x2, float y2) {
    if (!roi.on) return false;
    const float cx = (x1 + x2) * 0.5f, cy = (y1 + y2) * 0.5f;
    return !(cx >= roi.x1 && cx <= roi.x2 && cy >= roi.y1 && cy <= roi.y2);
}

// the IoU of ay_match_detections (ay_stats.hip): the same function
__device__ __forceinline__ float slide_iou(float ax1, float ay1, float ax2, float ay2, const float4 b) {
    return iou_p1(ax1, ay1, ax2, ay2, b.x, b.y, b.z, b.w);
}

// class id of a label: an integer in 0 .. AY_SLIDE_MAX_CLASSES - 1, or -1
__device__ __forceinline__ int slide_class(float v) {
    if (!(v >= 0.0f && v < (float)AY_SLIDE_MAX_CLASSES)) return -1;
    const int c = (int)v;
    return (float)c == v ? c : -1;
}

// cell index of a cell coordinate, clamped into 0 .. n - 1.  The last step is on integers: (float)(n - 1) rounds up to n for some
// n above 2^24, and an index n would be the first cell of the next grid row.
__device__ __forceinline__ int slide_clamp_cell(float f, int n) { return min((int)fminf(fmaxf(f, 0.0f), (float)(n - 1)), n - 1); }

// per-block partials over the non-ignored targets with finite coordinates: min / max of the centres (4 floats) and a histogram of
// the sides (bin k counts the targets with 2^(k-1) < max(x2 - x1, y2 - y1, 0) + 2 <= 2^k)
__global__ void __launch_bounds__(256) slide_stats_kernel(const float* __restrict__ targets, int T, SlideRoi roi, float* __restrict__ partials) {
    __shared__ float sh[256];
    __shared__ int hist[SLIDE_SIDE_BINS];
    if (threadIdx.x < SLIDE_SIDE_BINS) hist[threadIdx.x] = 0;
    __syncthreads();
    float mnx = 3.0e38f, mxx = -3.0e38f, mny = 3.0e38f, mxy = -3.0e38f;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < T; t += SLIDE_STATS_BLOCKS * 256) {
        const float* r = targets + (size_t)t * 5;
        const float x1 = r[1], y1 = r[2], x2 = r[3], y2 = r[4];
        const float w = x2 - x1, h = y2 - y1;
        if (slide_ignored(roi, x1, y1, x2, y2)) continue;
        if (!(finite_f(x1) && finite_f(y1) && finite_f(x2) && finite_f(y2) && finite_f(w) && finite_f(h))) continue;
        const float cx = (x1 + x2) * 0.5f, cy = (y1 + y2) * 0.5f;
        mnx = fminf(mnx, cx), mxx = fmaxf(mxx, cx), mny = fminf(mny, cy), mxy = fmaxf(mxy, cy);
        const int bits = __float_as_int(fmaxf(fmaxf(w, h), 0.0f) + 2.0f);     // >= 2: exponent >= 1
        const int bin = ((bits >> 23) & 255) - 127 + ((bits & 0x7fffff) != 0);  // ceil(log2(side + 2))
        atomicAdd(&hist[min(bin, SLIDE_SIDE_BINS - 1)], 1);
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
        if (threadIdx.x == 0) partials[blockIdx.x * SLIDE_STATS_WORDS + q] = sh[0];
    }
    if (threadIdx.x < SLIDE_SIDE_BINS) partials[blockIdx.x * SLIDE_STATS_WORDS + 4 + threadIdx.x] = __int_as_float(hist[threadIdx.x]);
}

// per target: the ignored flag, its cell (-1 = ignored, n_cells = oversize), the cell histogram and the class-presence flag
__global__ void __launch_bounds__(256) slide_bin_count_kernel(const float* __restrict__ targets, int T, SlideRoi roi, SlideGrid g,
                                                               uint8_t* __restrict__ target_ignored, int32_t* __restrict__ cell_of,
                                                               int32_t* __restrict__ cell_start, int32_t* __restrict__ class_flags,
                                                               int32_t* __restrict__ flags_out) {
    const int t = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const bool in = t < T;
    float cls_f = -1.0f, x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
    if (in) {
        const float* r = targets + (size_t)t * 5;
        cls_f = r[0], x1 = r[1], y1 = r[2], x2 = r[3], y2 = r[4];
    }
    const bool live = in && !slide_ignored(roi, x1, y1, x2, y2);
    // class presence: one atomic per wavefront and distinct class (a slide has a few classes: one atomic per target would queue
    // every target of the slide on two or three words)
    const int cls = slide_class(cls_f);
    bool pending = live && cls >= 0;
    for (unsigned long long todo = __ballot(pending); todo; todo = __ballot(pending)) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lc = __shfl(cls, leader);
        if (pending && cls == lc) {
            pending = false;
            if (lane == leader) atomicOr(&class_flags[lc], 1);
        }
    }
    if (!in) return;
    target_ignored[t] = (uint8_t)!live;
    if (!live) {
        cell_of[t] = -1;
        return;
    }
    if (cls < 0) atomicOr(flags_out, AY_SLIDE_FLAG_CLASS);
    int c = g.gx * g.gy;
    const float w = x2 - x1, h = y2 - y1;
    if (w <= g.c - 2.0f && h <= g.c - 2.0f && finite_f(x1) && finite_f(y1) && finite_f(x2) && finite_f(y2)) {
        const float fx = floorf(((x1 + x2) * 0.5f - g.x0) / g.c), fy = floorf(((y1 + y2) * 0.5f - g.y0) / g.c);
        c = slide_clamp_cell(fy, g.gy) * g.gx + slide_clamp_cell(fx, g.gx);
    }
    cell_of[t] = c;
    atomicAdd(&cell_start[c], 1);
}

// exclusive scan of a[0 .. n) in place, a[n] = total; one workgroup, a contiguous chunk per thread
__global__ void __launch_bounds__(1024) slide_scan_kernel(int32_t* __restrict__ a, int n) {
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

__global__ void __launch_bounds__(256) slide_scatter_kernel(const float* __restrict__ targets, int T, const int32_t* __restrict__ cell_of,
                                                             const int32_t* __restrict__ cell_start, int32_t* __restrict__ cursor,
                                                             float4* __restrict__ box, int32_t* __restrict__ orig) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int c = cell_of[t];
    if (c < 0) return;
    const int p = cell_start[c] + atomicAdd(&cursor[c], 1);
    const float* r = targets + (size_t)t * 5;
    box[p] = make_float4(r[1], r[2], r[3], r[4]);
    orig[p] = t;
}

// first maximum by (IoU descending, original index ascending) among the targets with a positive IoU; (0, -1) while there is none
__device__ __forceinline__ void slide_take(float v, int idx, float& best, int& arg) {
    if (v > best || (v == best && v > 0.0f && idx < arg)) {
        best = v;
        arg = idx;
    }
}

__device__ __forceinline__ void slide_scan_range(int lo, int hi, int stride, float x1, float y1, float x2, float y2,
                                                  const float4* __restrict__ box, const int32_t* __restrict__ orig, float& best, int& arg) {
    for (int q = lo; q < hi; q += stride) slide_take(slide_iou(x1, y1, x2, y2, box[q]), orig[q], best, arg);
}

// one lane per row: best target, eligibility per threshold, claim keys
__global__ void __launch_bounds__(256) slide_match_kernel(const float* __restrict__ rows, int M, int T, SlideRoi roi, SlideGrid g, SlideThres thr,
                                                           const float4* __restrict__ box, const int32_t* __restrict__ orig,
                                                           const int32_t* __restrict__ cell_start, const int32_t* __restrict__ class_flags,
                                                           float* __restrict__ best_iou, int32_t* __restrict__ best_target,
                                                           uint8_t* __restrict__ row_ignored, uint32_t* __restrict__ elig,
                                                           unsigned long long* __restrict__ claim_key) {
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const bool in = i < M;
    float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f, conf = 0.f, cls_conf = 0.f, label = -1.f;
    if (in) {
        const float* r = rows + (size_t)i * 7;
        x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3], conf = r[4], cls_conf = r[5], label = r[6];
    }
    const bool ign = in && slide_ignored(roi, x1, y1, x2, y2);
    const bool live = in && !ign;
    const int n_cells = g.gx * g.gy;
    const int over_lo = cell_start[n_cells], over_hi = cell_start[n_cells + 1];
    // cells whose regular targets can share a pixel with the row (see the head of the file)
    const float sx = 2.0f + (fabsf(x1) + fabsf(x2) + fabsf(g.x0) + g.c) * 0x1p-20f;
    const float sy = 2.0f + (fabsf(y1) + fabsf(y2) + fabsf(g.y0) + g.c) * 0x1p-20f;
    const int xa = slide_clamp_cell(floorf((x1 - 0.5f * g.c - sx - g.x0) / g.c), g.gx);
    const int xb = slide_clamp_cell(floorf((x2 + 0.5f * g.c + sx - g.x0) / g.c), g.gx);
    const int ya = slide_clamp_cell(floorf((y1 - 0.5f * g.c - sy - g.y0) / g.c), g.gy);
    const int yb = slide_clamp_cell(floorf((y2 + 0.5f * g.c + sy - g.y0) / g.c), g.gy);
    const bool wide = live && (long long)(xb - xa + 1) * (yb - ya + 1) > SLIDE_WIDE_CELLS;
    float best = 0.0f;
    int arg = -1;
    if (live && !wide) {
        for (int y = ya; y <= yb; ++y)   // the cells xa .. xb of a grid row are one range of the sorted array
            slide_scan_range(cell_start[y * g.gx + xa], cell_start[y * g.gx + xb + 1], 1, x1, y1, x2, y2, box, orig, best, arg);
        slide_scan_range(over_lo, over_hi, 1, x1, y1, x2, y2, box, orig, best, arg);
    }
    // wide rows, one after the other, by the whole wavefront (every lane of the wavefront is here: nobody has returned)
    for (unsigned long long todo = __ballot(wide); todo; todo &= todo - 1) {
        const int src = __ffsll((long long)todo) - 1;
        const float wx1 = __shfl(x1, src), wy1 = __shfl(y1, src), wx2 = __shfl(x2, src), wy2 = __shfl(y2, src);
        const int wxa = __shfl(xa, src), wxb = __shfl(xb, src), wya = __shfl(ya, src), wyb = __shfl(yb, src);
        float b = 0.0f;
        int a = -1;
        for (int y = wya; y <= wyb; ++y)
            slide_scan_range(cell_start[y * g.gx + wxa] + lane, cell_start[y * g.gx + wxb + 1], 64, wx1, wy1, wx2, wy2, box, orig, b, a);
        slide_scan_range(over_lo + lane, over_hi, 64, wx1, wy1, wx2, wy2, box, orig, b, a);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ob = __shfl_xor(b, off);
            const int oa = __shfl_xor(a, off);
            slide_take(ob, oa, b, a);
        }
        if (lane == src) {
            best = b;
            arg = a;
        }
    }
    if (!in) return;
    best_iou[i] = best;
    best_target[i] = arg;
    row_ignored[i] = (uint8_t)ign;
    const int cls = slide_class(label);
    const bool present = live && cls >= 0 && class_flags[cls] != 0;
    const float score = conf * cls_conf + 0.0f;   // (-0 becomes +0: the bits then order like the values)
    const unsigned long long key = ((unsigned long long)(0xFFFFFFFFu - __float_as_uint(score)) << 32) | (unsigned)i;
    uint32_t mask = 0;
    for (int k = 0; k < thr.n; ++k) {
        if (present && best >= thr.v[k]) {   // thr > 0: arg >= 0 here
            mask |= 1u << k;
            atomicMin(&claim_key[(size_t)k * T + arg], key);
        }
    }
    elig[i] = mask;
}

// tp of every row and claim of every target at every threshold, grid-stride; the counts go through registers, a wave shuffle and
// LDS to one atomic per workgroup, threshold and counter; thread 0 adds the number of oversize targets
constexpr int SLIDE_FINISH_BLOCKS = 256;
__global__ void __launch_bounds__(256) slide_finish_kernel(int M, int T, int K, int n_cells, const uint32_t* __restrict__ elig,
                                                            const int32_t* __restrict__ best_target,
                                                            const unsigned long long* __restrict__ claim_key,
                                                            const int32_t* __restrict__ cell_start, uint8_t* __restrict__ tp,
                                                            int32_t* __restrict__ claim, int32_t* __restrict__ stats) {
    __shared__ int red[2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long n = M > T ? M : T, stride = (long long)gridDim.x * 256;
    for (int k = 0; k < K; ++k) {
        int n_elig = 0, n_claimed = 0;
        for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < n; j += stride) {
            if (j < M) {
                const bool e = (elig[j] >> k) & 1;
                bool hit = false;
                if (e) hit = (uint32_t)claim_key[(size_t)k * T + best_target[j]] == (uint32_t)j;   // e: best_target >= 0
                tp[(size_t)k * M + j] = (uint8_t)hit;
                n_elig += e;
            }
            if (j < T) {
                const unsigned long long key = claim_key[(size_t)k * T + j];
                const bool claimed = key != ~0ull;
                claim[(size_t)k * T + j] = claimed ? (int32_t)(uint32_t)key : -1;
                n_claimed += claimed;
            }
        }
        for (int o = 32; o > 0; o >>= 1) n_elig += __shfl_down(n_elig, o, 64), n_claimed += __shfl_down(n_claimed, o, 64);
        __syncthreads();
        if (lane == 0) red[0][wave] = n_elig, red[1][wave] = n_claimed;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int e = red[0][0] + red[0][1] + red[0][2] + red[0][3], c = red[1][0] + red[1][1] + red[1][2] + red[1][3];
            if (e) atomicAdd(&stats[2 * k], e);
            if (c) atomicAdd(&stats[2 * k + 1], c);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) stats[2 * K + 1] = cell_start[n_cells + 1] - cell_start[n_cells];
}

static inline size_t slide_align(size_t v) { return (v + 255) & ~(size_t)255; }
static inline size_t slide_cell_cap(int n_targets) {   // cells of the grid at most (cell indices stay in int32)
    const size_t want = (size_t)(n_targets > 2048 ? n_targets : 2048) * 2;
    return want < ((size_t)1 << 30) ? want : ((size_t)1 << 30);
}

struct SlideWs {
    float* partials;
    int32_t *class_flags, *cell_of, *orig, *cell_start, *cursor;
    uint32_t* elig;
    unsigned long long* claim_key;
    float4* box;
    size_t bytes;
};

static SlideWs slide_carve(void* ws, int n_rows, int n_targets, int n_thres) {
    SlideWs w;
    size_t off = 0;
    char* base = (char*)ws;
    auto take = [&](size_t bytes) {
        char* p = base + off;
        off += slide_align(bytes);
        return p;
    };
    const size_t m = (size_t)(n_rows > 0 ? n_rows : 1), t = (size_t)(n_targets > 0 ? n_targets : 1), cells = slide_cell_cap(n_targets);
    const size_t k = (size_t)(n_thres > 0 ? n_thres : 1);
    w.partials = (float*)take(sizeof(float) * SLIDE_STATS_BLOCKS * SLIDE_STATS_WORDS);
    w.class_flags = (int32_t*)take(4 * (size_t)AY_SLIDE_MAX_CLASSES);
    w.claim_key = (unsigned long long*)take(8 * k * t);
    w.box = (float4*)take(sizeof(float4) * t);
    w.orig = (int32_t*)take(4 * t);
    w.cell_of = (int32_t*)take(4 * t);
    w.elig = (uint32_t*)take(4 * m);
    w.cell_start = (int32_t*)take(4 * (cells + 2));
    w.cursor = (int32_t*)take(4 * (cells + 2));
    w.bytes = off;
    return w;
}

#define AY_SLIDE_HIP(call, what)                                            \
    do {                                                                    \
        hipError_t e_ = (call);                                             \
        if (e_ != hipSuccess) {                                             \
            ay::set_error("%s: %s", what, hipGetErrorString(e_));           \
            return AY_ERR_LAUNCH;                                           \
        }                                                                   \
    } while (0)

// Cell side and grid from the reduction's partials.  Any cell side gives the same result; the choice is about work.  Without a
// caller's side: the smallest power of two (>= 8) that leaves at most max(16, T / 4096) targets oversize (every row tests those in
// full, so a few tile-sized annotations must not blow the cells up for everyone).  The side is doubled until the grid over the
// centres' extent fits cell_cap cells: one target far from all others costs larger cells, never an unbounded grid.
static SlideGrid slide_choose_grid(const float* partials, int T, size_t cell_cap, float cell_side) {
    double mnx = 3.0e38, mxx = -3.0e38, mny = 3.0e38, mxy = -3.0e38;
    long long hist[SLIDE_SIDE_BINS] = {0}, cnt = 0;
    for (int b = 0; b < SLIDE_STATS_BLOCKS; ++b) {
        const float* v = partials + b * SLIDE_STATS_WORDS;
        mnx = fmin(mnx, v[0]), mxx = fmax(mxx, v[1]), mny = fmin(mny, v[2]), mxy = fmax(mxy, v[3]);
        for (int k = 0; k < SLIDE_SIDE_BINS; ++k) {
            int32_t n;
            memcpy(&n, v + 4 + k, sizeof(n));
            hist[k] += n, cnt += n;
        }
    }
    SlideGrid g = {0.0f, 0.0f, cell_side > 0.0f ? cell_side : 8.0f, 1, 1};
    if (cnt < 1) return g;   // no finite non-ignored target: one cell, possibly an oversize list
    double c = cell_side;
    if (!(cell_side > 0.0f)) {
        const long long allowed = T / 4096 > 16 ? T / 4096 : 16;
        int bin = SLIDE_SIDE_BINS - 2;   // (the last bin is open-ended: never taken for "fits")
        long long above = hist[SLIDE_SIDE_BINS - 1];
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

}  // namespace ay

extern "C" size_t ay_slide_match_workspace_bytes(int n_rows, int n_targets, int n_thres) {
    return ay::slide_carve(nullptr, n_rows, n_targets, n_thres).bytes;
}

extern "C" int ay_slide_match(const float* rows, int n_rows, const float* targets, int n_targets, const float* iou_thres, int n_thres,
                              const float* roi, float cell_side, uint8_t* tp, float* best_iou, int32_t* best_target, int32_t* claim,
                              uint8_t* row_ignored, uint8_t* target_ignored, int32_t* stats, void* workspace, size_t workspace_bytes,
                              ay_stream_t stream) {
    using namespace ay;
    const int M = n_rows, T = n_targets, K = n_thres;
    AY_CHECK_ARG(M >= 0 && T >= 0, "ay_slide_match: n_rows %d n_targets %d", M, T);
    AY_CHECK_ARG(iou_thres && K >= 1 && K <= AY_SLIDE_MAX_THRES, "ay_slide_match: n_thres %d outside 1 .. %d", K, AY_SLIDE_MAX_THRES);
    SlideThres thr;
    thr.n = K;
    for (int k = 0; k < AY_SLIDE_MAX_THRES; ++k) thr.v[k] = k < K ? iou_thres[k] : 2.0f;
    for (int k = 0; k < K; ++k) AY_CHECK_ARG(thr.v[k] > 0.0f && thr.v[k] <= 1.0f, "ay_slide_match: iou_thres[%d] = %g outside (0, 1]", k, thr.v[k]);
    AY_CHECK_ARG(!(cell_side > 0.0f) || (cell_side >= 2.0f && cell_side <= 1.0e30f), "ay_slide_match: cell_side %g outside 2 .. 1e30", cell_side);
    AY_CHECK_ARG((unsigned long long)K * (unsigned long long)(T > M ? T : M) < (1ull << 40), "ay_slide_match: n_thres x rows too large");
    AY_CHECK_ARG(stats && workspace, "ay_slide_match: null stats or workspace");
    AY_CHECK_ARG(M == 0 || (rows && tp && best_iou && best_target && row_ignored), "ay_slide_match: null row array");
    AY_CHECK_ARG(T == 0 || (targets && claim && target_ignored), "ay_slide_match: null target array");
    const SlideWs w = slide_carve(workspace, M, T, K);
    AY_CHECK_ARG(workspace_bytes >= w.bytes, "ay_slide_match: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
    AY_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "ay_slide_match: workspace not 16-byte aligned");
    SlideRoi r = {0, 0.f, 0.f, 0.f, 0.f};
    if (roi) r = SlideRoi{1, roi[0], roi[1], roi[2], roi[3]};
    hipStream_t st = S(stream);
    AY_SLIDE_HIP(hipMemsetAsync(stats, 0, sizeof(int32_t) * (2 * K + 2), st), "ay_slide_match: memset");
    AY_SLIDE_HIP(hipMemsetAsync(w.class_flags, 0, sizeof(int32_t) * AY_SLIDE_MAX_CLASSES, st), "ay_slide_match: memset");
    SlideGrid g = {0.0f, 0.0f, 8.0f, 1, 1};
    if (T > 0) {
        const unsigned tblocks = (unsigned)(((long long)T + 255) / 256);
        AY_SLIDE_HIP(hipMemsetAsync(w.claim_key, 0xFF, sizeof(unsigned long long) * (size_t)K * T, st), "ay_slide_match: memset");
        // 1. geometry reduction over the targets -> cell side and grid (host)
        hipLaunchKernelGGL(slide_stats_kernel, dim3(SLIDE_STATS_BLOCKS), dim3(256), 0, st, targets, T, r, w.partials);
        AY_CHECK_LAUNCH("slide_stats_kernel");
        float partials[SLIDE_STATS_BLOCKS * SLIDE_STATS_WORDS];
        AY_SLIDE_HIP(hipMemcpyAsync(partials, w.partials, sizeof(partials), hipMemcpyDeviceToHost, st), "ay_slide_match: copy");
        AY_SLIDE_HIP(hipStreamSynchronize(st), "ay_slide_match: sync");
        g = slide_choose_grid(partials, T, slide_cell_cap(T), cell_side);
        const int n_cells = g.gx * g.gy;
        // 2. counting sort of the non-ignored targets by cell (the oversize list is cell n_cells)
        AY_SLIDE_HIP(hipMemsetAsync(w.cell_start, 0, sizeof(int32_t) * (n_cells + 2), st), "ay_slide_match: memset");
        AY_SLIDE_HIP(hipMemsetAsync(w.cursor, 0, sizeof(int32_t) * (n_cells + 2), st), "ay_slide_match: memset");
        hipLaunchKernelGGL(slide_bin_count_kernel, dim3(tblocks), dim3(256), 0, st, targets, T, r, g, target_ignored, w.cell_of, w.cell_start,
                           w.class_flags, stats + 2 * K);
        AY_CHECK_LAUNCH("slide_bin_count_kernel");
        hipLaunchKernelGGL(slide_scan_kernel, dim3(1), dim3(1024), 0, st, w.cell_start, n_cells + 1);
        AY_CHECK_LAUNCH("slide_scan_kernel");
        hipLaunchKernelGGL(slide_scatter_kernel, dim3(tblocks), dim3(256), 0, st, targets, T, (const int32_t*)w.cell_of,
                           (const int32_t*)w.cell_start, w.cursor, w.box, w.orig);
        AY_CHECK_LAUNCH("slide_scatter_kernel");
    } else {
        AY_SLIDE_HIP(hipMemsetAsync(w.cell_start, 0, sizeof(int32_t) * 3, st), "ay_slide_match: memset");
    }
    // 3. best target per row, claim keys
    if (M > 0) {
        hipLaunchKernelGGL(slide_match_kernel, dim3((unsigned)(((long long)M + 255) / 256)), dim3(256), 0, st, rows, M, T, r, g, thr,
                           (const float4*)w.box, (const int32_t*)w.orig, (const int32_t*)w.cell_start, (const int32_t*)w.class_flags,
                           best_iou, best_target, row_ignored, w.elig, w.claim_key);
        AY_CHECK_LAUNCH("slide_match_kernel");
    }
    // 4. flags, claims, counts
    const long long n = M > T ? M : T;
    if (n > 0) {
        const long long fblocks = (n + 255) / 256;
        hipLaunchKernelGGL(slide_finish_kernel, dim3((unsigned)(fblocks < SLIDE_FINISH_BLOCKS ? fblocks : SLIDE_FINISH_BLOCKS)), dim3(256), 0, st, M, T, K, g.gx * g.gy,
                           (const uint32_t*)w.elig, (const int32_t*)best_target, (const unsigned long long*)w.claim_key,
                           (const int32_t*)w.cell_start, tp, claim, stats);
        AY_CHECK_LAUNCH("slide_finish_kernel");
    }
    return AY_OK;
}
