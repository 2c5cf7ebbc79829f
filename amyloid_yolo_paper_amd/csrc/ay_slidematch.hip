// Slide-level matching of detections against annotations (stats.match_slide, wsi.evaluate_region): the true-positive rule of
// get_batch_statistics (utils/utils.py:154-190) for ONE image of any size -- a whole slide with 10^4 .. 10^5 annotated objects and
// a few 10^5 detection rows -- where ay_match_detections (one wavefront per image, 2048 targets in LDS) cannot go.
//
// THE SLIDE MATCH RULE is stated in include/amyloid_yolo.h; tests/slide_match_reference.py restates it on the CPU as the reference
// writes it (sort, then a sequential walk with a claimed set).
//
// HOW.  The walk only looks sequential.  A row's candidate is its own first-maximum IoU target whatever earlier rows did; rows are
// coupled only through which of them reaches a target first.  So the rule is an argmax per row and a minimum per target:
//   1. the non-ignored targets are binned by ay_box_grid.h (the grid cell of a target's centre; the original index travels with the
//      box, the tie-break needs it).  A target is REGULAR iff x2 - x1 <= c - 2 and y2 - y1 <= c - 2 (c = the cell side) and its four
//      coordinates are finite; the others go to the OVERSIZE list behind the last cell.
//   2. one lane per row scans the cells that can hold the centre of a regular target sharing a pixel with the row, plus the oversize
//      list, and keeps the maximum by (IoU descending, original index ascending): torch's first maximum.  A target shares a pixel
//      with the row only if tx2 > rx1 - 1 and tx1 < rx2 + 1; with a width of at most c - 2 its centre then lies inside
//      (rx1 - c / 2, rx2 + c / 2).  The scanned interval is wider by a slack of 2 px + 2^-20 of the magnitudes involved, which
//      covers every fp32 rounding on the way, and the row's cell bounds go through the same expression as the target's cell
//      (grid_cell_coord) -- every step of it is monotone in v, so a centre inside the interval cannot land in a cell outside the
//      range.  Both are clamped into the grid the same way.  A row whose range exceeds SLIDE_WIDE_CELLS cells (a box over half the slide) is
//      scanned by its whole wavefront instead of one lane.
//      Whatever the cell side, the cells scanned hold every target with a positive IoU, so the result does not depend on it.
//   3. an eligible row takes part in claim_key[k][best_target] = min over ((0xFFFFFFFF - score bits) << 32 | row index): one 64-bit
//      vector atomic per row and threshold.  The minimum is the first eligible row in rank order (scores are >= +0, so their bits
//      order like the values).
//   4. a last kernel turns the keys into claim / tp and counts.
// Integer atomics and min / max only: the same bytes on every run, whatever order the threads or the scatter's cursor take.
#include "ay_box_grid.h"

namespace ay {

constexpr int SLIDE_WIDE_CELLS = 32;      // a row whose cell range is larger is scanned by its wavefront

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

// the targets as the centre grid sees them (ay_box_grid.h): the non-ignored ones, plain sides and 2 px of room in a cell
struct SlideTargets {
    const float* __restrict__ targets;
    SlideRoi roi;
    __device__ __forceinline__ float4 box(int t) const {
        const float* r = targets + (size_t)t * 5;
        return make_float4(r[1], r[2], r[3], r[4]);
    }
    __device__ __forceinline__ bool live(const float4 b) const { return !slide_ignored(roi, b.x, b.y, b.z, b.w); }
    static __device__ __forceinline__ float extent(float lo, float hi) { return hi - lo; }
    static __device__ __forceinline__ float side(float w, float h) { return fmaxf(fmaxf(w, h), 0.0f) + 2.0f; }
    static __device__ __forceinline__ bool regular(const float4 b, float c) {
        const float w = b.z - b.x, h = b.w - b.y;
        return w <= c - 2.0f && h <= c - 2.0f && finite_f(b.x) && finite_f(b.y) && finite_f(b.z) && finite_f(b.w);
    }
};

// per target: the ignored flag, its cell (-1 = ignored, n_cells = oversize), the cell histogram and the class-presence flag
__global__ void __launch_bounds__(256) slide_bin_count_kernel(const float* __restrict__ targets, int T, SlideRoi roi, BoxGrid g,
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
    grid_count(t, grid_cell<SlideTargets>(make_float4(x1, y1, x2, y2), g), cell_of, cell_start);
}

__global__ void __launch_bounds__(256) slide_scatter_kernel(const float* __restrict__ targets, int T, const int32_t* __restrict__ cell_of,
                                                             const int32_t* __restrict__ cell_start, int32_t* __restrict__ cursor,
                                                             float4* __restrict__ box, int32_t* __restrict__ orig) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int c = cell_of[t];
    if (c < 0) return;
    const int p = grid_slot(c, cell_start, cursor);
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
__global__ void __launch_bounds__(256) slide_match_kernel(const float* __restrict__ rows, int M, int T, SlideRoi roi, BoxGrid g, SlideThres thr,
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
    const int n_cells = g.n_cells();
    const int over_lo = cell_start[n_cells], over_hi = cell_start[n_cells + 1];
    // cells whose regular targets can share a pixel with the row (see the head of the file)
    const float sx = 2.0f + (fabsf(x1) + fabsf(x2) + fabsf(g.x0) + g.c) * 0x1p-20f;
    const float sy = 2.0f + (fabsf(y1) + fabsf(y2) + fabsf(g.y0) + g.c) * 0x1p-20f;
    const int xa = grid_cell_coord(x1 - 0.5f * g.c - sx, g.x0, g.c, g.gx);
    const int xb = grid_cell_coord(x2 + 0.5f * g.c + sx, g.x0, g.c, g.gx);
    const int ya = grid_cell_coord(y1 - 0.5f * g.c - sy, g.y0, g.c, g.gy);
    const int yb = grid_cell_coord(y2 + 0.5f * g.c + sy, g.y0, g.c, g.gy);
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

// tp of every row and claim of every target at every threshold, grid-stride; the counts go through registers and block_sum_256 to
// one atomic per workgroup, threshold and counter; thread 0 adds the number of oversize targets
constexpr int SLIDE_FINISH_BLOCKS = 256;
__global__ void __launch_bounds__(256) slide_finish_kernel(int M, int T, int K, int n_cells, const uint32_t* __restrict__ elig,
                                                            const int32_t* __restrict__ best_target,
                                                            const unsigned long long* __restrict__ claim_key,
                                                            const int32_t* __restrict__ cell_start, uint8_t* __restrict__ tp,
                                                            int32_t* __restrict__ claim, int32_t* __restrict__ stats) {
    __shared__ int red[4];
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
        const int e = block_sum_256(n_elig, red), c = block_sum_256(n_claimed, red);   // (k and K are uniform over the workgroup)
        if (threadIdx.x == 0) {
            if (e) atomicAdd(&stats[2 * k], e);
            if (c) atomicAdd(&stats[2 * k + 1], c);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) stats[2 * K + 1] = cell_start[n_cells + 1] - cell_start[n_cells];
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
    WsCarver cv(ws);
    const size_t m = (size_t)(n_rows > 0 ? n_rows : 1), t = (size_t)(n_targets > 0 ? n_targets : 1), cells = grid_cell_cap(n_targets);
    const size_t k = (size_t)(n_thres > 0 ? n_thres : 1);
    w.partials = cv.take<float>(GRID_STATS_BLOCKS * GRID_STATS_WORDS);
    w.class_flags = cv.take<int32_t>(AY_SLIDE_MAX_CLASSES);
    w.claim_key = cv.take<unsigned long long>(k * t);
    w.box = cv.take<float4>(t);
    w.orig = cv.take<int32_t>(t);
    w.cell_of = cv.take<int32_t>(t);
    w.elig = cv.take<uint32_t>(m);
    w.cell_start = cv.take<int32_t>(cells + 2);
    w.cursor = cv.take<int32_t>(cells + 2);
    w.bytes = cv.bytes();
    return w;
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
    AY_CHECK_HIP(hipMemsetAsync(stats, 0, sizeof(int32_t) * (2 * K + 2), st), "ay_slide_match: memset");
    AY_CHECK_HIP(hipMemsetAsync(w.class_flags, 0, sizeof(int32_t) * AY_SLIDE_MAX_CLASSES, st), "ay_slide_match: memset");
    BoxGrid g = {0.0f, 0.0f, 8.0f, 1, 1};
    if (T > 0) {
        const unsigned tblocks = (unsigned)(((long long)T + 255) / 256);
        AY_CHECK_HIP(hipMemsetAsync(w.claim_key, 0xFF, sizeof(unsigned long long) * (size_t)K * T, st), "ay_slide_match: memset");
        // 1. geometry reduction over the targets -> cell side and grid (host)
        const SlideTargets items = {targets, r};
        hipLaunchKernelGGL(grid_stats_kernel<SlideTargets>, dim3(GRID_STATS_BLOCKS), dim3(256), 0, st, items, T, w.partials);
        AY_CHECK_LAUNCH("grid_stats_kernel");
        float partials[GRID_STATS_BLOCKS * GRID_STATS_WORDS];
        AY_CHECK_HIP(hipMemcpyAsync(partials, w.partials, sizeof(partials), hipMemcpyDeviceToHost, st), "ay_slide_match: copy");
        AY_CHECK_HIP(hipStreamSynchronize(st), "ay_slide_match: sync");
        g = grid_choose(partials, T, /* ignored targets are on no list */ false, grid_cell_cap(T), cell_side);
        const int n_cells = g.n_cells();
        // 2. counting sort of the non-ignored targets by cell (the oversize list is cell n_cells)
        AY_CHECK_HIP(hipMemsetAsync(w.cell_start, 0, sizeof(int32_t) * (n_cells + 2), st), "ay_slide_match: memset");
        AY_CHECK_HIP(hipMemsetAsync(w.cursor, 0, sizeof(int32_t) * (n_cells + 2), st), "ay_slide_match: memset");
        hipLaunchKernelGGL(slide_bin_count_kernel, dim3(tblocks), dim3(256), 0, st, targets, T, r, g, target_ignored, w.cell_of, w.cell_start,
                           w.class_flags, stats + 2 * K);
        AY_CHECK_LAUNCH("slide_bin_count_kernel");
        hipLaunchKernelGGL(grid_scan_kernel, dim3(1), dim3(1024), 0, st, w.cell_start, n_cells + 1);
        AY_CHECK_LAUNCH("grid_scan_kernel");
        hipLaunchKernelGGL(slide_scatter_kernel, dim3(tblocks), dim3(256), 0, st, targets, T, (const int32_t*)w.cell_of,
                           (const int32_t*)w.cell_start, w.cursor, w.box, w.orig);
        AY_CHECK_LAUNCH("slide_scatter_kernel");
    } else {
        AY_CHECK_HIP(hipMemsetAsync(w.cell_start, 0, sizeof(int32_t) * 3, st), "ay_slide_match: memset");
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
        hipLaunchKernelGGL(slide_finish_kernel, dim3((unsigned)(fblocks < SLIDE_FINISH_BLOCKS ? fblocks : SLIDE_FINISH_BLOCKS)), dim3(256), 0, st, M, T, K, g.n_cells(),
                           (const uint32_t*)w.elig, (const int32_t*)best_target, (const unsigned long long*)w.claim_key,
                           (const int32_t*)w.cell_start, tp, claim, stats);
        AY_CHECK_LAUNCH("slide_finish_kernel");
    }
    return AY_OK;
}
