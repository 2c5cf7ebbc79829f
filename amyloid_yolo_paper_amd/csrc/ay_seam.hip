// Slide-level seam merge for whole-slide detection with OVERLAPPING tiles (wsi.detect_region(overlap > 0)).
//
// An object that lies in the overlap band of two (or, at a grid corner, four) tiles is reported by each of them, often as a
// truncated box by the tile that sees only a part of it.  This file keeps the per-tile detections on the device (ay_seam_append)
// and removes the second sightings once per slide (ay_seam_merge).
//
// THE RULE (the specification; tests/seam_reference.py restates it on the CPU).  Input: rows [M][7] fp32
// (x1, y1, x2, y2, conf, cls_conf, cls_pred) in slide pixels and tile_id [M] int32.  Output: a keep flag per row and the number of
// rows kept.  Rows are never altered: the result is a subset of the input, bit for bit.
//   * score_i = conf_i * cls_conf_i, one fp32 multiply (the NMS score of utils/utils.py non_max_suppression).
//   * rank: i comes before j iff score_i > score_j, or the scores are equal and i < j.
//   * ov(i, j) = inter / min(area_i, area_j) in fp32 with the +1 pixel convention of bbox_iou(x1y1x2y2=True):
//     iw = min(x2_i, x2_j) - max(x1_i, x1_j) + 1, likewise ih, both clamped at 0, inter = iw * ih,
//     area = (x2 - x1 + 1) * (y2 - y1 + 1); no fused multiply-add (the library is built with -ffp-contract=off).  Intersection
//     over the SMALLER box, not IoU: a box cut in half by a tile edge has IoU of about 0.5 with the whole one but ov near 1.
//   * Walk the rows in rank order.  Row i is dropped iff some row j that ranks before it AND WAS KEPT has the same cls_pred, a
//     different tile_id and ov(i, j) > seam_thres.  Otherwise it is kept.  Exact greedy suppression: a row whose only stronger
//     partner was itself dropped is kept.  Rows of one tile never suppress each other (the per-tile merge-NMS has seen them).
//
// HOW.  The work is local (a box only meets boxes near it), so the rows are binned by ay_box_grid.h (the grid cell of a row's
// centre, a cell side c chosen from the data) and a row searches the 3x3 cells around its own.  A row is REGULAR iff w + 1 <= c
// and h + 1 <= c (w = x2 - x1 + 1, likewise h) and x1, y1 are finite: two regular rows that share a pixel have centres less than
// c - 1 apart, hence lie in neighbouring cells.  All other rows (larger than a cell, or not finite) form the OVERSIZE list, the
// last segment of the sorted array: a regular row tests it in full, an oversize row tests every row.  The result therefore equals
// the rule for every input, whatever the box sizes and whatever the cell side.
// The greedy order is resolved in parallel over three states undecided / kept / dropped: a row is dropped as soon as one of its
// potential suppressors (earlier rank, same class, other tile, ov > thres) is kept, kept once all of them are dropped (or there
// are none).  The undecided row of best rank can always be decided, so every round makes progress and the loop ends after at
// most M rounds; the number of rounds is the longest dependency chain and is NOT capped.  A row's final state is a function of
// the input alone (the unique fixed point of the rule), so nothing in the result depends on the order in which threads run,
// on the order of the rows inside a cell (the scatter's cursor is an integer atomic) or on how many rounds a launch resolves.
#include "ay_box_grid.h"

namespace ay {

enum { SEAM_UNDECIDED = 0, SEAM_KEPT = 1, SEAM_DROPPED = 2 };
constexpr int SEAM_TRIES = 4;            // attempts of an undecided row inside one round launch
constexpr int SEAM_ROUNDS_PER_SYNC = 8;  // round launches between two reads of the "rows undecided" counter

// ---- append ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int seam_clamp_count(int c, int max_det) { return c < 0 ? 0 : (c > max_det ? max_det : c); }

// one workgroup per image: the image's slot range starts at slide_count[0] + the ordered prefix over the (clamped) counts of the
// images before it, so rows land in tile order and, within a tile, in NMS output order
__global__ void __launch_bounds__(256) seam_append_kernel(const float* __restrict__ rows, const int32_t* __restrict__ count, int max_det,
                                                           float scale, const float* __restrict__ origins_xy,
                                                           const int32_t* __restrict__ tile_ids, float* __restrict__ slide_rows,
                                                           int32_t* __restrict__ slide_tile, const int32_t* __restrict__ slide_count,
                                                           int capacity) {
    __shared__ int red[4];
    const int b = blockIdx.x;
    int part = 0;
    for (int k = threadIdx.x; k < b; k += 256) part += seam_clamp_count(count[k], max_det);
    const long long base = (long long)slide_count[0] + block_sum_256(part, red);
    const int n = seam_clamp_count(count[b], max_det);
    const float ox = origins_xy[2 * b], oy = origins_xy[2 * b + 1];
    const int32_t id = tile_ids[b];
    for (int r = threadIdx.x; r < n; r += 256) {
        const long long dst = base + r;
        if (dst >= capacity) break;   // reported by seam_append_commit_kernel
        const float* s = rows + ((size_t)b * max_det + r) * 7;
        float* d = slide_rows + (size_t)dst * 7;
        d[0] = s[0] * scale + ox;     // fl32(fl32(v * scale) + origin): two roundings, as on the host path
        d[1] = s[1] * scale + oy;
        d[2] = s[2] * scale + ox;
        d[3] = s[3] * scale + oy;
        d[4] = s[4];
        d[5] = s[5];
        d[6] = s[6];
        slide_tile[dst] = id;
    }
}

// behind the append on the same stream: slide_count[0] += rows appended, slide_count[1] |= AY_SEAM_FLAG_*
__global__ void __launch_bounds__(256) seam_append_commit_kernel(const int32_t* __restrict__ count, int batch, int max_det,
                                                                  int32_t* __restrict__ slide_count, int capacity) {
    __shared__ int red[4];
    int part = 0, over = 0;
    for (int k = threadIdx.x; k < batch; k += 256) {
        part += seam_clamp_count(count[k], max_det);
        over += count[k] > max_det;
    }
    const int total = block_sum_256(part, red);
    const int any_over = block_sum_256(over, red);
    if (threadIdx.x == 0) {
        const long long want = (long long)slide_count[0] + total;
        int flags = slide_count[1];
        if (any_over) flags |= AY_SEAM_FLAG_MAX_DET;
        if (want > capacity) flags |= AY_SEAM_FLAG_CAPACITY;
        slide_count[0] = (int32_t)(want > capacity ? capacity : want);
        slide_count[1] = flags;
    }
}

// ---- merge -------------------------------------------------------------------------------------------------------------------
// the rows as the centre grid sees them (ay_box_grid.h): all of them, sides with the +1 pixel convention
struct SeamRows {
    const float* __restrict__ rows;
    __device__ __forceinline__ float4 box(int i) const {
        const float* r = rows + (size_t)i * 7;
        return make_float4(r[0], r[1], r[2], r[3]);
    }
    __device__ __forceinline__ bool live(const float4) const { return true; }
    static __device__ __forceinline__ float extent(float lo, float hi) { return hi - lo + 1.0f; }
    static __device__ __forceinline__ float side(float w, float h) { return fmaxf(fmaxf(w, h), 0.0f) + 1.0f; }
    static __device__ __forceinline__ bool regular(const float4 b, float c) {
        const float w = b.z - b.x + 1.0f, h = b.w - b.y + 1.0f;
        return w + 1.0f <= c && h + 1.0f <= c && finite_f(b.x) && finite_f(b.y);
    }
};

__global__ void __launch_bounds__(256) seam_bin_count_kernel(SeamRows items, int M, BoxGrid g, int32_t* __restrict__ cell_of,
                                                              int32_t* __restrict__ cell_start) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    grid_count(i, grid_cell<SeamRows>(items.box(i), g), cell_of, cell_start);
}

// sorted records: box (x1, y1, x2, y2) and meta (score bits, cls bits, tile id, original row)
__global__ void __launch_bounds__(256) seam_scatter_kernel(const float* __restrict__ rows, const int32_t* __restrict__ tile_id, int M,
                                                            const int32_t* __restrict__ cell_of, const int32_t* __restrict__ cell_start,
                                                            int32_t* __restrict__ cursor, float4* __restrict__ box, int4* __restrict__ meta,
                                                            int32_t* __restrict__ sorted_cell, int32_t* __restrict__ state) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const int c = cell_of[i];
    const int p = grid_slot(c, cell_start, cursor);
    const float* r = rows + (size_t)i * 7;
    box[p] = make_float4(r[0], r[1], r[2], r[3]);
    const float score = r[4] * r[5];
    meta[p] = make_int4(__float_as_int(score), __float_as_int(r[6]), tile_id[i], i);
    sorted_cell[p] = c;
    state[p] = SEAM_UNDECIDED;
}

__device__ __forceinline__ int seam_load_state(const int32_t* s) { return __hip_atomic_load(s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// is row q (box bq, meta mq) a potential suppressor of row p?
__device__ __forceinline__ bool seam_suppresses(const float4 bq, const int4 mq, const float4 bp, const int4 mp, float area_p, float thres) {
    const float sq = __int_as_float(mq.x), sp = __int_as_float(mp.x);
    if (!(sq > sp || (sq == sp && mq.w < mp.w))) return false;                      // rank
    if (!(__int_as_float(mq.y) == __int_as_float(mp.y)) || mq.z == mp.z) return false;  // same class, other tile
    const float iw = fminf(bq.z, bp.z) - fmaxf(bq.x, bp.x) + 1.0f;
    const float ih = fminf(bq.w, bp.w) - fmaxf(bq.y, bp.y) + 1.0f;
    const float inter = fmaxf(iw, 0.0f) * fmaxf(ih, 0.0f);
    const float area_q = (bq.z - bq.x + 1.0f) * (bq.w - bq.y + 1.0f);
    return inter / fminf(area_p, area_q) > thres;
}

// 0 = a potential suppressor is kept (drop), 1 = all potential suppressors in [lo, hi) are dropped, 2 = one is undecided
__device__ __forceinline__ int seam_scan_range(int lo, int hi, int p, const float4 bp, const int4 mp, float area_p, float thres,
                                                const float4* __restrict__ box, const int4* __restrict__ meta, const int32_t* state) {
    int res = 1;
    for (int q = lo; q < hi; ++q) {
        if (q == p) continue;
        if (!seam_suppresses(box[q], meta[q], bp, mp, area_p, thres)) continue;
        const int s = seam_load_state(state + q);
        if (s == SEAM_KEPT) return 0;
        if (s == SEAM_UNDECIDED) res = 2;
    }
    return res;
}

// one round: every undecided row (thread p = its position in the cell-sorted order) looks its potential suppressors up again
__global__ void __launch_bounds__(256) seam_round_kernel(int M, BoxGrid g, float thres, const float4* __restrict__ box,
                                                          const int4* __restrict__ meta, const int32_t* __restrict__ sorted_cell,
                                                          const int32_t* __restrict__ cell_start, int32_t* state,
                                                          int32_t* __restrict__ undecided /* nullable */) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    bool open = false;
    if (p < M && seam_load_state(state + p) == SEAM_UNDECIDED) {
        open = true;
        const float4 bp = box[p];
        const int4 mp = meta[p];
        const float area_p = (bp.z - bp.x + 1.0f) * (bp.w - bp.y + 1.0f);
        const int n_cells = g.n_cells(), c = sorted_cell[p];
        const int over_lo = cell_start[n_cells];
        for (int t = 0; t < SEAM_TRIES && open; ++t) {
            int res = 1;
            if (c == n_cells) {   // oversize: everything
                res = seam_scan_range(0, M, p, bp, mp, area_p, thres, box, meta, state);
            } else {
                const int ix = c % g.gx, iy = c / g.gx;
                const int xa = max(ix - 1, 0), xb = min(ix + 1, g.gx - 1);
                for (int y = max(iy - 1, 0); y <= min(iy + 1, g.gy - 1) && res; ++y) {   // the three cells of a grid row are one range
                    const int r = seam_scan_range(cell_start[y * g.gx + xa], cell_start[y * g.gx + xb + 1], p, bp, mp, area_p, thres, box,
                                                  meta, state);
                    res = r == 0 ? 0 : max(res, r);
                }
                if (res) {
                    const int r = seam_scan_range(over_lo, M, p, bp, mp, area_p, thres, box, meta, state);
                    res = r == 0 ? 0 : max(res, r);
                }
            }
            if (res != 2) {
                __hip_atomic_store(state + p, res == 0 ? SEAM_DROPPED : SEAM_KEPT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                open = false;
            }
        }
    }
    if (undecided) {   // one atomic per wavefront
        const unsigned long long m = __ballot(open);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(undecided, __popcll(m));
    }
}

__global__ void __launch_bounds__(256) seam_finish_kernel(int M, const int4* __restrict__ meta, const int32_t* __restrict__ state,
                                                           uint8_t* __restrict__ keep, int32_t* __restrict__ stats) {
    __shared__ int red[4];
    const int p = blockIdx.x * 256 + threadIdx.x;
    int k = 0;
    if (p < M) {
        k = state[p] == SEAM_KEPT;
        keep[meta[p].w] = (uint8_t)k;
    }
    const int total = block_sum_256(k, red);
    if (threadIdx.x == 0 && total) atomicAdd(&stats[0], total);   // one atomic per workgroup
}

__global__ void seam_set_rounds_kernel(int32_t* stats, int rounds) { stats[1] = rounds; }

struct SeamWs {
    int32_t* undecided;
    float* partials;
    int32_t *cell_of, *sorted_cell, *state, *cell_start, *cursor;
    float4* box;
    int4* meta;
    size_t bytes;
};

static SeamWs seam_carve(void* ws, int n_rows) {
    SeamWs w;
    WsCarver cv(ws);
    const size_t n = (size_t)(n_rows > 0 ? n_rows : 1), cells = grid_cell_cap(n_rows);
    w.undecided = cv.take<int32_t>(1);
    w.partials = cv.take<float>(GRID_STATS_BLOCKS * GRID_STATS_WORDS);
    w.box = cv.take<float4>(n);
    w.meta = cv.take<int4>(n);
    w.cell_of = cv.take<int32_t>(n);
    w.sorted_cell = cv.take<int32_t>(n);
    w.state = cv.take<int32_t>(n);
    w.cell_start = cv.take<int32_t>(cells + 2);
    w.cursor = cv.take<int32_t>(cells + 2);
    w.bytes = cv.bytes();
    return w;
}

}  // namespace ay

extern "C" int ay_seam_append(const float* rows, const int32_t* count, int batch, int max_det, float scale, const float* origins_xy,
                              const int32_t* tile_ids, float* slide_rows, int32_t* slide_tile, int32_t* slide_count, int capacity,
                              ay_stream_t stream) {
    using namespace ay;
    AY_CHECK_ARG(rows && count && origins_xy && tile_ids && slide_rows && slide_tile && slide_count, "ay_seam_append: null");
    AY_CHECK_ARG(batch > 0 && max_det > 0 && capacity > 0, "ay_seam_append: batch %d max_det %d capacity %d", batch, max_det, capacity);
    hipLaunchKernelGGL(seam_append_kernel, dim3(batch), dim3(256), 0, S(stream), rows, count, max_det, scale, origins_xy, tile_ids,
                       slide_rows, slide_tile, (const int32_t*)slide_count, capacity);
    AY_CHECK_LAUNCH("seam_append_kernel");
    hipLaunchKernelGGL(seam_append_commit_kernel, dim3(1), dim3(256), 0, S(stream), count, batch, max_det, slide_count, capacity);
    AY_CHECK_LAUNCH("seam_append_commit_kernel");
    return AY_OK;
}

extern "C" size_t ay_seam_merge_workspace_bytes(int n_rows) { return ay::seam_carve(nullptr, n_rows).bytes; }

extern "C" int ay_seam_merge(const float* slide_rows, const int32_t* slide_tile, int n_rows, float seam_thres, uint8_t* keep, int32_t* stats,
                             void* workspace, size_t workspace_bytes, ay_stream_t stream) {
    using namespace ay;
    AY_CHECK_ARG(n_rows >= 0 && n_rows <= (1 << 28), "ay_seam_merge: n_rows %d", n_rows);
    AY_CHECK_ARG(stats, "ay_seam_merge: null stats");
    hipStream_t st = S(stream);
    AY_CHECK_HIP(hipMemsetAsync(stats, 0, 2 * sizeof(int32_t), st), "ay_seam_merge: memset");
    if (n_rows == 0) return AY_OK;
    AY_CHECK_ARG(slide_rows && slide_tile && keep && workspace, "ay_seam_merge: null");
    const SeamWs w = seam_carve(workspace, n_rows);
    AY_CHECK_ARG(workspace_bytes >= w.bytes, "ay_seam_merge: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
    AY_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "ay_seam_merge: workspace not 16-byte aligned");
    const int M = n_rows;
    const unsigned blocks = (unsigned)((M + 255) / 256);

    // 1. geometry reduction -> cell side and grid (host)
    const SeamRows items = {slide_rows};
    hipLaunchKernelGGL(grid_stats_kernel<SeamRows>, dim3(GRID_STATS_BLOCKS), dim3(256), 0, st, items, M, w.partials);
    AY_CHECK_LAUNCH("grid_stats_kernel");
    float partials[GRID_STATS_BLOCKS * GRID_STATS_WORDS];
    AY_CHECK_HIP(hipMemcpyAsync(partials, w.partials, sizeof(partials), hipMemcpyDeviceToHost, st), "ay_seam_merge: copy");
    AY_CHECK_HIP(hipStreamSynchronize(st), "ay_seam_merge: sync");
    const BoxGrid g = grid_choose(partials, M, /* rows that are not finite are oversize whatever the cell */ true, grid_cell_cap(M), 0.0f);
    const int n_cells = g.n_cells();

    // 2. counting sort by cell (the oversize list is cell n_cells)
    AY_CHECK_HIP(hipMemsetAsync(w.cell_start, 0, sizeof(int32_t) * (n_cells + 2), st), "ay_seam_merge: memset");
    AY_CHECK_HIP(hipMemsetAsync(w.cursor, 0, sizeof(int32_t) * (n_cells + 2), st), "ay_seam_merge: memset");
    hipLaunchKernelGGL(seam_bin_count_kernel, dim3(blocks), dim3(256), 0, st, items, M, g, w.cell_of, w.cell_start);
    AY_CHECK_LAUNCH("seam_bin_count_kernel");
    hipLaunchKernelGGL(grid_scan_kernel, dim3(1), dim3(1024), 0, st, w.cell_start, n_cells + 1);
    AY_CHECK_LAUNCH("grid_scan_kernel");
    hipLaunchKernelGGL(seam_scatter_kernel, dim3(blocks), dim3(256), 0, st, slide_rows, slide_tile, M, (const int32_t*)w.cell_of,
                       (const int32_t*)w.cell_start, w.cursor, w.box, w.meta, w.sorted_cell, w.state);
    AY_CHECK_LAUNCH("seam_scatter_kernel");

    // 3. rounds until no row is undecided (no cap: the longest dependency chain decides)
    int rounds = 0;
    for (;;) {
        AY_CHECK_HIP(hipMemsetAsync(w.undecided, 0, sizeof(int32_t), st), "ay_seam_merge: memset");
        for (int r = 0; r < SEAM_ROUNDS_PER_SYNC; ++r, ++rounds) {
            hipLaunchKernelGGL(seam_round_kernel, dim3(blocks), dim3(256), 0, st, M, g, seam_thres, (const float4*)w.box,
                               (const int4*)w.meta, (const int32_t*)w.sorted_cell, (const int32_t*)w.cell_start, w.state,
                               r == SEAM_ROUNDS_PER_SYNC - 1 ? w.undecided : (int32_t*)nullptr);
            AY_CHECK_LAUNCH("seam_round_kernel");
        }
        int32_t left = 0;
        AY_CHECK_HIP(hipMemcpyAsync(&left, w.undecided, sizeof(left), hipMemcpyDeviceToHost, st), "ay_seam_merge: copy");
        AY_CHECK_HIP(hipStreamSynchronize(st), "ay_seam_merge: sync");
        if (left == 0) break;
    }

    // 4. keep flags in input order, number kept
    hipLaunchKernelGGL(seam_finish_kernel, dim3(blocks), dim3(256), 0, st, M, (const int4*)w.meta, (const int32_t*)w.state, keep, stats);
    AY_CHECK_LAUNCH("seam_finish_kernel");
    hipLaunchKernelGGL(seam_set_rounds_kernel, dim3(1), dim3(1), 0, st, stats, rounds);
    AY_CHECK_LAUNCH("seam_set_rounds_kernel");
    return AY_OK;
}
