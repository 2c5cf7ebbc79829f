// Slide-level burden (wsi.burden_map, wsi.densest_fields, wsi.quantify_region): the detections of a whole slide turned into class
// count maps on a grid of `cell`-pixel cells, and the densest microscope-sized fields of every class.
//
// THE BURDEN RULE and THE FIELD RULE are stated in include/amyloid_yolo.h; tests/burden_reference.py restates them on the CPU (plain
// loops over cells, the selection as the sequential loop of the rule).
//
// HOW.
//   ay_burden_bin: a zeroing kernel, then one lane per row: two fp32 operations for the centre, the flags, an integer cell; the lanes
//     of a wavefront that share a counter are merged and add once (integer atomicAdd into counts: order-free, the same bytes every
//     run).  The statistics go through LDS adds to one global atomic per workgroup and word.
//   ay_field_select: the F x F field sums of the C count planes and the tissue plane in separable form -- a row pass of F into the
//     workspace, a column pass of F behind it, the tissue plane first so that the class planes can write 0 for every field that is
//     not eligible -- and then one workgroup per class that loops the K rounds of the rule: every thread walks its share of the
//     fields (eight loads in flight), skips what cannot beat its own best so far, tests the rest against the picks of the earlier
//     rounds (at most 64 pairs in LDS) and keeps the maximum of the 64-bit key (n << 32) | (0xffffffff - index), which is the largest
//     count with ties to the lowest index; a wave shuffle and one LDS step make it the workgroup's.
// Kernel launches only: no memset node, no allocation, no host read.
#include "ay_box_grid.h"   // WsCarver

namespace ay {

constexpr int BURDEN_THREADS = 256;
constexpr int BURDEN_SELECT_THREADS = 1024;
constexpr int BURDEN_SELECT_LOADS = 8;
constexpr int BURDEN_STAT_WORDS = AY_BURDEN_MAX_CLASSES + 3;
constexpr int BURDEN_MAX_FIELD = 46340;   // field * cell <= 46340 (THE TISSUE RULE's bound), cell >= 1

__global__ void __launch_bounds__(BURDEN_THREADS) burden_zero_kernel(int32_t* __restrict__ counts, long long n, int32_t* __restrict__ stats, int n_stats) {
    const long long stride = (long long)gridDim.x * BURDEN_THREADS;
    for (long long i = (long long)blockIdx.x * BURDEN_THREADS + threadIdx.x; i < n; i += stride) counts[i] = 0;
    if (blockIdx.x == 0 && (int)threadIdx.x < n_stats) stats[threadIdx.x] = 0;
}

__device__ __forceinline__ bool burden_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }   // false for NaN and +-inf

// pixel of a finite centre coordinate: clamped into the slide; the last step is on integers ((float)(n - 1) rounds up for some n
// above 2^24)
__device__ __forceinline__ int burden_pixel(float c, int n) { return min((int)floorf(fminf(fmaxf(c, 0.0f), (float)(n - 1))), n - 1); }

__global__ void __launch_bounds__(BURDEN_THREADS) burden_bin_kernel(const float* __restrict__ rows, int M, int C, int H, int W, int cell, int gx,
                                                                     size_t plane, float min_conf, int32_t* __restrict__ counts,
                                                                     int32_t* __restrict__ stats) {
    __shared__ int sh[BURDEN_STAT_WORDS];   // counted per class, below, flagged, flag bits
    for (int k = threadIdx.x; k < C + 3; k += BURDEN_THREADS) sh[k] = 0;
    __syncthreads();
    const long long i = (long long)blockIdx.x * BURDEN_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int key = -1, c = -1;   // key: the row's counter, class-major (below 2^30)
    if (i < M) {
        const float* r = rows + (size_t)i * 7;
        const float x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3], conf = r[4], label = r[6];
        const float cx = (x1 + x2) * 0.5f, cy = (y1 + y2) * 0.5f;
        int flags = 0;
        if (!(burden_finite(cx) && burden_finite(cy))) flags |= AY_BURDEN_FLAG_NONFINITE;
        if (label >= 0.0f && label < (float)C) {
            c = (int)label;
            if ((float)c != label) c = -1;
        }
        if (c < 0) flags |= AY_BURDEN_FLAG_CLASS;
        if (flags) {
            atomicAdd(&sh[C + 1], 1);
            atomicOr(&sh[C + 2], flags);
        } else if (!(conf >= min_conf)) {
            atomicAdd(&sh[C], 1);
        } else {
            const int ix = burden_pixel(cx, W) / cell, iy = burden_pixel(cy, H) / cell;
            key = (int)((size_t)c * plane + (size_t)iy * gx + ix);
        }
    }
    // the lanes of a wavefront that share a counter add once, through the first of them: rows arrive in tile order and a dense
    // slide puts thousands of them into a few cells, which one atomic per row would queue on a few words (profiles/burden.txt).
    // Every lane of the wavefront is here (nobody has returned); the loop runs once per distinct counter of the wavefront.
    bool pending = key >= 0;
    for (unsigned long long todo = __ballot(pending); todo; todo = __ballot(pending)) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lk = __shfl(key, leader);
        const bool same = pending && key == lk;
        const int n = __popcll(__ballot(same));
        if (same) {
            pending = false;
            if (lane == leader) {
                atomicAdd(&counts[lk], n);
                atomicAdd(&sh[c], n);
            }
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < C + 3; k += BURDEN_THREADS) {
        const int v = sh[k];
        if (v) {
            if (k == C + 2) atomicOr(&stats[k], v);
            else atomicAdd(&stats[k], v);
        }
    }
}

// plane p of the C + 1 planes: a class's counts, or the tissue
__device__ __forceinline__ const int32_t* burden_plane(const int32_t* __restrict__ counts, const int32_t* __restrict__ tissue, int C, int p, size_t cells) {
    return p < C ? counts + (size_t)p * cells : tissue;
}

// row pass: rowsum[p][y][fx] = sum over dx < F of plane[p][y][fx + dx]; blockIdx.y = p (the tissue plane is not launched without tissue)
__global__ void __launch_bounds__(BURDEN_THREADS) burden_row_pass_kernel(const int32_t* __restrict__ counts, const int32_t* __restrict__ tissue, int C,
                                                                          int gy, int gx, int nx, int F, int32_t* __restrict__ rowsum) {
    const int p = blockIdx.y;
    const int32_t* src = burden_plane(counts, tissue, C, p, (size_t)gy * gx);
    int32_t* dst = rowsum + (size_t)p * gy * nx;
    const long long n = (long long)gy * nx, stride = (long long)gridDim.x * BURDEN_THREADS;
    for (long long i = (long long)blockIdx.x * BURDEN_THREADS + threadIdx.x; i < n; i += stride) {
        const int y = (int)(i / nx), fx = (int)(i - (long long)y * nx);
        const int32_t* s = src + (size_t)y * gx + fx;
        int sum = 0;
        for (int d = 0; d < F; ++d) sum += s[d];
        dst[i] = sum;
    }
}

// column pass: fieldsum[p][fy][fx] = sum over dy < F of rowsum[p][fy + dy][fx], p = p0 + blockIdx.y.  With `elig` (the finished field
// sums of the tissue plane; the class planes are launched behind it) the count of a field that is not ELIGIBLE is written as 0: no
// round can take it, and the selection needs no second load per field.
__global__ void __launch_bounds__(BURDEN_THREADS) burden_col_pass_kernel(const int32_t* __restrict__ rowsum, int p0, int gy, int ny, int nx, int F,
                                                                          const int32_t* __restrict__ elig, int need,
                                                                          int32_t* __restrict__ fieldsum) {
    const int p = p0 + blockIdx.y;
    const int32_t* src = rowsum + (size_t)p * gy * nx;
    int32_t* dst = fieldsum + (size_t)p * ny * nx;
    const long long n = (long long)ny * nx, stride = (long long)gridDim.x * BURDEN_THREADS;
    for (long long i = (long long)blockIdx.x * BURDEN_THREADS + threadIdx.x; i < n; i += stride) {
        const int32_t* s = src + i;   // (fy, fx) of the row sums; one row further is nx further
        int sum = 0;
        for (int d = 0; d < F; ++d) sum += s[(size_t)d * nx];
        if (elig && elig[i] < need) sum = 0;
        dst[i] = sum;
    }
}

// one workgroup per class: fills the class's rows of `fields` with -1 and runs the K rounds of THE FIELD RULE over the field sums
// (those of the fields that are not eligible are 0 already)
__global__ void __launch_bounds__(BURDEN_SELECT_THREADS) burden_select_kernel(const int32_t* __restrict__ fieldsum, int C, int ny, int nx, int F,
                                                                              int has_tissue, int K, int32_t* __restrict__ fields,
                                                                              int32_t* __restrict__ n_found) {
    __shared__ int pick_y[AY_BURDEN_MAX_FIELDS], pick_x[AY_BURDEN_MAX_FIELDS];
    __shared__ unsigned long long wave_best[BURDEN_SELECT_THREADS / 64];
    const int c = blockIdx.x, tid = threadIdx.x;
    const unsigned nf = (unsigned)ny * (unsigned)nx;   // 0 when the grid holds no field; at most 2^30: every index below fits 32 bits
    const int32_t* nsum = fieldsum + (size_t)c * nf;
    const int32_t* tsum = fieldsum + (size_t)C * nf;
    int32_t* out = fields + (size_t)c * K * 4;
    for (int k = tid; k < K * 4; k += BURDEN_SELECT_THREADS) out[k] = -1;
    int found = 0;
    for (int round = 0; round < K && nf > 0u; ++round) {
        unsigned long long key = 0;   // a count of 0 never wins: the round's stop condition
        // BURDEN_SELECT_LOADS independent loads in flight per thread: the walk is bound by the latency of its loads, not by their bytes
        for (unsigned base = tid; base < nf; base += BURDEN_SELECT_THREADS * BURDEN_SELECT_LOADS) {
            int n[BURDEN_SELECT_LOADS];
#pragma unroll
            for (int u = 0; u < BURDEN_SELECT_LOADS; ++u) {
                const unsigned idx = base + u * BURDEN_SELECT_THREADS;
                n[u] = idx < nf ? nsum[idx] : 0;
            }
#pragma unroll
            for (int u = 0; u < BURDEN_SELECT_LOADS; ++u) {
                const unsigned idx = base + u * BURDEN_SELECT_THREADS;
                if (n[u] <= 0) continue;   // (a field that is not eligible holds 0)
                const unsigned long long cand = ((unsigned long long)(unsigned)n[u] << 32) | (0xffffffffu - idx);
                if (cand <= key) continue;
                const int fy = (int)(idx / (unsigned)nx), fx = (int)(idx - (unsigned)fy * (unsigned)nx);
                bool open = true;
                for (int j = 0; j < round; ++j) open = open && !(abs(fy - pick_y[j]) < F && abs(fx - pick_x[j]) < F);
                if (open) key = cand;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(key, o, 64);
            key = other > key ? other : key;
        }
        if ((tid & 63) == 0) wave_best[tid >> 6] = key;
        __syncthreads();
        unsigned long long best = 0;
#pragma unroll
        for (int w = 0; w < BURDEN_SELECT_THREADS / 64; ++w) best = wave_best[w] > best ? wave_best[w] : best;
        if ((best >> 32) == 0) break;   // workgroup-uniform: every thread read the same words
        if (tid == 0) {
            const unsigned idx = 0xffffffffu - (unsigned)best;
            const int fy = (int)(idx / (unsigned)nx), fx = (int)(idx - (unsigned)fy * (unsigned)nx);
            pick_y[round] = fy, pick_x[round] = fx;
            out[round * 4 + 0] = fy, out[round * 4 + 1] = fx, out[round * 4 + 2] = (int)(best >> 32);
            out[round * 4 + 3] = has_tissue ? tsum[idx] : 0;
        }
        ++found;
        __syncthreads();   // the pick is visible; wave_best may be written again
    }
    if (tid == 0) n_found[c] = found;
}

struct BurdenWs {
    int32_t *rowsum, *fieldsum;
    size_t bytes;
};

// (gy, gx, field already checked) -> the two arrays of the separable sums; no field: both empty
static BurdenWs burden_carve(void* ws, int C, int gy, int gx, int F) {
    BurdenWs w;
    const size_t ny = gy >= F ? (size_t)(gy - F + 1) : 0, nx = gx >= F ? (size_t)(gx - F + 1) : 0;
    const size_t planes = (size_t)C + 1;
    WsCarver cv(ws);
    w.rowsum = cv.take<int32_t>(planes * (ny ? (size_t)gy * nx : 0));
    w.fieldsum = cv.take<int32_t>(planes * ny * nx);
    w.bytes = cv.bytes();
    return w;
}

static inline bool burden_select_dims_ok(int C, int gy, int gx, int F) {
    return C >= 1 && C <= AY_BURDEN_MAX_CLASSES && gy >= 1 && gx >= 1 && (long long)gy * gx <= (1ll << 30) && F >= 1 && F <= BURDEN_MAX_FIELD;
}

static inline unsigned burden_blocks(long long n) {
    const long long b = (n + BURDEN_THREADS - 1) / BURDEN_THREADS;
    return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

}  // namespace ay

extern "C" int ay_burden_bin(const float* rows, int n_rows, int num_classes, int slide_h, int slide_w, int cell, float min_conf,
                             int32_t* counts, int32_t* stats, ay_stream_t stream) {
    using namespace ay;
    const int M = n_rows, C = num_classes;
    AY_CHECK_ARG(M >= 0 && (M == 0 || rows), "ay_burden_bin: n_rows %d%s", M, rows ? "" : " with null rows");
    AY_CHECK_ARG(C >= 1 && C <= AY_BURDEN_MAX_CLASSES, "ay_burden_bin: num_classes %d outside 1 .. %d", C, AY_BURDEN_MAX_CLASSES);
    AY_CHECK_ARG(cell >= 1, "ay_burden_bin: cell %d < 1", cell);
    AY_CHECK_ARG(slide_h >= 1 && slide_w >= 1, "ay_burden_bin: slide %d x %d", slide_h, slide_w);
    AY_CHECK_ARG(counts && stats, "ay_burden_bin: null counts or stats");
    const int gy = (slide_h - 1) / cell + 1, gx = (slide_w - 1) / cell + 1;
    const long long cells = (long long)gy * gx;
    AY_CHECK_ARG(cells * C <= (1ll << 30), "ay_burden_bin: %d classes x %d x %d cells exceed 2^30 counters", C, gy, gx);
    hipStream_t st = S(stream);
    hipLaunchKernelGGL(burden_zero_kernel, dim3(burden_blocks(cells * C)), dim3(BURDEN_THREADS), 0, st, counts, cells * C, stats, C + 3);
    AY_CHECK_LAUNCH("burden_zero_kernel");
    if (M > 0) {
        hipLaunchKernelGGL(burden_bin_kernel, dim3((unsigned)(((long long)M + BURDEN_THREADS - 1) / BURDEN_THREADS)), dim3(BURDEN_THREADS), 0, st,
                           rows, M, C, slide_h, slide_w, cell, gx, (size_t)cells, min_conf, counts, stats);
        AY_CHECK_LAUNCH("burden_bin_kernel");
    }
    return AY_OK;
}

extern "C" size_t ay_field_select_workspace_bytes(int num_classes, int gy, int gx, int field) {
    if (!ay::burden_select_dims_ok(num_classes, gy, gx, field)) return 0;
    return ay::burden_carve(nullptr, num_classes, gy, gx, field).bytes;
}

extern "C" int ay_field_select(const int32_t* counts, int num_classes, int gy, int gx, const int32_t* tissue, int field, int need_tissue,
                               int top_k, int32_t* fields, int32_t* n_found, void* workspace, size_t workspace_bytes, ay_stream_t stream) {
    using namespace ay;
    const int C = num_classes, F = field, K = top_k;
    AY_CHECK_ARG(C >= 1 && C <= AY_BURDEN_MAX_CLASSES, "ay_field_select: num_classes %d outside 1 .. %d", C, AY_BURDEN_MAX_CLASSES);
    AY_CHECK_ARG(F >= 1 && F <= BURDEN_MAX_FIELD, "ay_field_select: field %d outside 1 .. %d (field x cell <= 46340)", F, BURDEN_MAX_FIELD);
    AY_CHECK_ARG(K >= 1 && K <= AY_BURDEN_MAX_FIELDS, "ay_field_select: top_k %d outside 1 .. %d", K, AY_BURDEN_MAX_FIELDS);
    AY_CHECK_ARG(burden_select_dims_ok(C, gy, gx, F), "ay_field_select: grid %d x %d", gy, gx);
    AY_CHECK_ARG(need_tissue >= 0, "ay_field_select: need_tissue %d < 0", need_tissue);
    AY_CHECK_ARG(counts && fields && n_found, "ay_field_select: null counts, fields or n_found");
    const BurdenWs w = burden_carve(workspace, C, gy, gx, F);
    AY_CHECK_ARG(workspace_bytes >= w.bytes && (w.bytes == 0 || workspace), "ay_field_select: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
    AY_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "ay_field_select: workspace not 16-byte aligned");
    hipStream_t st = S(stream);
    const int ny = gy >= F && gx >= F ? gy - F + 1 : 0, nx = ny ? gx - F + 1 : 0;
    const int planes = C + (tissue ? 1 : 0);
    if (ny > 0) {
        hipLaunchKernelGGL(burden_row_pass_kernel, dim3(burden_blocks((long long)gy * nx), planes), dim3(BURDEN_THREADS), 0, st, counts, tissue, C, gy,
                           gx, nx, F, w.rowsum);
        AY_CHECK_LAUNCH("burden_row_pass_kernel");
        const int32_t* elig = nullptr;
        if (tissue) {   // the tissue plane first: the class planes read its field sums
            hipLaunchKernelGGL(burden_col_pass_kernel, dim3(burden_blocks((long long)ny * nx), 1), dim3(BURDEN_THREADS), 0, st,
                               (const int32_t*)w.rowsum, C, gy, ny, nx, F, elig, 0, w.fieldsum);
            AY_CHECK_LAUNCH("burden_col_pass_kernel");
            elig = w.fieldsum + (size_t)C * ny * nx;
        }
        hipLaunchKernelGGL(burden_col_pass_kernel, dim3(burden_blocks((long long)ny * nx), C), dim3(BURDEN_THREADS), 0, st,
                           (const int32_t*)w.rowsum, 0, gy, ny, nx, F, elig, need_tissue, w.fieldsum);
        AY_CHECK_LAUNCH("burden_col_pass_kernel");
    }
    hipLaunchKernelGGL(burden_select_kernel, dim3(C), dim3(BURDEN_SELECT_THREADS), 0, st, (const int32_t*)w.fieldsum, C, ny, nx, F, tissue ? 1 : 0, K,
                       fields, n_found);
    AY_CHECK_LAUNCH("burden_select_kernel");
    return AY_OK;
}
