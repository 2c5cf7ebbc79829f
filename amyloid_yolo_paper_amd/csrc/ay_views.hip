// Dihedral test-time views for whole-slide detection (wsi.detect_region(views=...); THE VIEW RULE and THE VOTE RULE are stated in
// include/amyloid_yolo.h and restated in NumPy by tests/views_reference.py).
//
//   region_tiles_views_u8_kernel   the list cut of ay_ingest.hip (region_tiles_cut_u8_kernel), written in every requested view.  A
//                                  workgroup computes one 32 x 32 block of I0 (the image the cut kernel would write, pixel by pixel
//                                  through the same region_tap of ay_common.h, after the nearest resize) ONCE, keeps it in LDS and stores it into each view from there: the
//                                  slide bytes are fetched once for all views.  A view is a permutation of I0, so the block lands in
//                                  each view as one rectangle, written row by row: lanes run along the OUTPUT row also for the
//                                  transposed views, whose LDS reads then walk a column of the block.  LDS rows are 33 floats apart:
//                                  ds_read_b32 / ds_write_b32 bank by (addr / 4) % 32 within a half wave, which holds 8 quads x 4
//                                  rows of the rectangle: the row-wise reads (word 33 * row + 4 * quad + k) and the column-wise reads
//                                  (word 33 * (4 * quad + k) + row) both fall on bank 4 * quad + row + k, 32 different banks.
//   unview_rows_kernel             decoded rows (cx, cy, w, h, ...) of a view back to the frame of I0, in place.
//   view_votes_kernel              which views hold a row that supports an emitted detection: integer OR atomics, so the bits do not
//                                  depend on the order of arrival.
//   view_select_kernel             stable in-place compaction of the detections with enough votes, one workgroup per image.
//
// Every entry point is kernel launches only: no allocation, no host synchronisation, no memset or copy node, no scratch.
#include "ay_box.h"
#include "ay_cut.h"

namespace ay {

// VIEW_BLOCK, ViewList, take_views, region_tiles_views_u8_kernel and launch_views live in ay_cut.h, which ay_stain.hip shares.

__global__ void __launch_bounds__(256) unview_rows_kernel(float* __restrict__ pred, size_t total, int N, int K, ViewList views, float Sf) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int v = views.v[(i / N) % views.n];
        if (v == 0) continue;
        float* p = pred + i * K;
        const float cx = p[0], cy = p[1], w = p[2], h = p[3];
        const bool FX = v & 1, FY = (v >> 1) & 1, T = (v >> 2) & 1;
        const float a = T ? cy : cx, b = T ? cx : cy;
        p[0] = FX ? Sf - a : a;
        p[1] = FY ? Sf - b : b;
        p[2] = T ? h : w;
        p[3] = T ? w : h;
    }
}

__global__ void __launch_bounds__(256) zero_i32_kernel(int32_t* __restrict__ p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = 0;
}

constexpr int VOTE_CHUNK = 256;   // detections a workgroup holds in LDS at a time

// grid (x, batch): the workgroups of an image share its V * N rows; a workgroup walks the image's detections in chunks
__global__ void __launch_bounds__(256) view_votes_kernel(const float* __restrict__ pred, int n_views, int N, int C, float conf_thres,
                                                         float vote_thres, const float* __restrict__ rows, const int32_t* __restrict__ count,
                                                         int max_det, int32_t* __restrict__ votes) {
    __shared__ float det[5][VOTE_CHUNK];   // x1, y1, x2, y2, class
    __shared__ int bits[VOTE_CHUNK];
    const int b = blockIdx.y, K = 5 + C, tid = threadIdx.x;
    const int D = min(max(count[b], 0), max_det);
    const size_t R = (size_t)n_views * N;
    const float* pb = pred + (size_t)b * R * K;
    const float* rb = rows + (size_t)b * max_det * 7;
    for (int d0 = 0; d0 < D; d0 += VOTE_CHUNK) {   // D is the same for the whole workgroup
        const int nd = min(VOTE_CHUNK, D - d0);
        if (tid < nd) {
            const float* r = rb + (size_t)(d0 + tid) * 7;
            det[0][tid] = r[0];
            det[1][tid] = r[1];
            det[2][tid] = r[2];
            det[3][tid] = r[3];
            det[4][tid] = (float)(int)r[6];
        }
        bits[tid] = 0;
        __syncthreads();
        for (size_t r = (size_t)blockIdx.x * 256 + tid; r < R; r += (size_t)gridDim.x * 256) {
            const float* p = pb + r * K;
            if (!(p[4] >= conf_thres)) continue;
            int cls = 0;
            float best = p[5];
            for (int k = 1; k < C; ++k)
                if (p[5 + k] > best) best = p[5 + k], cls = k;   // first maximum
            const float x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
            const int bit = 1 << (int)(r / N);
            for (int d = 0; d < nd; ++d)
                if (det[4][d] == (float)cls && iou_p1(det[0][d], det[1][d], det[2][d], det[3][d], x1, y1, x2, y2) > vote_thres)
                    atomicOr(&bits[d], bit);
        }
        __syncthreads();
        if (tid < nd && bits[tid]) atomicOr(&votes[(size_t)b * max_det + d0 + tid], bits[tid]);
        __syncthreads();
    }
}

// one workgroup per image: chunks of 256 rows in order; a chunk is read into registers before any of it is written, and a row only
// ever moves towards the front, so nothing unread is overwritten
__global__ void __launch_bounds__(256) view_select_kernel(float* __restrict__ rows, int32_t* __restrict__ keep_idx, int32_t* __restrict__ count,
                                                          const int32_t* __restrict__ votes, int max_det, int min_views) {
    __shared__ int wave_sum[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cnt = count[b];
    const int D = min(max(cnt, 0), max_det);
    float* rb = rows + (size_t)b * max_det * 7;
    int32_t* kb = keep_idx ? keep_idx + (size_t)b * max_det : nullptr;
    const int32_t* vb = votes + (size_t)b * max_det;
    int base = 0;
    for (int d0 = 0; d0 < D; d0 += 256) {
        const int d = d0 + tid;
        float r[7];
        int ki = 0;
        bool take = false;
        if (d < D) {
            take = __popc((unsigned)vb[d] & 0xffu) >= min_views;
#pragma unroll
            for (int k = 0; k < 7; ++k) r[k] = rb[(size_t)d * 7 + k];
            if (kb) ki = kb[d];
        }
        const unsigned long long m = __ballot(take);
        if (lane == 0) wave_sum[wave] = __popcll(m);
        __syncthreads();   // every row of the chunk is in registers
        int pos = base + __popcll(m & ((1ull << lane) - 1ull));
        for (int k = 0; k < wave; ++k) pos += wave_sum[k];
        const int chunk = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
        if (take) {
#pragma unroll
            for (int k = 0; k < 7; ++k) rb[(size_t)pos * 7 + k] = r[k];
            if (kb) kb[pos] = ki;
        }
        base += chunk;
        __syncthreads();
    }
    if (tid == 0 && cnt <= max_det) count[b] = base;   // an overfull image keeps its count: the caller's check still fires
}

}  // namespace ay

extern "C" int ay_ingest_region_tiles_views_u8(const void* region_hwc_u8, int region_h, int region_w, size_t row_stride_bytes, int shrink,
                                               int tile, const int32_t* origins_xy, int n, const int* views, int n_views, int out_size,
                                               float* out_nchw, ay_stream_t stream) {
    using namespace ay;
    AY_CHECK_ARG(region_hwc_u8 && out_nchw && origins_xy && views, "ay_ingest_region_tiles_views_u8: null");
    AY_CHECK_ARG(region_h > 0 && region_w > 0 && row_stride_bytes >= (size_t)region_w * 3 && (shrink == 1 || shrink == 2),
                 "ay_ingest_region_tiles_views_u8: region %dx%d stride %zu shrink %d", region_h, region_w, row_stride_bytes, shrink);
    AY_CHECK_ARG(tile > 0 && tile <= (1 << 24) && n > 0 && out_size > 0, "ay_ingest_region_tiles_views_u8: %d tiles of %d -> %d", n, tile,
                 out_size);
    return launch_views(region_hwc_u8, region_h, region_w, row_stride_bytes, shrink, tile, origins_xy, n, views, n_views, out_size, out_nchw,
                        stream, PlainColour{}, "ay_ingest_region_tiles_views_u8");
}

extern "C" int ay_unview_rows(float* pred, int n_images, const int* views, int n_views, int n_rows, int num_classes, int img_dim,
                              ay_stream_t stream) {
    using namespace ay;
    AY_CHECK_ARG(pred && views, "ay_unview_rows: null");
    AY_CHECK_ARG(n_images > 0 && n_rows > 0 && num_classes > 0 && img_dim > 0, "ay_unview_rows: %d images of %d rows, %d classes, size %d",
                 n_images, n_rows, num_classes, img_dim);
    ViewList vl;
    AY_CHECK_ARG(take_views(views, n_views, &vl), "ay_unview_rows: need 1 .. 8 distinct view ids in 0 .. 7 (n_views %d)", n_views);
    const size_t total = (size_t)n_images * n_rows;
    size_t blocks = (total + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    hipLaunchKernelGGL(unview_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, S(stream), pred, total, n_rows, 5 + num_classes, vl,
                       (float)img_dim);
    AY_CHECK_LAUNCH("unview_rows_kernel");
    return AY_OK;
}

extern "C" int ay_view_votes(const float* pred, int batch, int n_views, int n_rows_per_view, int num_classes, float conf_thres,
                             float vote_thres, const float* rows, const int32_t* count, int max_det, int32_t* votes, ay_stream_t stream) {
    using namespace ay;
    AY_CHECK_ARG(pred && rows && count && votes, "ay_view_votes: null");
    AY_CHECK_ARG(batch > 0 && batch <= 65535 && n_views >= 1 && n_views <= 8 && n_rows_per_view > 0 && num_classes > 0 && max_det > 0,
                 "ay_view_votes: batch %d, %d views of %d rows, %d classes, max_det %d", batch, n_views, n_rows_per_view, num_classes,
                 max_det);
    const size_t nz = (size_t)batch * max_det;
    size_t zb = (nz + 255) / 256;
    if (zb > 1024) zb = 1024;
    hipLaunchKernelGGL(zero_i32_kernel, dim3((unsigned)zb), dim3(256), 0, S(stream), votes, nz);
    AY_CHECK_LAUNCH("zero_i32_kernel");
    const size_t R = (size_t)n_views * n_rows_per_view;
    size_t gx = (R + 255) / 256;
    if (gx > 128) gx = 128;
    hipLaunchKernelGGL(view_votes_kernel, dim3((unsigned)gx, (unsigned)batch), dim3(256), 0, S(stream), pred, n_views, n_rows_per_view,
                       num_classes, conf_thres, vote_thres, rows, count, max_det, votes);
    AY_CHECK_LAUNCH("view_votes_kernel");
    return AY_OK;
}

extern "C" int ay_view_select(float* rows, int32_t* keep_idx, int32_t* count, const int32_t* votes, int batch, int max_det, int min_views,
                              ay_stream_t stream) {
    using namespace ay;
    AY_CHECK_ARG(rows && count && votes, "ay_view_select: null");
    AY_CHECK_ARG(batch > 0 && max_det > 0 && min_views >= 1 && min_views <= 8, "ay_view_select: batch %d, max_det %d, min_views %d", batch,
                 max_det, min_views);
    hipLaunchKernelGGL(view_select_kernel, dim3((unsigned)batch), dim3(256), 0, S(stream), rows, keep_idx, count, votes, max_det, min_views);
    AY_CHECK_LAUNCH("view_select_kernel");
    return AY_OK;
}
