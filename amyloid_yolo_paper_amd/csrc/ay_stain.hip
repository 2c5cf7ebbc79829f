// Stain normalisation for whole-slide detection (wsi.stain_stats, wsi.StainMap, wsi.detect_region(stain=...), wsi.normalize_region;
// THE STAIN RULE is stated in include/amyloid_yolo.h and restated in NumPy fp32 by tests/stain_reference.py).
//
//   stain_hist_u8_kernel    histograms of the two stain concentrations over the tissue pixels of a resident region: a read stream
//                           that walks the IMAGE in ay_slide_pass.h's 48-byte items and work units, here of 16 rows x up to 2048
//                           items; the branches of the unrolled pixel loop diverge only on the tissue test.  A lane unmixes the
//                           TISSUE pixels of its item (od in LDS, D in scalar registers; most of a slide is glass and costs a
//                           minimum and a compare) and counts them in the workgroup's int32 LDS histograms, which go to the uint64
//                           histogram in memory with integer atomics when the workgroup is done, and every HIST_FLUSH units before
//                           that: HIST_FLUSH * 16 * 2048 * 16 < 2^31.
//   stain_apply_u8_kernel   the mapped (halved) image in the uint8 form, one pixel per thread.
//   The stain CUT is the cut kernel / the views kernel of ay_cut.h instantiated here with StainColour (ay_common.h) as colour stage.
//
// Every entry point is kernel launches only: no allocation, no host synchronisation, no memset or copy node, no scratch.
#include "ay_cut.h"
#include "ay_slide_pass.h"

namespace ay {

constexpr int HIST_WORDS = 2 * AY_STAIN_BINS + 1;

template <bool WIDE, int SHRINK>
__global__ void __launch_bounds__(256) stain_hist_u8_kernel(const uint8_t* __restrict__ reg, int H, int W, int RW, size_t stride, int bg,
                                                             int n_xc, long long units, const ay_stain_params* __restrict__ params,
                                                             unsigned long long* __restrict__ hist) {
    __shared__ float od[256];
    __shared__ int lh[HIST_WORDS];
    const int tid = threadIdx.x;
    od[tid] = params->od[tid];
    float D[9];                                              // uniform: scalar registers
#pragma unroll
    for (int i = 0; i < 9; ++i) D[i] = params->D[i];
    for (int i = tid; i < HIST_WORDS; i += 256) lh[i] = 0;
    __syncthreads();
    const unsigned row_bytes = (unsigned)RW * 3, used = (unsigned)W * (3 * SHRINK);   // bytes of a source row; those that belong to a pixel
    const unsigned nq = (used + SLIDE_ITEM - 1) / SLIDE_ITEM;
    int cnt = 0, pending = 0;                                // the lane's tissue pixels since the last flush
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {   // u is workgroup-uniform: so are the barriers of the flush
        const SlideUnit un = slide_unit<HIST_BAND, HIST_XQ>(u, n_xc, nq, 0, H);
        tissue_walk<WIDE, SHRINK>(
            reg, stride, row_bytes, used, un, bg, [](unsigned, int) {},
            [&](int, const int* b) {
                ++cnt;
                const float o0 = od[b[0]], o1 = od[b[1]], o2 = od[b[2]];
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const float c = (o0 * D[s] + o1 * D[3 + s]) + o2 * D[6 + s];
                    // c < 0 ? 0 : min((int)(c * 64), 511), without converting a float beyond the int range
                    const int bin = c < 0.0f ? 0 : (c < 8.0f ? (int)(c * 64.0f) : AY_STAIN_BINS - 1);
                    atomicAdd(&lh[s * AY_STAIN_BINS + bin], 1);
                }
            },
            []() {});
        if (++pending == HIST_FLUSH) flush_lds_hist(lh, HIST_WORDS, 2 * AY_STAIN_BINS, cnt, hist), pending = 0;
    }
    flush_lds_hist(lh, HIST_WORDS, 2 * AY_STAIN_BINS, cnt, hist);
}

__global__ void __launch_bounds__(256) stain_apply_u8_kernel(const uint8_t* __restrict__ reg, int RH, int RW, size_t stride, int shrink,
                                                              StainColour colour, uint8_t* __restrict__ out, size_t out_stride) {
    __shared__ StainColour::Tables tab;
    colour.load(tab);
    const int H = RH / shrink, W = RW / shrink;
    const size_t total = (size_t)H * W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned X = (unsigned)(i % W), Y = (unsigned)(i / W);
        int b[3];
        float px[3];
        if (!region_tap_u8(reg, stride, shrink, H, W, X, Y, b)) continue;   // never: X < W and Y < H
        colour.map(tab, b, px);
        uint8_t* o = out + (size_t)Y * out_stride + (size_t)X * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = (uint8_t)(px[c] * 255.0f + 0.5f);
    }
}

}  // namespace ay

extern "C" int ay_stain_hist_u8(const void* region_hwc_u8, int region_h, int region_w, size_t row_stride_bytes, int shrink, int bg_level,
                                const ay_stain_params* params_device, uint64_t* hist, ay_stream_t stream) {
    using namespace ay;
    AY_CHECK_ARG(region_hwc_u8 && params_device && hist, "ay_stain_hist_u8: null");
    if (!check_region("ay_stain_hist_u8", region_h, region_w, row_stride_bytes, shrink, true)) return AY_ERR_ARG;
    if (!check_bg_level("ay_stain_hist_u8", bg_level)) return AY_ERR_ARG;
    AY_CHECK_ARG(((uintptr_t)hist & 7) == 0, "ay_stain_hist_u8: hist %p", (void*)hist);
    const int H = region_h / shrink, W = region_w / shrink;
    if (H == 0 || W == 0) return AY_OK;   // a one-pixel region has no halved image
    const SlideUnits g = slide_units(W, shrink, H, HIST_BAND, HIST_XQ);
    launch_wide_shrink(region_hwc_u8, row_stride_bytes, shrink, [&](auto wide, auto sh) {
        hipLaunchKernelGGL((stain_hist_u8_kernel<wide.value, sh.value>), dim3(g.blocks), dim3(256), 0, S(stream), (const uint8_t*)region_hwc_u8,
                           H, W, region_w, row_stride_bytes, bg_level, g.n_xc, g.units, params_device, (unsigned long long*)hist);
    });
    AY_CHECK_LAUNCH("stain_hist_u8_kernel");
    return AY_OK;
}

extern "C" int ay_ingest_region_tiles_stain_u8(const void* region_hwc_u8, int region_h, int region_w, size_t row_stride_bytes, int shrink,
                                               int tile, const int32_t* origins_xy, int n, const int* views, int n_views,
                                               const ay_stain_params* params_device, int out_size, float* out_nchw, ay_stream_t stream) {
    using namespace ay;
    AY_CHECK_ARG(region_hwc_u8 && out_nchw && origins_xy && views && params_device, "ay_ingest_region_tiles_stain_u8: null");
    if (!check_region("ay_ingest_region_tiles_stain_u8", region_h, region_w, row_stride_bytes, shrink, false)) return AY_ERR_ARG;
    AY_CHECK_ARG(tile > 0 && tile <= (1 << 24) && n > 0 && out_size > 0, "ay_ingest_region_tiles_stain_u8: %d tiles of %d -> %d", n, tile,
                 out_size);
    if (n_views == 1 && views[0] == 0)   // the list cut's geometry and kernel
        return launch_cut(region_hwc_u8, region_h, region_w, row_stride_bytes, shrink, tile, ListOrigins{origins_xy}, (size_t)n, out_size,
                          out_nchw, stream, StainColour{params_device});
    return launch_views(region_hwc_u8, region_h, region_w, row_stride_bytes, shrink, tile, origins_xy, n, views, n_views, out_size, out_nchw,
                        stream, StainColour{params_device}, "ay_ingest_region_tiles_stain_u8");
}

extern "C" int ay_stain_apply_u8(const void* region_hwc_u8, int region_h, int region_w, size_t row_stride_bytes, int shrink,
                                 const ay_stain_params* params_device, uint8_t* out_hwc_u8, size_t out_stride_bytes, ay_stream_t stream) {
    using namespace ay;
    AY_CHECK_ARG(region_hwc_u8 && params_device && out_hwc_u8, "ay_stain_apply_u8: null");
    if (!check_region("ay_stain_apply_u8", region_h, region_w, row_stride_bytes, shrink, false)) return AY_ERR_ARG;
    const int H = region_h / shrink, W = region_w / shrink;
    AY_CHECK_ARG(out_stride_bytes >= (size_t)W * 3, "ay_stain_apply_u8: out rows of %d pixels %zu bytes apart", W, out_stride_bytes);
    if (H == 0 || W == 0) return AY_OK;   // a one-pixel region has no halved image
    const size_t total = (size_t)H * W;
    size_t blocks = (total + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    hipLaunchKernelGGL(stain_apply_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, S(stream), (const uint8_t*)region_hwc_u8, region_h, region_w,
                       row_stride_bytes, shrink, StainColour{params_device}, out_hwc_u8, out_stride_bytes);
    AY_CHECK_LAUNCH("stain_apply_u8_kernel");
    return AY_OK;
}
