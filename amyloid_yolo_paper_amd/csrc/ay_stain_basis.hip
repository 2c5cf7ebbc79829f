// Stain basis estimation: each slide's own two stain vectors (wsi.estimate_basis; THE BASIS RULE is stated in include/amyloid_yolo.h
// and restated in NumPy and Python integers by tests/stain_basis_reference.py).  Integers only.
//
//   stain_moments_u8_kernel          n_tissue, n_sel and the first and second moments of the integer optical density over the SELECTED
//                                    pixels of a resident region.  A lane sums the pixels of its item in int32 registers (16 pixels of
//                                    at most 2466^2 fit), its items in 64-bit registers; when the workgroup has no unit left the
//                                    wavefronts reduce, meet in LDS, and memory sees at most 11 64-bit integer atomics per workgroup.
//   stain_direction_hist_u8_kernel   the histogram of d = p2 / (p1 + |p2|) over the selected pixels, p1 and p2 the projections on the
//                                    plane (eq1, eq2 in scalar registers): one unsigned 32-bit division per selected pixel, counted in
//                                    the workgroup's int32 LDS bins, which go to memory as stain_hist_u8_kernel's do, at the latest
//                                    every HIST_FLUSH units: HIST_FLUSH * 16 * 2048 * 16 < 2^31.
//
// Both walk ay_stain_hist_u8's read stream (ay_slide_pass.h: 48-byte items, units of 16 rows x up to 2048 items, the four (WIDE,
// SHRINK) instances), test for tissue before anything else and keep odq in LDS.  Kernel launches only: no allocation, no host
// synchronisation, no memset or copy node, no scratch.
#include "ay_slide_pass.h"

namespace ay {

constexpr int BASIS_EQ_MAX = 1024;  // |eq_c| <= 1024: |256 * p2| <= 2466 * 1024 * 3 * 256 < 2^31

// The walk over unit `un` with THE BASIS RULE's selection on top: tissue() for every tissue pixel of the item, selected(o0, o1, o2) for
// those whose smallest integer OD reaches beta_q, item_done() behind the item's last pixel.
template <bool WIDE, int SHRINK, typename Tissue, typename Selected, typename ItemDone>
__device__ __forceinline__ void basis_unit(const uint8_t* __restrict__ reg, size_t stride, unsigned row_bytes, unsigned used,
                                           const SlideUnit& un, const int* odq, int bg, int beta_q, Tissue tissue, Selected selected,
                                           ItemDone item_done) {
    tissue_walk<WIDE, SHRINK>(
        reg, stride, row_bytes, used, un, bg, [](unsigned, int) {},
        [&](int, const int* b) {
            tissue();
            const int o0 = odq[b[0]], o1 = odq[b[1]], o2 = odq[b[2]];
            if (min(min(o0, o1), o2) >= beta_q) selected(o0, o1, o2);
        },
        item_done);
}

template <bool WIDE, int SHRINK>
__global__ void __launch_bounds__(256) stain_moments_u8_kernel(const uint8_t* __restrict__ reg, int H, int W, int RW, size_t stride, int bg,
                                                                int beta_q, int n_xc, long long units,
                                                                const ay_stain_basis_params* __restrict__ params,
                                                                unsigned long long* __restrict__ moments) {
    constexpr int N = AY_BASIS_MOMENT_WORDS;
    __shared__ int odq[256];
    __shared__ unsigned long long part[4][N];
    const int tid = threadIdx.x;
    odq[tid] = params->odq[tid];
    __syncthreads();
    const unsigned row_bytes = (unsigned)RW * 3, used = (unsigned)W * (3 * SHRINK);
    const unsigned nq = (used + SLIDE_ITEM - 1) / SLIDE_ITEM;
    unsigned long long acc[N] = {};                          // the lane's sums over its items
    int it[N] = {};                                          // the sums of one item: 16 * 2466^2 < 2^31
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const SlideUnit un = slide_unit<HIST_BAND, HIST_XQ>(u, n_xc, nq, 0, H);
        basis_unit<WIDE, SHRINK>(
            reg, stride, row_bytes, used, un, odq, bg, beta_q, [&]() { ++it[0]; },
            [&](int o0, int o1, int o2) {
                ++it[1];
                it[2] += o0, it[3] += o1, it[4] += o2;
                it[5] += o0 * o0, it[6] += o0 * o1, it[7] += o0 * o2;
                it[8] += o1 * o1, it[9] += o1 * o2, it[10] += o2 * o2;
            },
            [&]() {
#pragma unroll
                for (int k = 0; k < N; ++k) acc[k] += (unsigned long long)(unsigned)it[k], it[k] = 0;
            });
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1)
#pragma unroll
        for (int k = 0; k < N; ++k) acc[k] += __shfl_down(acc[k], d, 64);
    if ((tid & 63) == 0)
#pragma unroll
        for (int k = 0; k < N; ++k) part[tid >> 6][k] = acc[k];
    __syncthreads();
    if (tid < N) {
        const unsigned long long v = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
        if (v) atomicAdd(moments + tid, v);
    }
}

template <bool WIDE, int SHRINK>
__global__ void __launch_bounds__(256) stain_direction_hist_u8_kernel(const uint8_t* __restrict__ reg, int H, int W, int RW, size_t stride,
                                                                       int bg, int beta_q, int a0, int a1, int a2, int c0, int c1, int c2,
                                                                       int n_xc, long long units,
                                                                       const ay_stain_basis_params* __restrict__ params,
                                                                       unsigned long long* __restrict__ hist) {
    __shared__ int odq[256];
    __shared__ int lh[AY_BASIS_HIST_WORDS];
    const int tid = threadIdx.x;
    odq[tid] = params->odq[tid];
    for (int i = tid; i < AY_BASIS_HIST_WORDS; i += 256) lh[i] = 0;
    __syncthreads();
    const unsigned row_bytes = (unsigned)RW * 3, used = (unsigned)W * (3 * SHRINK);
    const unsigned nq = (used + SLIDE_ITEM - 1) / SLIDE_ITEM;
    int cnt = 0, pending = 0;                                // the lane's selected pixels since the last flush
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {   // u is workgroup-uniform: so are the barriers of the flush
        const SlideUnit un = slide_unit<HIST_BAND, HIST_XQ>(u, n_xc, nq, 0, H);
        basis_unit<WIDE, SHRINK>(
            reg, stride, row_bytes, used, un, odq, bg, beta_q, []() {},
            [&](int o0, int o1, int o2) {
                ++cnt;
                const int p1 = (o0 * a0 + o1 * a1) + o2 * a2, p2 = (o0 * c0 + o1 * c1) + o2 * c2;
                int slot = AY_BASIS_DIR_BINS;                // p1 <= 0: outside the half plane
                if (p1 > 0) {
                    // floor(256 * p2 / (p1 + |p2|)) from one unsigned division: for p2 < 0 it is -ceil(256 * |p2| / (p1 + |p2|))
                    const unsigned m = (unsigned)(p2 < 0 ? -p2 : p2), den = (unsigned)p1 + m, num = m << 8;
                    const unsigned q = num / den;
                    const int k = p2 < 0 ? -(int)(q + (q * den != num)) : (int)q;
                    slot = k + AY_BASIS_DIR_BINS / 2;
                }
                atomicAdd(&lh[slot], 1);
            },
            []() {});
        if (++pending == HIST_FLUSH) flush_lds_hist(lh, AY_BASIS_HIST_WORDS, AY_BASIS_DIR_BINS + 1, cnt, hist), pending = 0;
    }
    flush_lds_hist(lh, AY_BASIS_HIST_WORDS, AY_BASIS_DIR_BINS + 1, cnt, hist);
}

static inline bool check_basis(const char* entry, const void* region, int region_h, int region_w, size_t row_stride_bytes, int shrink,
                               int bg_level, int beta_q, const void* params, const void* out) {
    if (!(region && params && out)) {
        set_error("%s: null", entry);
        return false;
    }
    if (!check_region(entry, region_h, region_w, row_stride_bytes, shrink, true)) return false;
    if (!check_bg_level(entry, bg_level)) return false;
    if (beta_q >= 0 && beta_q <= AY_BASIS_OD_MAX && ((uintptr_t)out & 7) == 0) return true;
    set_error("%s: beta_q %d, output %p", entry, beta_q, out);
    return false;
}

}  // namespace ay

extern "C" int ay_stain_moments_u8(const void* region_hwc_u8, int region_h, int region_w, size_t row_stride_bytes, int shrink, int bg_level,
                                   int beta_q, const ay_stain_basis_params* params_device, uint64_t* moments, ay_stream_t stream) {
    using namespace ay;
    if (!check_basis("ay_stain_moments_u8", region_hwc_u8, region_h, region_w, row_stride_bytes, shrink, bg_level, beta_q, params_device,
                     moments))
        return AY_ERR_ARG;
    const int H = region_h / shrink, W = region_w / shrink;
    if (H == 0 || W == 0) return AY_OK;   // a one-pixel region has no halved image
    const SlideUnits g = slide_units(W, shrink, H, HIST_BAND, HIST_XQ);
    launch_wide_shrink(region_hwc_u8, row_stride_bytes, shrink, [&](auto wide, auto sh) {
        hipLaunchKernelGGL((stain_moments_u8_kernel<wide.value, sh.value>), dim3(g.blocks), dim3(256), 0, S(stream),
                           (const uint8_t*)region_hwc_u8, H, W, region_w, row_stride_bytes, bg_level, beta_q, g.n_xc, g.units, params_device,
                           (unsigned long long*)moments);
    });
    AY_CHECK_LAUNCH("stain_moments_u8_kernel");
    return AY_OK;
}

extern "C" int ay_stain_direction_hist_u8(const void* region_hwc_u8, int region_h, int region_w, size_t row_stride_bytes, int shrink,
                                          int bg_level, int beta_q, int eq1_0, int eq1_1, int eq1_2, int eq2_0, int eq2_1, int eq2_2,
                                          const ay_stain_basis_params* params_device, uint64_t* hist, ay_stream_t stream) {
    using namespace ay;
    if (!check_basis("ay_stain_direction_hist_u8", region_hwc_u8, region_h, region_w, row_stride_bytes, shrink, bg_level, beta_q,
                     params_device, hist))
        return AY_ERR_ARG;
    const int eq[6] = {eq1_0, eq1_1, eq1_2, eq2_0, eq2_1, eq2_2};
    for (int i = 0; i < 6; ++i)
        AY_CHECK_ARG(eq[i] >= -BASIS_EQ_MAX && eq[i] <= BASIS_EQ_MAX, "ay_stain_direction_hist_u8: plane component %d outside -1024 .. 1024",
                     eq[i]);
    const int H = region_h / shrink, W = region_w / shrink;
    if (H == 0 || W == 0) return AY_OK;   // a one-pixel region has no halved image
    const SlideUnits g = slide_units(W, shrink, H, HIST_BAND, HIST_XQ);
    launch_wide_shrink(region_hwc_u8, row_stride_bytes, shrink, [&](auto wide, auto sh) {
        hipLaunchKernelGGL((stain_direction_hist_u8_kernel<wide.value, sh.value>), dim3(g.blocks), dim3(256), 0, S(stream),
                           (const uint8_t*)region_hwc_u8, H, W, region_w, row_stride_bytes, bg_level, beta_q, eq1_0, eq1_1, eq1_2, eq2_0,
                           eq2_1, eq2_2, g.n_xc, g.units, params_device, (unsigned long long*)hist);
    });
    AY_CHECK_LAUNCH("stain_direction_hist_u8_kernel");
    return AY_OK;
}
