// The frame of the parity-path convolutions (ay_conv_f32_mfma.hip, ay_conv_split.hip): the reference's block on NCHW fp32
// activations and OIHW fp32 filters, route concatenation + nearest x2 upsampling folded into the loader, unfused fp32 epilogue.
// A workgroup (4 waves) owns 64 output channels x an 8 x 32 pixel tile of one image, a wave 64 channels x 2 tile rows: 2 x 2
// accumulator tiles of 32 x 32.  Here, once: the argument struct, workgroup -> item, the geometry of the source(s), the filter
// descriptor, and on the host the argument fill, the launch and the entry checks.  The per-lane offsets of a staged pixel, the
// stage descriptor, accumulator zeroing and the epilogue are written out in each kernel: an inline function that is handed the
// kernel's arrays changes the order in which the optimiser takes them apart, and with it the instruction stream.
#pragma once
#include "ay_common.h"

namespace ay {

constexpr int NCHW_BN = 64, NCHW_TH = 8, NCHW_TW = 32;   // the workgroup tile: output channels x rows x columns

struct NchwArgs {
    const float *s1, *s2, *w, *scale, *shift, *res;
    float* out;
    int cin, cin1, up1, cout, hin, win, hout, wout, leaky;
    int tiles_x, tiles_y, n_cgroups, n_items;
};

// ---- workgroup -> item: the workgroups of one XCD (id & 7) walk a contiguous range of items, channel groups of a pixel tile
// adjacent: the input halo tile is fetched from HBM once and then hit in that XCD's L2
struct NchwItem { int b, y0, x0, co0; };   // image, first output row / column / channel
__device__ __forceinline__ bool nchw_item_index(const NchwArgs& a, int& item) {   // false: nothing to do, return (before the divisions)
    const int per_xcd = (a.n_items + 7) >> 3;
    item = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    return (int)(blockIdx.x >> 3) < per_xcd && item < a.n_items;
}
__device__ __forceinline__ NchwItem nchw_item(const NchwArgs& a, const int& item) {
    const int cg = item % a.n_cgroups, pt = item / a.n_cgroups;
    return {pt / (a.tiles_x * a.tiles_y), ((pt / a.tiles_x) % a.tiles_y) * NCHW_TH, (pt % a.tiles_x) * NCHW_TW, cg * NCHW_BN};
}

// ---- sources.  Every load is a raw buffer load: a wave-uniform descriptor (rebuilt per stage: base = first channel of the
// stage, range = what is left of that source) + ONE 32-bit per-lane offset that never changes.  Lanes with nothing to fetch (zero
// padding, channels / filters beyond the tensor, units beyond the stage) carry an offset beyond every range -- it stays beyond
// after a channel term below 2^31 is added -- and read zeros: no 64-bit per-lane addresses, no branches (with plain pointers the
// fp32 kernel spilled).  Channels [0, cin1) come from src1 (at half resolution when up1), the rest from src2.
constexpr unsigned NCHW_OOB = 0x80000000u;

struct NchwSource {
    int w1;                    // row pitch of src1
    unsigned plane1, plane2;   // floats per channel of src1 / src2
    const float *img1, *img2;  // image b in src1 / src2
    __device__ __forceinline__ NchwSource(const NchwArgs& a, int b) {
        const int cin2 = a.cin - a.cin1;
        const int h1 = a.hin >> a.up1;
        w1 = a.win >> a.up1;
        plane1 = (unsigned)(h1 * w1), plane2 = (unsigned)(a.hin * a.win);
        img1 = a.s1 + (size_t)b * a.cin1 * plane1;
        img2 = cin2 > 0 ? a.s2 + (size_t)b * cin2 * plane2 : nullptr;
    }
};

// the filters from W[0][ci0][tap0] on, KK2 taps per channel.  The range ends with the last filter; a channel tail (cin not a
// multiple of the stage: the 3-channel stem) is masked by hand by the kernels, since an offset past the row of one filter lands in
// the next filter's row, not out of range
__device__ __forceinline__ __amdgpu_buffer_rsrc_t nchw_filter_rsrc(const NchwArgs& a, int KK2, int ci0, int tap0) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w) + (size_t)ci0 * KK2 + tap0, 0,
                                             ((a.cout * a.cin - ci0) * KK2 - tap0) * 4, 0x00020000);
}

// ---- host side.  `entry` is the C entry point's name: the prefix of its messages
// what ay_conv_fwd_f32, ay_conv_fwd_f32_valu and ay_conv_fwd_split ask of their arguments alike.  up1 == 1 reads src1 at
// (y >> 1, x >> 1) of a plane of (hin >> 1) x (win >> 1): an odd side would address one row / column past it
static inline int nchw_check_entry(const char* entry, const ay_conv_desc* d, const float* src1, int cin1, int up1, const float* src2,
                                   const float* w, const float* scale, const float* shift, const float* out) {
    AY_CHECK_ARG(d && src1 && w && scale && shift && out, "%s: null argument", entry);
    AY_CHECK_ARG(cin1 > 0 && cin1 <= d->cin && (cin1 == d->cin || src2), "%s: channel split %d/%d", entry, cin1, d->cin);
    AY_CHECK_ARG(up1 == 0 || (up1 == 1 && d->hin % 2 == 0 && d->win % 2 == 0), "%s: up1", entry);
    const int pad = (d->ksize - 1) / 2;
    AY_CHECK_ARG(d->stride > 0 && d->hout == (d->hin + 2 * pad - d->ksize) / d->stride + 1 && d->wout == (d->win + 2 * pad - d->ksize) / d->stride + 1,
                 "%s: output size mismatch", entry);
    return AY_OK;
}

// buffer descriptors address one image of either source and the filter tensor with 32-bit offsets
static inline bool nchw_fits_descriptors(const ay_conv_desc* d) {
    return (long long)d->cin * d->hin * d->win * 4 < (1ll << 31) && (long long)d->cout * d->cin * d->ksize * d->ksize * 4 < (1ll << 31);
}

static inline int nchw_fill_args(const char* entry, const ay_conv_desc* d, const float* src1, int cin1, int up1, const float* src2,
                                 const float* w, const float* scale, const float* shift, const float* residual, float* out, NchwArgs& a) {
    a.s1 = src1, a.s2 = src2, a.w = w, a.scale = scale, a.shift = shift, a.res = residual, a.out = out;
    a.cin = d->cin, a.cin1 = cin1, a.up1 = up1, a.cout = d->cout, a.hin = d->hin, a.win = d->win, a.hout = d->hout, a.wout = d->wout;
    a.leaky = d->leaky;
    a.tiles_x = (d->wout + NCHW_TW - 1) / NCHW_TW;
    a.tiles_y = (d->hout + NCHW_TH - 1) / NCHW_TH;
    a.n_cgroups = (d->cout + NCHW_BN - 1) / NCHW_BN;
    const long long n = (long long)a.tiles_x * a.tiles_y * d->batch * a.n_cgroups;
    AY_CHECK_ARG(n > 0 && n <= 0x3fffffffLL, "%s: grid out of range (%lld)", entry, n);
    a.n_items = (int)n;
    return AY_OK;
}

// launches the DUAL = true (`dual`) or false (`single`) instance of a kernel: a route has two sources
static inline int nchw_launch(void (*dual)(NchwArgs), void (*single)(NchwArgs), const char* what, const NchwArgs& a, hipStream_t st) {
    const unsigned grid = 8u * (unsigned)((a.n_items + 7) / 8);
    hipLaunchKernelGGL(a.cin1 < a.cin ? dual : single, dim3(grid), dim3(256), 0, st, a);
    AY_CHECK_LAUNCH(what);
    return AY_OK;
}

}  // namespace ay
