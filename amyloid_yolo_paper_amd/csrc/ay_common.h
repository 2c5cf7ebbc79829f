// Shared helpers for the gfx950 kernels of libamyloid_yolo_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/amyloid_yolo.h"

namespace ay {

void set_error(const char* fmt, ...);

#define AY_CHECK_ARG(cond, ...)          \
    do {                                 \
        if (!(cond)) {                   \
            ay::set_error(__VA_ARGS__);  \
            return AY_ERR_ARG;           \
        }                                \
    } while (0)

#define AY_CHECK_LAUNCH(what)                                                      \
    do {                                                                           \
        hipError_t e_ = hipGetLastError();                                         \
        if (e_ != hipSuccess) {                                                    \
            ay::set_error("%s: %s", what, hipGetErrorString(e_));                  \
            return AY_ERR_LAUNCH;                                                  \
        }                                                                          \
    } while (0)

// a HIP runtime call (memset, copy, synchronise) of an entry point: its error string, or go on
#define AY_CHECK_HIP(call, what)                                                   \
    do {                                                                           \
        hipError_t e_ = (call);                                                    \
        if (e_ != hipSuccess) {                                                    \
            ay::set_error("%s: %s", what, hipGetErrorString(e_));                  \
            return AY_ERR_LAUNCH;                                                  \
        }                                                                          \
    } while (0)

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// round-to-nearest-even f32 -> bf16 bits (plain cast: keeps NaN a NaN, v_cvt_pk_bf16_f32 at -O3)
__device__ __forceinline__ uint16_t f2bf(float f) {
    __bf16 b = (__bf16)f;
    return __builtin_bit_cast(uint16_t, b);
}
__device__ __forceinline__ float bf2f(uint16_t u) {
    return __builtin_bit_cast(float, (uint32_t)u << 16);
}
__device__ __forceinline__ uint32_t pack2bf(float lo, float hi) {
    return (uint32_t)f2bf(lo) | ((uint32_t)f2bf(hi) << 16);
}
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
// two floats -> one dword of bf16 (round to nearest even) in a single v_cvt_pk_bf16_f32
__device__ __forceinline__ uint32_t pack2bf2(f32x2 v) {
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
}
// one dword of bf16 -> two floats
__device__ __forceinline__ f32x2 bf2f2(uint32_t u) {
    return f32x2{__builtin_bit_cast(float, u << 16), __builtin_bit_cast(float, u & 0xffff0000u)};
}
// LeakyReLU on two values: max(x, slope * x) equals x > 0 ? x : slope * x for 0 < slope <= 1 (slope 1: identity)
__device__ __forceinline__ f32x2 leaky2(f32x2 x, float slope) {
    const f32x2 y = x * slope;
    return f32x2{__builtin_fmaxf(x[0], y[0]), __builtin_fmaxf(x[1], y[1])};
}

// ---- the two 16-bit storage types of the MFMA inference path -------------------------------------------------------
// The convolution kernels are templates over DT: operand / activation element type, its two matrix instructions and the
// conversions of the fused epilogue.  Same layouts, same bytes, same MFMA rate; Bf16 keeps fp32's exponent range (training
// and default), F16 (IEEE binary16, inference only) has an 11-bit significand: an 8x smaller rounding step per stored
// activation, finite up to 65504 -- stored activations are post-BatchNorm, the fp32 epilogue applies scale / shift before
// the single rounding.  v_cvt_pk_f16_f32 / v_cvt_pk_bf16_f32 both round to nearest even.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
struct Bf16 {
    typedef bf16x8 vec8;
    static constexpr int id = AY_DT_BF16;
    static __device__ __forceinline__ f32x16 mfma32(vec8 a, vec8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ f32x4 mfma16(vec8 a, vec8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ uint32_t pack2(f32x2 v) { return pack2bf2(v); }
    static __device__ __forceinline__ f32x2 unpack2(uint32_t u) { return bf2f2(u); }
    static __device__ __forceinline__ uint16_t from_f32(float f) { return f2bf(f); }
    static __device__ __forceinline__ float to_f32(uint16_t u) { return bf2f(u); }
    static __device__ __forceinline__ void enter() {}   // (F16::enter sets a conversion mode bit; bfloat16 shares fp32's range)
};
struct F16 {
    typedef f16x8 vec8;
    static constexpr int id = AY_DT_F16;
    static __device__ __forceinline__ f32x16 mfma32(vec8 a, vec8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ f32x4 mfma16(vec8 a, vec8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ uint32_t pack2(f32x2 v) { return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2_t)); }
    static __device__ __forceinline__ f32x2 unpack2(uint32_t u) { return __builtin_convertvector(__builtin_bit_cast(f16x2_t, u), f32x2); }
    static __device__ __forceinline__ uint16_t from_f32(float f) { return __builtin_bit_cast(uint16_t, (_Float16)f); }
    // Called first thing by every kernel that stores halves: MODE.FP16_OVFL = 1 (hwreg 1 = MODE, bit 23): a conversion that
    // overflows the half range SATURATES at +-65504 instead of producing +-inf; true infinities and NaNs pass through.  A
    // post-BatchNorm or post-shortcut value beyond 65504 (the residual stream of Darknet-53 adds without bound across blocks; the
    // synthetic weights stay below 2 300) would otherwise become inf and turn into NaN one layer later without a diagnostic.
    // Free: a mode bit, no instruction per value.
    static __device__ __forceinline__ void enter() { __builtin_amdgcn_s_setreg(1 | (23 << 6) | (0 << 11), 1); }
    static __device__ __forceinline__ float to_f32(uint16_t u) { return (float)__builtin_bit_cast(_Float16, u); }
};
template <typename DT>
__device__ __forceinline__ uint32_t pack2_scalar(float lo, float hi) {
    return (uint32_t)DT::from_f32(lo) | ((uint32_t)DT::from_f32(hi) << 16);
}

// 16-byte LDS-DMA (global_load_lds_dwordx4): lane l copies 16 B from its own `gsrc` to LDS byte address `lds_addr + 16*l`
// (`lds_addr` wave-uniform).  Issued through inline asm so that hipcc neither counts it nor guards LDS reads against it:
// with the builtin the compiler inserted `s_waitcnt vmcnt(0)` between a DMA and the next ds_read / MFMA whenever it could
// not prove the buffers distinct (seen on the 3-deep 1x1 ring: every DMA was waited for on the spot, 6x slower).  The
// caller owns the ordering: a counted `s_waitcnt vmcnt(N)` + barrier before anyone reads the data.
__device__ __forceinline__ void dma16(const void* gsrc, unsigned lds_addr) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(__builtin_amdgcn_readfirstlane(lds_addr))
                 : "memory");
}
// The same through a buffer descriptor (buffer_load_dwordx4 ... lds): lane l copies 16 B from descriptor base + `soff` (scalar)
// + `voff` (its own 32-bit offset) to LDS byte address `lds_addr + 16*l`.  A lane whose `voff` is >= the descriptor's
// num_records (e.g. 0x80000000) is out of range and delivers zeros: border / padding lanes need no zero page and no select,
// and no lane carries a 64-bit address.  The scalar offset takes no part in the range check.
__device__ __forceinline__ void dma16_buf(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff, unsigned lds_addr) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(rsrc), "s"(soff), "s"(__builtin_amdgcn_readfirstlane(lds_addr))
                 : "memory");
}
// 4-byte variant (global_load_lds_dword): lane l copies 4 B from its own `gsrc` to LDS byte address `lds_addr + 4*l`;
// for sources that are only 4-byte aligned (fp32 image rows at arbitrary column offsets).
__device__ __forceinline__ void dma4(const void* gsrc, unsigned lds_addr) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(__builtin_amdgcn_readfirstlane(lds_addr))
                 : "memory");
}
__device__ __forceinline__ unsigned lds_addr_of(const void* p) {
    return (unsigned)(uintptr_t)(const __attribute__((address_space(3))) void*)p;
}

// The tap of the whole-slide cut (ay_cut.h: ay_ingest.hip, ay_views.hip, ay_stain.hip): pixel (X, Y) of the (halved, for shrink == 2) H x W slide that the
// region `reg` (rows `stride` bytes apart) holds -> px[3] in 0 .. 1; the background 255 = 1.0 outside.  shrink == 2 is the 2x2 mean
// with round-half-up in uint8.  X and Y are origin + offset added in `unsigned` (int32 origin, 0 <= offset < 2^24): a sum below 0
// or beyond 2^31 - 1 wraps to a value >= 2^31 > W, H, so the one unsigned comparison per axis gates every read for any origin, and
// no signed sum can overflow.
//
// region_tap_u8 hands out the (halved) bytes b[3] and whether the pixel lies inside (b is untouched outside); the COLOUR STAGE of
// the cut turns them into px[3].  PlainColour is byte / 255; StainColour is THE STAIN RULE's mapped value (include/amyloid_yolo.h),
// with od, A and T in LDS.  A cut kernel declares `__shared__ typename Colour::Tables tab`, calls colour.load(tab) once (every thread
// of the workgroup: it holds a barrier) and region_tap(colour, tab, ...) per pixel.
__device__ __forceinline__ bool region_tap_u8(const uint8_t* __restrict__ reg, size_t stride, int shrink, int H, int W, unsigned X,
                                              unsigned Y, int b[3]) {
    if (!(Y < (unsigned)H && X < (unsigned)W)) return false;
    if (shrink == 1) {
        const uint8_t* p = reg + (size_t)Y * stride + (size_t)X * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) b[c] = p[c];
    } else {
        const uint8_t* p0 = reg + (size_t)(2 * Y) * stride + (size_t)(2 * X) * 3;
        const uint8_t* p1 = p0 + stride;
#pragma unroll
        for (int c = 0; c < 3; ++c) b[c] = (p0[c] + p0[3 + c] + p1[c] + p1[3 + c] + 2) >> 2;
    }
    return true;
}

struct PlainColour {
    struct Tables {};
    __device__ __forceinline__ void load(Tables&) const {}
    __device__ __forceinline__ void map(const Tables&, const int b[3], float px[3]) const {
#pragma unroll
        for (int c = 0; c < 3; ++c) px[c] = (float)b[c] / 255.0f;
    }
};

// THE STAIN RULE's mapped value of one channel from its mapped optical density
__device__ __forceinline__ float stain_value(float o, const float* T) {
    o = o > 0.0f ? o : 0.0f;
    o = o < 4.0f ? o : 4.0f;
    const float u = o * 64.0f;
    const int k = min((int)u, 255);
    const float f = u - (float)k;
    const float t0 = T[k];
    float x = t0 + f * (T[k + 1] - t0);
    x = x > 0.0f ? x : 0.0f;
    return x < 1.0f ? x : 1.0f;
}

struct StainColour {
    const ay_stain_params* __restrict__ params;
    struct Tables {
        float od[256], A[9], T[257];
    };
    __device__ __forceinline__ void load(Tables& t) const {
        for (int i = threadIdx.x; i < 257; i += blockDim.x) {
            if (i < 256) t.od[i] = params->od[i];
            if (i < 9) t.A[i] = params->A[i];
            t.T[i] = params->T[i];
        }
        __syncthreads();
    }
    __device__ __forceinline__ void map(const Tables& t, const int b[3], float px[3]) const {
        const float o0 = t.od[b[0]], o1 = t.od[b[1]], o2 = t.od[b[2]];
#pragma unroll
        for (int c = 0; c < 3; ++c) px[c] = stain_value((o0 * t.A[c] + o1 * t.A[3 + c]) + o2 * t.A[6 + c], t.T);
    }
};

template <typename Colour>
__device__ __forceinline__ void region_tap(const Colour& colour, const typename Colour::Tables& tab, const uint8_t* __restrict__ reg,
                                           size_t stride, int shrink, int H, int W, unsigned X, unsigned Y, float px[3]) {
    int b[3];
    px[0] = px[1] = px[2] = 1.0f;
    if (region_tap_u8(reg, stride, shrink, H, W, X, Y, b)) colour.map(tab, b, px);
}

static inline hipStream_t S(ay_stream_t s) { return (hipStream_t)s; }

}  // namespace ay
