// Split-bf16 parity path: the convolutional block of ay_conv_f32_mfma.hip (NCHW fp32 in and out, OIHW fp32 filters, route +
// nearest x2 upsample in the loader, the same unfused fp32 epilogue) with every fp32 operand written as a sum of bf16 planes
// and the plane products run on v_mfma_f32_32x32x16_bf16 (1024 FLOP/clk/SIMD against 64 for v_mfma_f32_32x32x2_f32).
//
// THE SPLIT RULE (include/amyloid_yolo.h): p0 = bf16_rne(x), p1 = bf16_rne(x - p0), p2 = bf16_rne(x - p0 - p1), subtractions in
// fp32 (exact).  nsplit = 2 ("bf16x3") accumulates p0q0 + p0q1 + p1q0; nsplit = 3 ("bf16x6") adds p0q2 + p2q0 + p1q1.
// nsplit = 2: one set of fp32 accumulators, per tap in the order (0,0) (0,1) (1,0).  nsplit = 3: p0q0 goes to one set and the five
// correction products, (0,1) (1,0) (0,2) (2,0) (1,1) per tap, to a second one that is added in the epilogue: the chain that carries
// the leading bits then rounds once per tap instead of six times (measured against float64: 0.2 .. 0.5 of the exact-fp32 kernel's
// own error, against 0.7 .. 1.2 with one set -- which missed the model-level 1e-4 bar on one fixture).
//
// The frame is ay_conv_nchw.h's, shared with the fp32 kernel: the workgroup tile, the item walk, the geometry of the sources,
// the filter descriptor, the host side.  As there, the next fill is prefetched into registers under the MFMAs of this one.
//
// Stage = 16 input channels = the K of one MFMA (the 3-channel stem and a cin % 16 tail are zero-filled).  A loader thread owns
// one K-HALF (8 channels) of one pixel or of one (tap, filter): 8 plane-strided loads (coalesced across lanes along the pixels),
// the split, one 16-byte ds_write_b128 per plane.
//
// LDS image, per plane:   pixels  [k-half][P][8 ch] bf16        filters  [k-half][tap][co][8 ch] bf16
// i.e. the 32-byte row [16 ch] of a pixel / filter is stored as its two 16-byte k-halves in two arrays of 16-byte pitch.  The
// MFMA operand of lane l (r = l & 31, h = l >> 5: k = 8 h + j) is ONE ds_read_b128 at half h, position base + r.  ds_read_b128
// is served in 16-lane groups {0-3,12-15,20-27} {4-11,16-19,28-31} (+32); the r of a group are the 16 residues modulo 16, so at a
// 16-byte pitch a group covers the 16 slots of the 256-byte bank row exactly once for ANY base: conflict-free without padding
// (a [P][16 ch] image at a 32-byte pitch would put a group on the 8 even slots twice).  Stride 2 stores the columns of a pixel
// row as [even columns | odd columns], so that the 32 pixels of a tap (columns 2 r + kw) are again 32 consecutive positions.
// Per tap: 4 nsplit ds_read_b128 for 4 {3 | 6} MFMAs.
//
// LDS budget: a full 3x3 filter stage of three planes (54 KiB) plus the stride-2 halo tile (17 x 65 pixels x 32 B x 3 =
// 104 KiB) exceeds a CU's 160 KiB, so filters are staged PER TAP ROW: a stage is KS fills (fill = the KS taps of one kernel
// row, 64 x KS x 32 B per plane); the pixel tile is written on the first fill of a stage only.  Stride 1: 33 / 50 KiB (two
// workgroups per CU), 1x1: 20 / 30 KiB, stride 2: 81 / 122 KiB (one workgroup per CU).  static_assert below.
// Registers: the second accumulator set of nsplit = 3 leaves the 3x3 stride-1 instance no room for the prefetch at two workgroups
// per CU (LATE_LOADS below).
#include "ay_conv_nchw.h"

namespace ay {

// THE SPLIT RULE on 8 values: plane p of v[0..7] as 8 bf16 in 4 dwords
template <int NSPLIT>
__device__ __forceinline__ void split8(const float (&v)[8], u32x4 (&pl)[NSPLIT]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f32x2 r = {v[2 * j], v[2 * j + 1]};
#pragma unroll
        for (int p = 0; p < NSPLIT; ++p) {
            const uint32_t u = pack2bf2(r);
            pl[p][j] = u;
            if (p + 1 < NSPLIT) r = r - bf2f2(u);   // exact in fp32
        }
    }
}

template <int KS, int STRIDE, int NSPLIT>
struct SplitGeom {
    static constexpr int BN = NCHW_BN, TH = NCHW_TH, TW = NCHW_TW, KC = 16;
    static constexpr int TP = KS;                 // taps per fill: one kernel row
    static constexpr int IN_H = (TH - 1) * STRIDE + KS, IN_W = (TW - 1) * STRIDE + KS;
    static constexpr int XPL = IN_H * IN_W;
    static constexpr int XHALF = XPL * 16, XPLANE = 2 * XHALF;          // bytes
    static constexpr int WHALF = TP * BN * 16, WPLANE = 2 * WHALF;      // bytes
    static constexpr int LDS_BYTES = NSPLIT * (XPLANE + WPLANE);
    static constexpr int WG_PER_CU = LDS_BYTES <= 80 * 1024 ? 2 : 1;
    // nsplit = 3 carries two accumulator sets (128 registers).  With the 40 registers of the prefetch on top the 3x3 stride-1
    // instance does not fit the 256 registers a lane has at two workgroups per CU (it spilled), and one workgroup per CU measured
    // 0.96 of the fp32 path: that instance loads a fill between the two barriers instead, where the registers are needed for
    // nothing else, and leaves the latency to the other workgroup of the CU
    static constexpr bool LATE_LOADS = NSPLIT == 3 && KS == 3 && STRIDE == 1;
    static_assert(LDS_BYTES * WG_PER_CU <= 160 * 1024, "LDS budget of a CU");
};

template <int KS, int STRIDE, int NSPLIT, bool DUAL>
__global__ void __launch_bounds__(256, (SplitGeom<KS, STRIDE, NSPLIT>::WG_PER_CU)) conv_split_kernel(NchwArgs a) {
    using G = SplitGeom<KS, STRIDE, NSPLIT>;
    constexpr int BN = G::BN, TH = G::TH, TW = G::TW, KC = G::KC, TP = G::TP;
    constexpr int PAD = (KS - 1) / 2, KK2 = KS * KS, NPASS = KS;
    constexpr int IN_W = G::IN_W, XPL = G::XPL;
    constexpr int XHALF = G::XHALF, XPLANE = G::XPLANE, WHALF = G::WHALF, WPLANE = G::WPLANE;
    constexpr int EVENS = (IN_W + 1) / 2;           // stride 2: positions [0, EVENS) of a row hold its even columns
    constexpr int NXU = (2 * XPL + 255) / 256;      // pixel units (k-half of one pixel) per thread and stage
    constexpr int NWU = (2 * TP * BN + 255) / 256;  // filter units (k-half of one (tap, filter)) per thread and fill
    static_assert(TW == 32 && TH == 8 && BN == 64 && KC == 16, "wave tiling below");

    __shared__ __attribute__((aligned(16))) unsigned char lds[G::LDS_BYTES];
    unsigned char* const lx = lds;
    unsigned char* const lw = lds + NSPLIT * XPLANE;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int c = lane & 31, hh = lane >> 5;

    int item;
    if (!nchw_item_index(a, item)) return;
    const NchwItem it = nchw_item(a, item);
    const int b = it.b, y0 = it.y0, x0 = it.x0, co0 = it.co0;

    // ---- staging maps, fixed for the K loop: one fixed 32-bit offset per unit (ay_conv_nchw.h); the loads add j * plane * 4 < 2^31
    const NchwSource src(a, b);
    const int w1 = src.w1;
    const unsigned plane1 = src.plane1, plane2 = src.plane2;
    const float *const img1 = src.img1, *const img2 = src.img2;
    unsigned xo1[DUAL ? NXU : 1], xo2[NXU];  // byte offset of channel 8 * half of the stage in src1 (DUAL only) / in the plain source
#pragma unroll
    for (int i = 0; i < NXU; ++i) {
        const int e = i * 256 + tid;
        const int half = e / XPL, P = e % XPL;
        const int iy = y0 * STRIDE - PAD + P / IN_W, ix = x0 * STRIDE - PAD + P % IN_W;
        const bool in = e < 2 * XPL && iy >= 0 && iy < a.hin && ix >= 0 && ix < a.win;
        if constexpr (DUAL) {
            xo1[i] = in ? (unsigned)(half * 8 * plane1 + (iy >> a.up1) * w1 + (ix >> a.up1)) * 4u : NCHW_OOB;
            xo2[i] = in ? (unsigned)(half * 8 * plane2 + iy * a.win + ix) * 4u : NCHW_OOB;
        } else {  // one source, possibly at half resolution (a lazily upsampled layer)
            xo2[i] = in ? (unsigned)(half * 8 * plane1 + (iy >> a.up1) * w1 + (ix >> a.up1)) * 4u : NCHW_OOB;
        }
    }
    // filter unit u -> (co = u / (2 TP), half = (u / TP) & 1, tap of the fill = u % TP): byte offset of W[co][8 half][tap] from
    // W[0][stage's first channel][fill's first tap]
    unsigned wo[NWU];
#pragma unroll
    for (int i = 0; i < NWU; ++i) {
        const int u = i * 256 + tid;
        const int co = co0 + u / (2 * TP), half = (u / TP) & 1, t = u % TP;
        wo[i] = (u < 2 * TP * BN && co < a.cout) ? (unsigned)((co * a.cin + half * 8) * KK2 + t) * 4u : NCHW_OOB;
    }

    float rx[NXU][8], rw[NWU][8];
    auto issue_x = [&](int s) __attribute__((always_inline)) {
        const int ci0 = s * KC;
        const bool from1 = ci0 < a.cin1;   // wave-uniform: a stage never straddles the route boundary (host-checked)
        const float* base = from1 ? img1 + (size_t)ci0 * plane1 : img2 + (size_t)(ci0 - a.cin1) * plane2;
        const int left = from1 ? (a.cin1 - ci0) * (int)plane1 : (a.cin - ci0) * (int)plane2;   // floats up to the end of this source
        const unsigned pstep = (DUAL ? (from1 ? plane1 : plane2) : plane1) * 4u;
        const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, left * 4, 0x00020000);
#pragma unroll
        for (int i = 0; i < NXU; ++i) {
            unsigned off = xo2[i];
            if constexpr (DUAL) off = from1 ? xo1[i] : xo2[i];
#pragma unroll
            for (int j = 0; j < 8; ++j)
                rx[i][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xr, off + (unsigned)j * pstep, 0, 0));
        }
    };
    auto issue_w = [&](int s, int pass) __attribute__((always_inline)) {
        // a channel tail (cin % 16 != 0: the 3-channel stem) is masked by hand in commit_w
        const __amdgpu_buffer_rsrc_t wr = nchw_filter_rsrc(a, KK2, s * KC, pass * TP);
#pragma unroll
        for (int i = 0; i < NWU; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j)
                rw[i][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wr, wo[i] + (unsigned)(j * KK2 * 4), 0, 0));
    };
    auto commit_x = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NXU; ++i) {
            const int e = i * 256 + tid;
            const int half = e / XPL, P = e % XPL;
            const int ry = P / IN_W, rc = P % IN_W;
            const int q = ry * IN_W + (STRIDE == 1 ? rc : (rc & 1) * EVENS + (rc >> 1));
            u32x4 pl[NSPLIT];
            split8<NSPLIT>(rx[i], pl);
            if (e < 2 * XPL) {
#pragma unroll
                for (int p = 0; p < NSPLIT; ++p) *reinterpret_cast<u32x4*>(lx + p * XPLANE + half * XHALF + q * 16) = pl[p];
            }
        }
    };
    auto commit_w = [&](int s) __attribute__((always_inline)) {   // s: the stage the registers were loaded for
        const int live = a.cin - s * KC;                              // real channels of that stage
#pragma unroll
        for (int i = 0; i < NWU; ++i) {
            const int u = i * 256 + tid;
            const int col = u / (2 * TP), half = (u / TP) & 1, t = u % TP;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (half * 8 + j < live) ? rw[i][j] : 0.f;
            u32x4 pl[NSPLIT];
            split8<NSPLIT>(v, pl);
            if (u < 2 * TP * BN) {
#pragma unroll
                for (int p = 0; p < NSPLIT; ++p) *reinterpret_cast<u32x4*>(lw + p * WPLANE + half * WHALF + (t * BN + col) * 16) = pl[p];
            }
        }
    };

    f32x16 acc[2][2];
    // nsplit = 3: the five correction products go to a second accumulator set, added to the first in the epilogue, so that the
    // chain that carries the result's leading bits rounds once per tap, not six times
    constexpr bool TWO_SETS = NSPLIT == 3;
    f32x16 cor[2][2];   // left alone, and no registers, with one set
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        acc[i >> 5][(i >> 4) & 1][i & 15] = 0.f;
        if constexpr (TWO_SETS) cor[i >> 5][(i >> 4) & 1][i & 15] = 0.f;
    }

    // fragment bases: A = filter c (+32 m), k-half hh; B = pixel (row 2 wave + n, column c), k-half hh
    const unsigned char* const fa = lw + hh * WHALF + c * 16;
    const unsigned char* const fb = lx + hh * XHALF + ((2 * wave * STRIDE) * IN_W + c) * 16;

    const int nstages = (a.cin + KC - 1) / KC;
    issue_x(0);
    issue_w(0, 0);
    commit_x();
    commit_w(0);
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < nstages; ++s) {
        const bool more = s + 1 < nstages;
#pragma unroll
        for (int pass = 0; pass < NPASS; ++pass) {
            const bool last_pass = pass == NPASS - 1;
            auto issue_next = [&]() __attribute__((always_inline)) {
                if (!last_pass) {
                    issue_w(s, pass + 1);
                } else if (more) {
                    issue_x(s + 1);
                    issue_w(s + 1, 0);
                }
            };
            if constexpr (!G::LATE_LOADS) issue_next();
            // the loads stay in front of the MFMAs and the split of what they bring stays behind them: left alone, the scheduler
            // sinks the loads to the end of the block or hoists the split (and its wait for the loads) above it
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < TP; ++t) {
                const int kh = pass, kw = t;   // TP == KS: fill `pass` holds kernel row `pass`
                const int pos = STRIDE == 1 ? kw : (kw & 1) * EVENS + (kw >> 1);
                bf16x8 af[NSPLIT][2], bf[NSPLIT][2];
#pragma unroll
                for (int p = 0; p < NSPLIT; ++p) {
#pragma unroll
                    for (int m = 0; m < 2; ++m) af[p][m] = *reinterpret_cast<const bf16x8*>(fa + p * WPLANE + (t * BN + m * 32) * 16);
#pragma unroll
                    for (int n = 0; n < 2; ++n)
                        bf[p][n] = *reinterpret_cast<const bf16x8*>(fb + p * XPLANE + ((n * STRIDE + kh) * IN_W + pos) * 16);
                }
#pragma unroll
                for (int k = 0; k < (NSPLIT == 2 ? 3 : 6); ++k) {
                    constexpr int PA[6] = {0, 0, 1, 0, 2, 1}, PB[6] = {0, 1, 0, 2, 0, 1};
#pragma unroll
                    for (int m = 0; m < 2; ++m)
#pragma unroll
                        for (int n = 0; n < 2; ++n) {
                            if constexpr (TWO_SETS) {
                                if (k > 0) {
                                    cor[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[PA[k]][m], bf[PB[k]][n], cor[m][n], 0, 0, 0);
                                    continue;
                                }
                            }
                            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[PA[k]][m], bf[PB[k]][n], acc[m][n], 0, 0, 0);
                        }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if (!last_pass || more) {
                __syncthreads();
                if constexpr (G::LATE_LOADS) issue_next();
                if (last_pass) commit_x();
                commit_w(last_pass ? s + 1 : s);
                __syncthreads();
            }
        }
    }

    // ---- epilogue: C/D layout of 32x32: column (pixel) = lane & 31, row (channel) = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    const int ox = x0 + c;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int oy = y0 + 2 * wave + n;
        if (oy >= a.hout || ox >= a.wout) continue;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                if (co < a.cout) {
                    float sum = acc[m][n][r];
                    if constexpr (TWO_SETS) sum += cor[m][n][r];
                    float y = sum * a.scale[co] + a.shift[co];
                    if (a.leaky) y = y > 0.f ? y : 0.1f * y;
                    const size_t o = (((size_t)b * a.cout + co) * a.hout + oy) * a.wout + ox;
                    if (a.res) y += a.res[o];
                    a.out[o] = y;
                }
            }
    }
}

template <int KS, int STRIDE, int NSPLIT>
static int launch_split(const NchwArgs& a, hipStream_t st) {
    return nchw_launch(conv_split_kernel<KS, STRIDE, NSPLIT, true>, conv_split_kernel<KS, STRIDE, NSPLIT, false>, "conv_split_kernel", a, st);
}

template <int NSPLIT>
static int dispatch_split(const ay_conv_desc* d, const NchwArgs& a, hipStream_t st) {
    if (d->ksize == 3 && d->stride == 1) return launch_split<3, 1, NSPLIT>(a, st);
    if (d->ksize == 3 && d->stride == 2) return launch_split<3, 2, NSPLIT>(a, st);
    return launch_split<1, 1, NSPLIT>(a, st);
}

}  // namespace ay

extern "C" int ay_conv_fwd_split(const ay_conv_desc* d, const float* src1, int cin1, int up1, const float* src2, const float* w_oihw,
                                 const float* scale, const float* shift, const float* residual, float* out, int nsplit,
                                 ay_stream_t stream) {
    using namespace ay;
    const char* const entry = "ay_conv_fwd_split";
    if (const int rc = nchw_check_entry(entry, d, src1, cin1, up1, src2, w_oihw, scale, shift, out)) return rc;
    AY_CHECK_ARG(nsplit == 2 || nsplit == 3, "ay_conv_fwd_split: nsplit %d (2 = bf16x3, 3 = bf16x6)", nsplit);
    AY_CHECK_ARG(d->batch > 0 && d->cin > 0 && d->cout > 0 && d->hin > 0 && d->win > 0, "ay_conv_fwd_split: empty tensor");
    AY_CHECK_ARG((d->ksize == 3 && (d->stride == 1 || d->stride == 2)) || (d->ksize == 1 && d->stride == 1),
                 "ay_conv_fwd_split: %dx%d stride %d is not covered (3x3 stride 1 / 2, 1x1 stride 1)", d->ksize, d->ksize, d->stride);
    // a stage of 16 channels never straddles the route boundary
    AY_CHECK_ARG(cin1 == d->cin || cin1 % 16 == 0, "ay_conv_fwd_split: a route's first source needs a multiple of 16 channels (got %d)", cin1);
    AY_CHECK_ARG(nchw_fits_descriptors(d), "ay_conv_fwd_split: an image or the filter tensor exceeds the 32-bit descriptor range");
    NchwArgs a;
    if (const int rc = nchw_fill_args(entry, d, src1, cin1, up1, src2, w_oihw, scale, shift, residual, out, a)) return rc;
    return nsplit == 2 ? dispatch_split<2>(d, a, S(stream)) : dispatch_split<3>(d, a, S(stream));
}
