// Tissue map for whole-slide detection (wsi.tissue_counts, wsi.detect_region(min_tissue > 0)): per tile of a wsi.tile_grid grid, the
// number of tissue pixels -- min(R, G, B) < bg_level on the (halved) image, THE RULE in include/amyloid_yolo.h -- counted straight
// out of a resident uint8 HWC region.  A pure read stream that walks the IMAGE, not the tiles: a source byte comes from memory once,
// also where tiles overlap (load instructions touch some bytes twice: a lane reads the 8 bytes behind its 16 again, which are its
// neighbour's, and two units that meet inside a 16-byte block both read that block; those are cache hits).
//
// The image is cut, per axis, at every tile start (a * step) and every tile end (a * step + tile): inside one such interval the set
// of tiles that contain a pixel is a fixed range [t_lo, t_hi].  A work unit is (a band of rows of one y interval) x (one x interval);
// a workgroup classifies the unit's pixels, sums in registers, reduces over the wave and the workgroup and issues ONE integer atomic
// per tile of the unit's range (1 tile without overlap; 2 or 4 in the shared bands).  Integer sums: the same bits every run.
//
// min(R, G, B) < bg is "some byte of the pixel < bg", so a lane works on BYTES: it takes 16 consecutive bytes of a row (one 16-byte
// load when base and row stride are 16-byte multiples, byte loads otherwise and at a row's ragged end) plus the 8 behind them,
// builds the mask of bytes below bg and ORs three neighbouring bits at the byte positions where a pixel starts (row offset % 3 == 0;
// % 6 == 0 on the halved image, whose byte value is the 2x2 round-half-up mean of four source bytes 3 apart and a row apart).
#include "ay_slide_pass.h"

namespace ay {

__global__ void __launch_bounds__(256) zero_i32_kernel(int32_t* __restrict__ p, int n) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = 0;
}

// bytes [o, o + 24) of one row into w[0..5]; bytes at or behind row_bytes read as 0 (they are never part of a counted pixel)
template <bool WIDE>
__device__ __forceinline__ void load24(const uint8_t* __restrict__ row, unsigned o, unsigned row_bytes, uint32_t w[6]) {
    if (WIDE && o + 24 <= row_bytes) {   // row and o are multiples of 16
        const u32x4 a = *(const u32x4*)(row + o);
        const uint2 b = *(const uint2*)(row + o + 16);
        w[0] = a[0], w[1] = a[1], w[2] = a[2], w[3] = a[3], w[4] = b.x, w[5] = b.y;
    } else {
#pragma unroll
        for (int d = 0; d < 6; ++d) {
            uint32_t v = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const unsigned at = o + 4 * d + b;
                if (at < row_bytes) v |= (uint32_t)row[at] << (8 * b);
            }
            w[d] = v;
        }
    }
}

// tiles (per axis) that contain the interval [lo, hi), which no tile boundary cuts: t * step <= lo and hi <= t * step + tile
__device__ __forceinline__ void tile_range(int lo, int hi, int tile, int step, int tiles, int& t_lo, int& t_hi) {
    t_hi = min(lo / step, tiles - 1);
    t_lo = hi > tile ? (hi - tile + step - 1) / step : 0;
}

template <bool WIDE, int SHRINK>
__global__ void __launch_bounds__(256) tile_tissue_u8_kernel(const uint8_t* __restrict__ reg, int H, int W, int RW, size_t stride, int tile,
                                                              int step, int tiles_y, int tiles_x, int bg, int band, int n_bands, int n_xint,
                                                              long long units, int32_t* __restrict__ counts) {
    __shared__ int wave_sum[4];
    constexpr int BPP = 3 * SHRINK;                          // source bytes of one row per image pixel
    constexpr uint32_t STARTS = SHRINK == 1 ? 0x9249u : 0x41041u;   // every BPP-th bit
    const int r = tile % step, m = r ? 2 : 1;                // intervals per step: [a*step, a*step + r) and [a*step + r, (a+1)*step)
    const unsigned row_bytes = (unsigned)RW * 3;
    const int tid = threadIdx.x;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {   // u is workgroup-uniform: so are the barriers below
        const int xi = (int)(u % n_xint);
        const int bi = (int)((u / n_xint) % n_bands);
        const int yi = (int)(u / ((long long)n_xint * n_bands));
        int y_lo = (yi / m) * step + ((yi % m) ? r : 0);
        int y_hi = min((m == 2 && yi % m == 0) ? (yi / m) * step + r : (yi / m + 1) * step, H);
        const int x_lo = (xi / m) * step + ((xi % m) ? r : 0);
        const int x_hi = min((m == 2 && xi % m == 0) ? (xi / m) * step + r : (xi / m + 1) * step, W);
        int ty0, ty1, tx0, tx1;
        tile_range(y_lo, y_hi, tile, step, tiles_y, ty0, ty1);
        tile_range(x_lo, x_hi, tile, step, tiles_x, tx0, tx1);
        y_lo += bi * band;
        y_hi = min(y_hi, y_lo + band);
        if (y_lo >= y_hi || x_lo >= x_hi || ty0 > ty1 || tx0 > tx1) continue;
        const unsigned b0 = (unsigned)x_lo * BPP, b1 = (unsigned)x_hi * BPP;   // the unit's bytes of a source row
        const unsigned q0 = b0 >> 4, nq = ((b1 + 15) >> 4) - q0;
        const unsigned items = (unsigned)(y_hi - y_lo) * nq;
        int cnt = 0;
        for (unsigned i = tid; i < items; i += 256) {
            const unsigned o = (q0 + i % nq) << 4;
            const int Y = y_lo + (int)(i / nq);
            uint32_t f = 0;   // bit j: the image byte at row offset o + j is below bg
            if (SHRINK == 1) {
                uint32_t w[6];
                load24<WIDE>(reg + (size_t)Y * stride, o, row_bytes, w);
#pragma unroll
                for (int j = 0; j < 18; ++j) f |= (uint32_t)(byte_of(w, j) < bg) << j;
            } else {
                uint32_t w0[6], w1[6];
                load24<WIDE>(reg + (size_t)(2 * Y) * stride, o, row_bytes, w0);
                load24<WIDE>(reg + (size_t)(2 * Y + 1) * stride, o, row_bytes, w1);
#pragma unroll
                for (int j = 0; j < 18; ++j)
                    f |= (uint32_t)(((byte_of(w0, j) + byte_of(w0, j + 3) + byte_of(w1, j) + byte_of(w1, j + 3) + 2) >> 2) < bg) << j;
            }
            const unsigned first = (BPP - o % BPP) % BPP;        // first pixel start at or behind o
            const unsigned lo = b0 > o ? b0 - o : 0u, hi = min(b1 - o, 16u);   // o < b1: hi >= 1
            const uint32_t range = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
            cnt += __builtin_popcount((f | (f >> 1) | (f >> 2)) & (STARTS << first) & range);
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) cnt += __shfl_down(cnt, d, 64);
        if ((tid & 63) == 0) wave_sum[tid >> 6] = cnt;
        __syncthreads();
        const int total = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
        __syncthreads();
        if (total) {
            const int nx = tx1 - tx0 + 1, nt = (ty1 - ty0 + 1) * nx;
            for (int t = tid; t < nt; t += 256) atomicAdd(counts + (size_t)(ty0 + t / nx) * tiles_x + (tx0 + t % nx), total);
        }
    }
}

}  // namespace ay

extern "C" int ay_tile_tissue_u8(const void* region_hwc_u8, int region_h, int region_w, size_t row_stride_bytes, int shrink, int tile,
                                 int step, int tiles_y, int tiles_x, int bg_level, int32_t* counts, ay_stream_t stream) {
    using namespace ay;
    AY_CHECK_ARG(region_hwc_u8 && counts, "ay_tile_tissue_u8: null");
    if (!check_region("ay_tile_tissue_u8", region_h, region_w, row_stride_bytes, shrink, true)) return AY_ERR_ARG;
    AY_CHECK_ARG(tile > 0 && tile <= 46340 /* a count is at most tile^2: int32 */ && step > 0 && step <= tile && tiles_y > 0 && tiles_x > 0 && (long long)tiles_y * tiles_x <= (1 << 30),
                 "ay_tile_tissue_u8: tile grid %dx%d of %d step %d", tiles_y, tiles_x, tile, step);
    if (!check_bg_level("ay_tile_tissue_u8", bg_level)) return AY_ERR_ARG;
    const int T = tiles_y * tiles_x;
    hipLaunchKernelGGL(zero_i32_kernel, dim3((unsigned)((T + 255) / 256 > 1024 ? 1024 : (T + 255) / 256)), dim3(256), 0, S(stream), counts, T);
    AY_CHECK_LAUNCH("zero_i32_kernel");
    const int H = region_h / shrink, W = region_w / shrink;
    if (H == 0 || W == 0) return AY_OK;   // a one-pixel region has no halved image
    const int m = tile % step ? 2 : 1;
    const int n_yint = (H + step - 1) / step * m, n_xint = (W + step - 1) / step * m;
    const int band = 32, n_bands = (step + band - 1) / band;   // rows of one unit: enough units to fill the chip on one strip
    const long long units = (long long)n_yint * n_bands * n_xint;
    const unsigned blocks = (unsigned)(units > 256 * 32 ? 256 * 32 : units);
    launch_wide_shrink(region_hwc_u8, row_stride_bytes, shrink, [&](auto wide, auto sh) {
        hipLaunchKernelGGL((tile_tissue_u8_kernel<wide.value, sh.value>), dim3(blocks), dim3(256), 0, S(stream), (const uint8_t*)region_hwc_u8,
                           H, W, region_w, row_stride_bytes, tile, step, tiles_y, tiles_x, bg_level, band, n_bands, n_xint, units, counts);
    });
    AY_CHECK_LAUNCH("tile_tissue_u8_kernel");
    return AY_OK;
}
