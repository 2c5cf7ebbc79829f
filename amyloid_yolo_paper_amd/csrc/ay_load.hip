// Amyloid load (wsi.stain_load, wsi.quantify_region(load=True); THE LOAD RULE is stated in include/amyloid_yolo.h and restated in NumPy
// by tests/load_reference.py): the tissue pixels, the stain-positive pixels and the sum of their bins, per cell of the burden grid and
// per detection box, out of a resident strip of the slide.
//
//   stain_load_cells_kernel   the hot path: a read stream over the IMAGE in the mould of stain_hist_u8_kernel (ay_stain.hip): the same
//                             48-byte items (16 whole pixels of a row, 8 of the halved image), the same choice of 16-byte or byte loads,
//                             od in LDS, the three D of the ONE chosen stain in scalar registers, the tissue test before the unmixing.
//                             A work unit is 16 rows x up to 256 items.  AY_LOAD_MIN_CELL = 16 makes an item's 16 pixels lie in at
//                             most two cells of a row and a 16-row band in at most two cell rows: a lane sums its item in registers
//                             (two masks, two bin sums), splits them at the one cell boundary the item can hold and adds what is not 0
//                             to the workgroup's int32 table in LDS, [2 cell rows][LOAD_CX cells][3]; after every unit the table's
//                             used part goes to memory, one 64-bit integer atomic per (cell, sum) that is not 0, lanes on consecutive
//                             words, and is zeroed again.  Memory never sees an atomic per pixel or per lane.
//   stain_load_boxes_kernel   a gather: one wavefront per box, boxes grid-stride.  THE LOAD RULE's box in four fp32 steps, an integer
//                             intersection with the strip (most boxes miss it), the lanes over the pixels of the intersection (byte
//                             loads: region_tap_u8's), 64-bit sums per lane, a wave reduction and at most four 64-bit atomics per box
//                             and strip.  Correct for any box; ONE HUGE BOX RUNS ON ONE WAVE (it is sized for detections).
//
// Integers and order-free integer atomics only: the same bytes every run.  Kernel launches only: no allocation, no memset node, no
// host read, no scratch.
#include "ay_box.h"
#include "ay_common.h"

namespace ay {

constexpr int LOAD_BAND = 16;     // rows of a work unit
constexpr int LOAD_ITEM = 48;     // bytes of a row a lane takes at a time: 16 pixels, 8 of the halved image
constexpr int LOAD_XQ = 256;      // items of a row in a work unit: 4096 pixels, 2048 of the halved image
// cells a unit's pixels can lie in, per cell row: its <= 4096 pixels start r < cell pixels into a cell, (r + 4095) / cell + 1 <= 257
constexpr int LOAD_CX = LOAD_XQ * 16 / AY_LOAD_MIN_CELL + 1;
// The int32 table is flushed after EVERY unit: a word holds at most the bins of the unit's 16 * 256 * 16 = 65536 pixels, each at most
// 511: 33 488 896 < 2^31.
constexpr int LOAD_WORDS = 2 * LOAD_CX * 3;
constexpr int LOAD_MAX_SIDE = 1 << 24;   // H, W of the slide: (float)W is exact (THE LOAD RULE)

// THE STAIN RULE's bin of the chosen stain's concentration
__device__ __forceinline__ int load_bin(const float* od, const int b[3], float d0, float d1, float d2) {
    const float c = (od[b[0]] * d0 + od[b[1]] * d1) + od[b[2]] * d2;
    return c < 0.0f ? 0 : (c < 8.0f ? (int)(c * 64.0f) : AY_STAIN_BINS - 1);
}

template <bool WIDE, int SHRINK>
__global__ void __launch_bounds__(256) stain_load_cells_kernel(const uint8_t* __restrict__ reg, int H, int W, int RW, size_t stride, int bg,
                                                                int oy, int ox, int cell, int gx, int n_xc, long long units,
                                                                const ay_stain_params* __restrict__ params, int stain, int thres_bin,
                                                                unsigned long long* __restrict__ cells) {
    __shared__ float od[256];
    __shared__ int lc[LOAD_WORDS];
    constexpr int BPP = 3 * SHRINK;                          // source bytes of one row per image pixel
    constexpr int PPI = LOAD_ITEM / BPP;                     // pixels of an item
    const int tid = threadIdx.x;
    od[tid] = params->od[tid];
    const float d0 = params->D[stain], d1 = params->D[3 + stain], d2 = params->D[6 + stain];   // uniform: scalar registers
    for (int i = tid; i < LOAD_WORDS; i += 256) lc[i] = 0;
    __syncthreads();
    const unsigned row_bytes = (unsigned)RW * 3, used = (unsigned)W * BPP;   // bytes of a source row; those that belong to a pixel
    const unsigned nq = (used + LOAD_ITEM - 1) / LOAD_ITEM;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {   // u is workgroup-uniform: so are the barriers of the flush
        const unsigned q0 = (unsigned)(u % n_xc) * LOAD_XQ, wq = min((unsigned)LOAD_XQ, nq - q0);
        const int y_lo = (int)(u / n_xc) * LOAD_BAND, y_hi = min(y_lo + LOAD_BAND, H);
        // the unit's cells: rows cy0 .. cy0 + ncy - 1 (ncy <= 2: a band of 16 rows, cell >= 16), columns cx0 .. cx0 + ncx - 1
        const int cy0 = (oy + y_lo) / cell, ncy = (oy + y_hi - 1) / cell - cy0 + 1;
        const int y_cut = (cy0 + 1) * cell - oy;             // region rows from y_cut on lie in cell row cy0 + 1
        const int cx0 = (ox + (int)q0 * PPI) / cell, ncx = (ox + min((int)(q0 + wq) * PPI, W) - 1) / cell - cx0 + 1;
        const unsigned items = (unsigned)(y_hi - y_lo) * wq;
        for (unsigned i = tid; i < items; i += 256) {
            const unsigned qi = i % wq, o = (q0 + qi) * LOAD_ITEM;
            const int Y = y_lo + (int)(i / wq);
            uint32_t w0[12], w1[12];
            if (SHRINK == 1) {
                load48<WIDE>(reg + (size_t)Y * stride, o, row_bytes, w0);
            } else {
                load48<WIDE>(reg + (size_t)(2 * Y) * stride, o, row_bytes, w0);
                load48<WIDE>(reg + (size_t)(2 * Y + 1) * stride, o, row_bytes, w1);
            }
            const int X0 = ox + (int)(q0 + qi) * PPI;        // the item's first pixel on the slide
            const int ca = X0 / cell, xb = (ca + 1) * cell - X0;   // pixels p >= xb of the item lie in cell ca + 1; xb >= 1
            unsigned tm = 0, pm = 0;                         // bit p: pixel p is tissue; is positive
            int qs = 0, qa = 0;                              // bins of the positive pixels: all; those before xb
#pragma unroll
            for (int p = 0; p < PPI; ++p) {                  // the pixels of the item lie at the same bytes in every lane
                const int j = p * BPP;
                if (o + j >= used) continue;                 // behind the last pixel of the row
                int b[3];
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    b[c] = SHRINK == 1 ? byte_of(w0, j + c)
                                       : (byte_of(w0, j + c) + byte_of(w0, j + 3 + c) + byte_of(w1, j + c) + byte_of(w1, j + 3 + c) + 2) >> 2;
                if (min(min(b[0], b[1]), b[2]) >= bg) continue;  // THE TISSUE RULE: most of a slide is glass
                tm |= 1u << p;
                const int bin = load_bin(od, b, d0, d1, d2);
                if (bin >= thres_bin) {
                    pm |= 1u << p;
                    qs += bin;
                    if (p < xb) qa += bin;
                }
            }
            if (tm) {
                const unsigned low = xb >= PPI ? 0xffffu : (1u << xb) - 1u;
                int* a = lc + ((Y >= y_cut ? LOAD_CX : 0) + (ca - cx0)) * 3;
                const int ta = __builtin_popcount(tm & low), tb = __builtin_popcount(tm & ~low);
                if (ta) {
                    atomicAdd(a, ta);
                    const int pa = __builtin_popcount(pm & low);
                    if (pa) atomicAdd(a + 1, pa), atomicAdd(a + 2, qa);
                }
                if (tb) {                                    // a pixel of the image behind xb: cell ca + 1 is one of the unit's
                    atomicAdd(a + 3, tb);
                    const int pb = __builtin_popcount(pm & ~low);
                    if (pb) atomicAdd(a + 4, pb), atomicAdd(a + 5, qs - qa);
                }
            }
        }
        __syncthreads();
        const int per_row = ncx * 3, n = ncy * per_row;
        for (int k = tid; k < n; k += 256) {
            const int r = k >= per_row ? 1 : 0, at = k - r * per_row;
            int* s = lc + r * (LOAD_CX * 3) + at;
            const int v = *s;
            if (v) {
                atomicAdd(cells + ((size_t)(cy0 + r) * gx + cx0) * 3 + at, (unsigned long long)v);
                *s = 0;
            }
        }
        __syncthreads();
    }
}

// load_finite and load_edge, THE LOAD RULE's box ownership: ay_box.h (the focus pass owns the same pixels)

__global__ void __launch_bounds__(256) stain_load_boxes_kernel(const uint8_t* __restrict__ reg, int H, int W, size_t stride, int shrink, int bg,
                                                                int oy, int ox, int slide_h, int slide_w,
                                                                const ay_stain_params* __restrict__ params, int stain, int thres_bin,
                                                                const float* __restrict__ rows, int M, unsigned long long* __restrict__ boxes,
                                                                int32_t* __restrict__ flags) {
    __shared__ float od[256];
    const int tid = threadIdx.x, lane = tid & 63;
    od[tid] = params->od[tid];
    const float d0 = params->D[stain], d1 = params->D[3 + stain], d2 = params->D[6 + stain];
    __syncthreads();
    const long long n_waves = (long long)gridDim.x * 4;
    for (long long m = (long long)blockIdx.x * 4 + (tid >> 6); m < M; m += n_waves) {   // m is uniform over the wavefront
        const float* r = rows + (size_t)m * 7;
        const float x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
        if (!(load_finite(x1) && load_finite(y1) && load_finite(x2) && load_finite(y2))) {
            if (lane == 0) atomicOr(flags, AY_LOAD_FLAG_NONFINITE);
            continue;
        }
        const int lo_x = load_edge(x1, slide_w), hi_x = load_edge(x2, slide_w);
        const int lo_y = load_edge(y1, slide_h), hi_y = load_edge(y2, slide_h);
        // the box's pixels inside this strip, in pixels of the region
        const int ax = max(lo_x, ox) - ox, bx = min(hi_x, ox + W) - ox, ay_ = max(lo_y, oy) - oy, by = min(hi_y, oy + H) - oy;
        if (ax >= bx || ay_ >= by) continue;                 // empty, inverted, or not on this strip
        const int w = bx - ax, h = by - ay_;
        const int dy = 64 / w, dx = 64 % w;                  // a lane's step of 64 pixels, in rows and columns
        int x = lane % w, y = lane / w;
        unsigned long long t = 0, p = 0, s = 0;              // 64-bit per lane: a box may be the whole slide
        while (y < h) {
            int b[3];
            region_tap_u8(reg, stride, shrink, H, W, (unsigned)(ax + x), (unsigned)(ay_ + y), b);   // inside: ax + x < W, ay_ + y < H
            if (min(min(b[0], b[1]), b[2]) < bg) {
                ++t;
                const int bin = load_bin(od, b, d0, d1, d2);
                if (bin >= thres_bin) ++p, s += (unsigned)bin;
            }
            x += dx, y += dy;
            if (x >= w) x -= w, ++y;
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            t += __shfl_down(t, d, 64);
            p += __shfl_down(p, d, 64);
            s += __shfl_down(s, d, 64);
        }
        if (lane == 0) {
            unsigned long long* o = boxes + (size_t)m * 4;
            atomicAdd(o, (unsigned long long)w * (unsigned long long)h);
            if (t) atomicAdd(o + 1, t);
            if (p) atomicAdd(o + 2, p), atomicAdd(o + 3, s);
        }
    }
}

}  // namespace ay

extern "C" int ay_stain_load_u8(const void* region_hwc_u8, int region_h, int region_w, size_t row_stride_bytes, int shrink, int origin_y,
                                int origin_x, int slide_h, int slide_w, int bg_level, const ay_stain_params* params_device, int stain,
                                int thres_bin, int cell, uint64_t* cells, const float* rows, int n_rows, uint64_t* boxes, int32_t* flags,
                                ay_stream_t stream) {
    using namespace ay;
    AY_CHECK_ARG(region_hwc_u8 && params_device, "ay_stain_load_u8: null");
    AY_CHECK_ARG(region_h > 0 && region_w > 0 && region_w <= (1 << 30) / 3 && row_stride_bytes >= (size_t)region_w * 3 &&
                     (shrink == 1 || shrink == 2),
                 "ay_stain_load_u8: region %dx%d stride %zu shrink %d", region_h, region_w, row_stride_bytes, shrink);
    AY_CHECK_ARG(bg_level >= 0 && bg_level <= 256 && (stain == 0 || stain == 1) && thres_bin >= 0 && thres_bin <= AY_STAIN_BINS &&
                     cell >= AY_LOAD_MIN_CELL,
                 "ay_stain_load_u8: bg_level %d, stain %d, thres_bin %d, cell %d", bg_level, stain, thres_bin, cell);
    const int H = region_h / shrink, W = region_w / shrink;
    AY_CHECK_ARG(slide_h >= 1 && slide_h <= LOAD_MAX_SIDE && slide_w >= 1 && slide_w <= LOAD_MAX_SIDE && origin_y >= 0 && origin_x >= 0 &&
                     origin_y <= slide_h - H && origin_x <= slide_w - W,
                 "ay_stain_load_u8: a %dx%d image at (%d, %d) of a %dx%d slide", H, W, origin_y, origin_x, slide_h, slide_w);
    AY_CHECK_ARG(n_rows >= 0 && (n_rows == 0 || (rows && boxes && flags)) && ((uintptr_t)cells & 7) == 0 && ((uintptr_t)boxes & 7) == 0,
                 "ay_stain_load_u8: %d rows %p, boxes %p, flags %p, cells %p", n_rows, (const void*)rows, (void*)boxes, (void*)flags,
                 (void*)cells);
    if (H == 0 || W == 0) return AY_OK;   // a one-pixel region has no halved image
    if (cells) {
        const int gx = (slide_w + cell - 1) / cell;           // before the clamp: the caller's grid
        if (cell > LOAD_MAX_SIDE) cell = LOAD_MAX_SIDE;       // one cell either way, and (c + 1) * cell stays an int
        const unsigned nq = ((unsigned)W * 3 * shrink + LOAD_ITEM - 1) / LOAD_ITEM;
        const int n_xc = (int)((nq + LOAD_XQ - 1) / LOAD_XQ);
        const long long units = (long long)((H + LOAD_BAND - 1) / LOAD_BAND) * n_xc;
        const unsigned blocks = (unsigned)(units > 256 * 8 ? 256 * 8 : units);
        const bool wide = ((uintptr_t)region_hwc_u8 & 15) == 0 && row_stride_bytes % 16 == 0;
#define AY_LOAD_LAUNCH(WIDE, SHRINK)                                                                                                    \
    hipLaunchKernelGGL((stain_load_cells_kernel<WIDE, SHRINK>), dim3(blocks), dim3(256), 0, S(stream), (const uint8_t*)region_hwc_u8, H, W, \
                       region_w, row_stride_bytes, bg_level, origin_y, origin_x, cell, gx, n_xc, units, params_device, stain, thres_bin,    \
                       (unsigned long long*)cells)
        if (wide && shrink == 1) AY_LOAD_LAUNCH(true, 1);
        else if (wide) AY_LOAD_LAUNCH(true, 2);
        else if (shrink == 1) AY_LOAD_LAUNCH(false, 1);
        else AY_LOAD_LAUNCH(false, 2);
#undef AY_LOAD_LAUNCH
        AY_CHECK_LAUNCH("stain_load_cells_kernel");
    }
    if (n_rows) {
        const int want = (n_rows + 3) / 4;
        hipLaunchKernelGGL(stain_load_boxes_kernel, dim3((unsigned)(want > 256 * 8 ? 256 * 8 : want)), dim3(256), 0, S(stream),
                           (const uint8_t*)region_hwc_u8, H, W, row_stride_bytes, shrink, bg_level, origin_y, origin_x, slide_h, slide_w,
                           params_device, stain, thres_bin, rows, n_rows, (unsigned long long*)boxes, flags);
        AY_CHECK_LAUNCH("stain_load_boxes_kernel");
    }
    return AY_OK;
}
