// Amyloid load (wsi.stain_load, wsi.quantify_region(load=True); THE LOAD RULE is stated in include/amyloid_yolo.h and restated in NumPy
// by tests/load_reference.py): the tissue pixels, the stain-positive pixels and the sum of their bins, per cell of the burden grid and
// per detection box, out of a resident strip of the slide.
//
//   stain_load_cells_kernel   the hot path: a read stream over the IMAGE in ay_slide_pass.h's 48-byte items (16 whole pixels of a row,
//                             8 of the halved image; 16-byte or byte loads), od in LDS, the three D of the ONE chosen stain in scalar
//                             registers, the tissue test before the unmixing.  A work unit is 16 rows x up to 256 items.
//                             AY_LOAD_MIN_CELL = 16 makes an item's 16 pixels lie in at most two cells of a row and a 16-row band in
//                             at most two cell rows: a lane sums its item in registers (two masks, two bin sums), splits them at the
//                             one cell boundary the item can hold and adds what is not 0 to the workgroup's int32 table in LDS, [2 cell
//                             rows][LOAD_CX cells][3]; after every unit the table's used part goes to memory and is zeroed again.
//   stain_load_boxes_kernel   a gather: ay_slide_pass.h's box_walk, one wavefront per box.  THE LOAD RULE's box in four fp32 steps, an
//                             integer intersection with the strip (most boxes miss it), the lanes over the pixels of the intersection
//                             (byte loads: region_tap_u8's), 64-bit sums per lane, a wave reduction and at most four 64-bit atomics
//                             per box and strip.
//
// Integers and order-free integer atomics only: the same bytes every run.  Kernel launches only: no allocation, no memset node, no
// host read, no scratch.
#include "ay_slide_pass.h"

namespace ay {

constexpr int LOAD_BAND = 16;     // rows of a work unit
constexpr int LOAD_XQ = 256;      // items of a row in a work unit: 4096 pixels, 2048 of the halved image
// cells a unit's pixels can lie in, per cell row: its <= 4096 pixels start r < cell pixels into a cell, (r + 4095) / cell + 1 <= 257
constexpr int LOAD_CX = LOAD_XQ * 16 / AY_LOAD_MIN_CELL + 1;
// The int32 table is flushed after EVERY unit: a word holds at most the bins of the unit's 16 * 256 * 16 = 65536 pixels, each at most
// 511: 33 488 896 < 2^31.
constexpr int LOAD_WORDS = 2 * LOAD_CX * 3;

template <bool WIDE, int SHRINK>
__global__ void __launch_bounds__(256) stain_load_cells_kernel(const uint8_t* __restrict__ reg, int H, int W, int RW, size_t stride, int bg,
                                                                int oy, int ox, int cell, int gx, int n_xc, long long units,
                                                                const ay_stain_params* __restrict__ params, int stain, int thres_bin,
                                                                unsigned long long* __restrict__ cells) {
    __shared__ float od[256];
    __shared__ int lc[LOAD_WORDS];
    constexpr int PPI = SLIDE_ITEM / (3 * SHRINK);           // pixels of an item
    const int tid = threadIdx.x;
    od[tid] = params->od[tid];
    const float d0 = params->D[stain], d1 = params->D[3 + stain], d2 = params->D[6 + stain];   // uniform: scalar registers
    for (int i = tid; i < LOAD_WORDS; i += 256) lc[i] = 0;
    __syncthreads();
    const unsigned row_bytes = (unsigned)RW * 3, used = (unsigned)W * (3 * SHRINK);   // bytes of a source row; those that belong to a pixel
    const unsigned nq = (used + SLIDE_ITEM - 1) / SLIDE_ITEM;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {   // u is workgroup-uniform: so are the barriers of the flush
        const SlideUnit un = slide_unit<LOAD_BAND, LOAD_XQ>(u, n_xc, nq, 0, H);
        const UnitCells uc = unit_cells(oy + un.y_lo, oy + un.y_hi, ox + (int)un.q0 * PPI, ox + min((int)(un.q0 + un.wq) * PPI, W), cell);
        const int y_cut = (uc.cy0 + 1) * cell - oy;          // region rows from y_cut on lie in cell row cy0 + 1; ncy <= 2: 16 rows, cell >= 16
        ItemCells ic;
        int row;                                             // of the item
        unsigned tm, pm;                                     // bit p: pixel p is tissue; is positive
        int qs, qa;                                          // bins of the positive pixels: all; those before xb
        tissue_walk<WIDE, SHRINK>(
            reg, stride, row_bytes, used, un, bg,
            [&](unsigned q, int Y) { ic = item_cells<PPI>(ox + (int)q * PPI, cell), row = Y, tm = pm = 0, qs = qa = 0; },
            [&](int p, const int* b) {
                tm |= 1u << p;
                const int bin = load_bin(od, b, d0, d1, d2);
                if (bin >= thres_bin) {
                    pm |= 1u << p;
                    qs += bin;
                    if (p < ic.xb) qa += bin;
                }
            },
            [&]() {
                if (!tm) return;
                int* a = lc + ((row >= y_cut ? LOAD_CX : 0) + (ic.ca - uc.cx0)) * 3;
                const int ta = __builtin_popcount(tm & ic.low), tb = __builtin_popcount(tm & ~ic.low);
                if (ta) {
                    atomicAdd(a, ta);
                    const int pa = __builtin_popcount(pm & ic.low);
                    if (pa) atomicAdd(a + 1, pa), atomicAdd(a + 2, qa);
                }
                if (tb) {                                    // a pixel of the image behind xb: cell ca + 1 is one of the unit's
                    atomicAdd(a + 3, tb);
                    const int pb = __builtin_popcount(pm & ~ic.low);
                    if (pb) atomicAdd(a + 4, pb), atomicAdd(a + 5, qs - qa);
                }
            });
        __syncthreads();
        flush_cell_table<int, LOAD_CX>(lc, uc.ncy, uc.ncx, uc.cy0, uc.cx0, gx, cells);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) stain_load_boxes_kernel(const uint8_t* __restrict__ reg, int H, int W, size_t stride, int shrink, int bg,
                                                                int oy, int ox, int slide_h, int slide_w,
                                                                const ay_stain_params* __restrict__ params, int stain, int thres_bin,
                                                                const float* __restrict__ rows, int M, unsigned long long* __restrict__ boxes,
                                                                int32_t* __restrict__ flags) {
    __shared__ float od[256];
    od[threadIdx.x] = params->od[threadIdx.x];
    const float d0 = params->D[stain], d1 = params->D[3 + stain], d2 = params->D[6 + stain];
    __syncthreads();
    box_walk<3>(
        rows, M, slide_h, slide_w, flags, AY_LOAD_FLAG_NONFINITE,
        [&](int& ax, int& bx, int& ay_, int& by) {           // the box's pixels inside this strip, in pixels of the region
            ax = max(ax, ox) - ox, bx = min(bx, ox + W) - ox, ay_ = max(ay_, oy) - oy, by = min(by, oy + H) - oy;
        },
        [&](int X, int Y, unsigned long long* s) {           // tissue, positive, bin sum
            int b[3];
            region_tap_u8(reg, stride, shrink, H, W, (unsigned)X, (unsigned)Y, b);   // inside: X < W, Y < H
            if (tissue_px(b, bg)) {
                ++s[0];
                const int bin = load_bin(od, b, d0, d1, d2);
                const bool pos = bin >= thres_bin;
                s[1] += pos, s[2] += pos ? (unsigned)bin : 0u;
            }
        },
        [&](long long m, int w, int h, const unsigned long long* s) {
            unsigned long long* o = boxes + (size_t)m * 4;
            atomicAdd(o, (unsigned long long)w * (unsigned long long)h);
            if (s[0]) atomicAdd(o + 1, s[0]);
            if (s[1]) atomicAdd(o + 2, s[1]), atomicAdd(o + 3, s[2]);
        });
}

}  // namespace ay

extern "C" int ay_stain_load_u8(const void* region_hwc_u8, int region_h, int region_w, size_t row_stride_bytes, int shrink, int origin_y,
                                int origin_x, int slide_h, int slide_w, int bg_level, const ay_stain_params* params_device, int stain,
                                int thres_bin, int cell, uint64_t* cells, const float* rows, int n_rows, uint64_t* boxes, int32_t* flags,
                                ay_stream_t stream) {
    using namespace ay;
    AY_CHECK_ARG(region_hwc_u8 && params_device, "ay_stain_load_u8: null");
    if (!check_region("ay_stain_load_u8", region_h, region_w, row_stride_bytes, shrink, true)) return AY_ERR_ARG;
    if (!check_bg_level("ay_stain_load_u8", bg_level)) return AY_ERR_ARG;
    AY_CHECK_ARG((stain == 0 || stain == 1) && thres_bin >= 0 && thres_bin <= AY_STAIN_BINS && cell >= AY_LOAD_MIN_CELL,
                 "ay_stain_load_u8: stain %d, thres_bin %d, cell %d", stain, thres_bin, cell);
    const int H = region_h / shrink, W = region_w / shrink;
    if (!check_on_slide("ay_stain_load_u8", H, W, origin_y, origin_x, slide_h, slide_w)) return AY_ERR_ARG;
    if (!check_cells_boxes("ay_stain_load_u8", n_rows, rows, boxes, flags, cells)) return AY_ERR_ARG;
    if (H == 0 || W == 0) return AY_OK;   // a one-pixel region has no halved image
    if (cells) {
        const int gx = (slide_w + cell - 1) / cell;           // before the clamp: the caller's grid
        if (cell > SLIDE_MAX_SIDE) cell = SLIDE_MAX_SIDE;     // one cell either way, and (c + 1) * cell stays an int
        const SlideUnits g = slide_units(W, shrink, H, LOAD_BAND, LOAD_XQ);
        launch_wide_shrink(region_hwc_u8, row_stride_bytes, shrink, [&](auto wide, auto sh) {
            hipLaunchKernelGGL((stain_load_cells_kernel<wide.value, sh.value>), dim3(g.blocks), dim3(256), 0, S(stream),
                               (const uint8_t*)region_hwc_u8, H, W, region_w, row_stride_bytes, bg_level, origin_y, origin_x, cell, gx,
                               g.n_xc, g.units, params_device, stain, thres_bin, (unsigned long long*)cells);
        });
        AY_CHECK_LAUNCH("stain_load_cells_kernel");
    }
    if (n_rows) {
        hipLaunchKernelGGL(stain_load_boxes_kernel, dim3(box_walk_blocks(n_rows)), dim3(256), 0, S(stream), (const uint8_t*)region_hwc_u8, H,
                           W, row_stride_bytes, shrink, bg_level, origin_y, origin_x, slide_h, slide_w, params_device, stain, thres_bin,
                           rows, n_rows, (unsigned long long*)boxes, flags);
        AY_CHECK_LAUNCH("stain_load_boxes_kernel");
    }
    return AY_OK;
}
