// Focus map (wsi.focus_map, wsi.quantify_region(focus=True); THE FOCUS RULE is stated in include/amyloid_yolo.h and restated in NumPy by
// tests/focus_reference.py): n, the sum and the sum of squares of the 4-neighbour Laplacian of the luma over the EVALUATED pixels, per
// cell of the burden grid and per detection box, out of a resident strip of the slide.  The first kernels here whose result at a pixel
// depends on the rows above and below it: a call is told which centre rows it OWNS and needs one more row on either side resident.
//
//   focus_cells_kernel   the hot path: a read stream over the image in ay_slide_pass.h's 48-byte items (16 whole pixels of a row, 8 of the
//                        halved image; 16-byte or byte loads).  A work unit is a band of up to 32 centre rows x up to 32
//                        items.  Phase A: every row of the band plus one halo row above and below goes through LDS once, a luma byte per
//                        pixel and a tissue bit per pixel (one 16-bit mask per item); the pixel left of the unit's first item and the one
//                        right of its last are tapped with byte loads into a spare item slot on either side, so that an item's neighbour
//                        items and the unit's halo columns are read the same way and no seam exists between items or between units.  A
//                        pixel outside the image is NOT TISSUE whatever bg_level is: columns 0 and W - 1 drop out by the rule itself.
//                        Phase B: a lane takes item column tid % 32 of every 8th centre row: its item's 16 lumas in one 16-byte LDS
//                        read (lanes on consecutive 16 bytes: no bank conflict), the rows above and below likewise, the two side lumas as
//                        bytes, five masks; the evaluated pixels of the item are one AND of shifted masks, and an item without one costs
//                        nothing more.
//   ACCUMULATION         s2 is accumulated in 64 bits everywhere a workgroup or the device sums.  A lane keeps n, s1, s2 of the pixels
//                        left and right of the one cell boundary its item can hold (cell >= 16) in int32 registers over its at most 4
//                        rows of the unit (|lap| <= 1020: s2 <= 4 * 16 * 1 040 400 = 66 585 600 < 2^31) and adds them, whenever the cell
//                        row changes and at the end of the unit, to the workgroup's table in LDS, uint64 [3 cell rows][33 cells][3]
//                        (64-bit LDS atomics; s1 in two's complement), which therefore cannot overflow for any unit size.  After
//                        every unit the used part of the table goes to memory and is zeroed (flush_cell_table, ay_slide_pass.h).  The
//                        sums in memory are bounded by the rule's H * W < 2^43.
//   focus_boxes_kernel   a gather: ay_slide_pass.h's box_walk, one wavefront per box.  THE LOAD RULE's box (ay_box.h), intersected with
//                        the owned rows and with columns 1 .. W - 2 first (most boxes miss the strip), the lanes over the pixels of the
//                        intersection, five byte taps per tissue pixel (region_tap_u8), 64-bit sums per lane, a wave reduction and at
//                        most three 64-bit atomics per box and call.
//
// Integers and order-free integer atomics only: the same bytes every run.  Kernel launches only: no allocation, no memset node, no
// host read, no scratch.
#include "ay_slide_pass.h"

namespace ay {

constexpr int FOCUS_BAND = 32;    // centre rows of a work unit
constexpr int FOCUS_XQ = 32;      // items of a row in a work unit: 512 pixels, 256 of the halved image
constexpr int FOCUS_ROWS = FOCUS_BAND + 2;
constexpr int FOCUS_RSTEP = 256 / FOCUS_XQ;   // a lane's rows are this far apart
// cells a unit can lie in: its <= 512 pixels start r < cell pixels into a cell, (r + 511) / cell + 1 <= 33; 32 rows likewise in <= 3
constexpr int FOCUS_CX = FOCUS_XQ * 16 / AY_FOCUS_MIN_CELL + 1;
constexpr int FOCUS_CY = FOCUS_BAND / AY_FOCUS_MIN_CELL + 1;
constexpr int FOCUS_WORDS = FOCUS_CY * FOCUS_CX * 3;
static_assert((FOCUS_BAND / FOCUS_RSTEP) * 16 * 1020 * 1020 < (1ll << 31), "a lane's int32 s2");

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// THE FOCUS RULE's luma
__device__ __forceinline__ int focus_luma(const int b[3]) { return (77 * b[0] + 150 * b[1] + 29 * b[2] + 128) >> 8; }

template <int N>
__device__ __forceinline__ void lds_get(const uint8_t* p, uint32_t w[N]) {   // N dwords at a 4 * N-byte aligned LDS address
    if constexpr (N == 4) {
        const u32x4 a = *(const u32x4*)p;
        w[0] = a[0], w[1] = a[1], w[2] = a[2], w[3] = a[3];
    } else {
        const u32x2 a = *(const u32x2*)p;
        w[0] = a[0], w[1] = a[1];
    }
}

template <bool WIDE, int SHRINK>
__global__ void __launch_bounds__(256) focus_cells_kernel(const uint8_t* __restrict__ reg, int h_img, int W, int RW, size_t stride, int bg,
                                                           int oy, int c0, int c1, int cell, int gx, int n_xc, long long units,
                                                           unsigned long long* __restrict__ cells) {
    constexpr int BPP = 3 * SHRINK;                          // source bytes of one row per image pixel
    constexpr int PPI = SLIDE_ITEM / BPP;                    // pixels of an item: 16 or 8
    constexpr int GW = PPI / 4;                              // dwords of an item's lumas
    constexpr int LS = PPI * (FOCUS_XQ + 2);                 // bytes of a row of lumas: a spare item slot on either side
    constexpr int TS = FOCUS_XQ + 2;
    __shared__ __attribute__((aligned(16))) uint8_t lum[FOCUS_ROWS * LS];
    __shared__ uint16_t tm[FOCUS_ROWS * TS];                 // bit p: pixel p of the item is tissue
    __shared__ unsigned long long lc[FOCUS_WORDS];
    const int tid = threadIdx.x, qi = tid % FOCUS_XQ, r0 = tid / FOCUS_XQ;
    for (int i = tid; i < FOCUS_WORDS; i += 256) lc[i] = 0;
    const unsigned row_bytes = (unsigned)RW * 3, nq = ((unsigned)W * BPP + SLIDE_ITEM - 1) / SLIDE_ITEM;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {   // u is workgroup-uniform: so are the barriers
        const auto [q0, wq, yb, y_end, nc] = slide_unit<FOCUS_BAND, FOCUS_XQ>(u, n_xc, nq, c0, c1);
        // ---- phase A: the unit's centre rows are yb .. yb + nc - 1 of the slide; rows yb - 1 .. yb + nc -> LDS rows 0 .. nc + 1
        if ((unsigned)qi < wq) {
            const unsigned o = (q0 + qi) * SLIDE_ITEM;
            const int X0 = (int)(q0 + qi) * PPI;
            for (int r = r0; r < nc + 2; r += FOCUS_RSTEP) {
                const int y = yb - 1 + r - oy;               // row of the (halved) image the region holds: 0 <= y < h_img (host check)
                uint32_t w0[12], w1[12];
                item_load<WIDE, SHRINK>(reg, stride, y, o, row_bytes, w0, w1);
                uint32_t g[GW] = {};
                unsigned t = 0;
#pragma unroll
                for (int p = 0; p < PPI; ++p) {              // the pixels of the item lie at the same bytes in every lane
                    int b[3];
                    item_pixel<SHRINK>(w0, w1, p, b);
                    g[p >> 2] |= (uint32_t)focus_luma(b) << (8 * (p & 3));
                    if (X0 + p < W && tissue_px(b, bg)) t |= 1u << p;   // behind the row's last pixel: not tissue
                }
                uint8_t* d = lum + r * LS + PPI * (1 + qi);
                if constexpr (GW == 4) *(u32x4*)d = u32x4{g[0], g[1], g[2], g[3]};
                else *(u32x2*)d = u32x2{g[0], g[1]};
                tm[r * TS + 1 + qi] = (uint16_t)t;
            }
        }
        for (int i = tid; i < (nc + 2) * 2; i += 256) {      // the pixel left of the unit and the pixel right of it, of every row
            const int r = i >> 1, right = i & 1;
            const unsigned X = right ? (q0 + wq) * PPI : q0 * PPI - 1u;   // q0 == 0: wraps, outside
            int b[3] = {255, 255, 255};
            const bool in = region_tap_u8(reg, stride, SHRINK, h_img, W, X, (unsigned)(yb - 1 + r - oy), b);
            const bool t = in && tissue_px(b, bg);
            lum[r * LS + (right ? PPI * (1 + (int)wq) : PPI - 1)] = (uint8_t)focus_luma(b);
            tm[r * TS + (right ? 1 + (int)wq : 0)] = (uint16_t)(t ? (right ? 1u : 1u << (PPI - 1)) : 0u);
        }
        __syncthreads();
        // ---- phase B: the unit's cells are rows cy0 .. cy0 + ncy - 1 (ncy <= 3), columns cx0 .. cx0 + ncx - 1
        const UnitCells uc = unit_cells(yb, yb + nc, (int)(q0 * PPI), min((int)(q0 + wq) * PPI, W), cell);
        const int cut1 = (uc.cy0 + 1) * cell, cut2 = cut1 + cell;   // slide rows from cut1 (cut2) on lie in cell row cy0 + 1 (+ 2); < 2^26
        if ((unsigned)qi < wq) {
            const ItemCells ic = item_cells<PPI>((int)(q0 + qi) * PPI, cell);
            int na = 0, nb = 0, s1 = 0, s1a = 0, s2 = 0, s2a = 0, cur = 0;   // n left / right of xb; sums: all, left of xb
            auto spill = [&]() {
                unsigned long long* a = lc + (cur * FOCUS_CX + (ic.ca - uc.cx0)) * 3;
                if (na) {
                    atomicAdd(a, (unsigned long long)na);
                    atomicAdd(a + 1, (unsigned long long)(long long)s1a);
                    atomicAdd(a + 2, (unsigned long long)s2a);
                }
                if (nb) {                                    // an evaluated pixel behind xb: cell ca + 1 is one of the unit's
                    atomicAdd(a + 3, (unsigned long long)nb);
                    atomicAdd(a + 4, (unsigned long long)(long long)(s1 - s1a));
                    atomicAdd(a + 5, (unsigned long long)(s2 - s2a));
                }
                na = nb = s1 = s1a = s2 = s2a = 0;
            };
            for (int r = r0; r < nc; r += FOCUS_RSTEP) {
                const int Y = yb + r, cyr = (Y >= cut1) + (Y >= cut2);
                if (cyr != cur) {
                    spill();
                    cur = cyr;
                }
                const uint16_t* tr = tm + (r + 1) * TS + 1 + qi;
                const unsigned t = tr[0];
                const unsigned ev = t & tr[-TS] & tr[TS] & ((t << 1) | (tr[-1] >> (PPI - 1))) & ((t >> 1) | ((tr[1] & 1u) << (PPI - 1)));
                if (!ev) continue;                           // glass, or tissue without a whole neighbourhood
                const uint8_t* lr = lum + (r + 1) * LS + PPI * (1 + qi);
                uint32_t c[GW], up[GW], dn[GW];
                lds_get<GW>(lr, c);
                lds_get<GW>(lr - LS, up);
                lds_get<GW>(lr + LS, dn);
                const int left = lr[-1], right = lr[PPI];
#pragma unroll
                for (int p = 0; p < PPI; ++p) {
                    const int gl = p ? byte_of(c, p - 1) : left, gr = p < PPI - 1 ? byte_of(c, p + 1) : right;
                    int lap = 4 * byte_of(c, p) - gl - gr - byte_of(up, p) - byte_of(dn, p);
                    lap = (ev >> p) & 1u ? lap : 0;
                    const int sq = lap * lap;
                    s1 += lap, s2 += sq;
                    if (p < ic.xb) s1a += lap, s2a += sq;
                }
                na += __builtin_popcount(ev & ic.low), nb += __builtin_popcount(ev & ~ic.low);
            }
            spill();
        }
        __syncthreads();
        // the flush; the next unit's phase A writes lum and tm only, and its barrier stands before the next add to lc
        flush_cell_table<unsigned long long, FOCUS_CX>(lc, uc.ncy, uc.ncx, uc.cy0, uc.cx0, gx, cells);
    }
}

__global__ void __launch_bounds__(256) focus_boxes_kernel(const uint8_t* __restrict__ reg, int h_img, int W, size_t stride, int shrink, int bg,
                                                           int oy, int slide_h, int c0, int c1, const float* __restrict__ rows, int M,
                                                           unsigned long long* __restrict__ boxes, int32_t* __restrict__ flags) {
    box_walk<3>(
        rows, M, slide_h, W, flags, AY_FOCUS_FLAG_NONFINITE,
        // the box's pixels that this call owns and that can be evaluated: rows c0 .. c1 - 1, columns 1 .. W - 2 of the slide
        [&](int& ax, int& bx, int& ay_, int& by) { ax = max(ax, 1), bx = min(bx, W - 1), ay_ = max(ay_, c0), by = min(by, c1); },
        [&](int x, int y, unsigned long long* s) {           // n, s1 in two's complement, s2
            const unsigned X = (unsigned)x, Y = (unsigned)(y - oy);   // Y: row of the region's image; Y - 1 .. Y + 1 resident
            int b[3] = {255, 255, 255};
            int g[5];
            bool ok = true;
#pragma unroll
            for (int k = 0; k < 5 && ok; ++k) {              // the centre first: most pixels of a slide are glass
                const unsigned tx = k == 1 ? X - 1 : k == 2 ? X + 1 : X, ty = k == 3 ? Y - 1 : k == 4 ? Y + 1 : Y;
                ok = region_tap_u8(reg, stride, shrink, h_img, W, tx, ty, b) && tissue_px(b, bg);
                g[k] = focus_luma(b);
            }
            if (ok) {
                const int lap = 4 * g[0] - g[1] - g[2] - g[3] - g[4];
                ++s[0], s[1] += (unsigned long long)(long long)lap, s[2] += (unsigned long long)(lap * lap);
            }
        },
        [&](long long m, int, int, const unsigned long long* s) {
            if (!s[0]) return;
            unsigned long long* o = boxes + (size_t)m * 3;
            atomicAdd(o, s[0]);
            if (s[1]) atomicAdd(o + 1, s[1]);
            if (s[2]) atomicAdd(o + 2, s[2]);
        });
}

}  // namespace ay

extern "C" int ay_focus_u8(const void* region_hwc_u8, int region_h, int region_w, size_t row_stride_bytes, int shrink, int origin_y,
                           int slide_h, int slide_w, int own_y0, int own_y1, int bg_level, int cell, int64_t* cells, const float* rows,
                           int n_rows, int64_t* boxes, int32_t* flags, ay_stream_t stream) {
    using namespace ay;
    AY_CHECK_ARG(region_hwc_u8, "ay_focus_u8: null");
    if (!check_region("ay_focus_u8", region_h, region_w, row_stride_bytes, shrink, true)) return AY_ERR_ARG;
    if (!check_bg_level("ay_focus_u8", bg_level)) return AY_ERR_ARG;
    AY_CHECK_ARG(cell >= AY_FOCUS_MIN_CELL, "ay_focus_u8: cell %d", cell);
    const int h_img = region_h / shrink, W = region_w / shrink;
    if (!check_on_slide("ay_focus_u8", h_img, W, origin_y, 0, slide_h, slide_w)) return AY_ERR_ARG;
    AY_CHECK_ARG((long long)slide_h * slide_w < (1ll << 43) && W == slide_w,
                 "ay_focus_u8: a %dx%d image of a %dx%d slide (the region holds whole rows of the slide)", h_img, W, slide_h, slide_w);
    AY_CHECK_ARG(own_y0 >= 0 && own_y0 <= own_y1 && own_y1 <= slide_h, "ay_focus_u8: owned rows %d .. %d of %d", own_y0, own_y1, slide_h);
    if (!check_cells_boxes("ay_focus_u8", n_rows, rows, boxes, flags, cells)) return AY_ERR_ARG;
    const int c0 = own_y0 > 1 ? own_y0 : 1, c1 = own_y1 < slide_h - 1 ? own_y1 : slide_h - 1;   // the centre rows: c0 <= Y < c1
    const bool some = c0 < c1 && W >= 3;
    AY_CHECK_ARG(!some || (c0 - 1 >= origin_y && c1 <= origin_y + h_img - 1),
                 "ay_focus_u8: rows %d .. %d are needed, the region holds %d .. %d", c0 - 1, c1, origin_y, origin_y + h_img - 1);
    if (!some) return AY_OK;                                  // no pixel to evaluate: nothing is launched, added or flagged
    if (cells) {
        const int gx = (slide_w + cell - 1) / cell;           // before the clamp: the caller's grid
        if (cell > SLIDE_MAX_SIDE) cell = SLIDE_MAX_SIDE;     // one cell either way, and (c + 1) * cell stays an int
        const SlideUnits g = slide_units(W, shrink, c1 - c0, FOCUS_BAND, FOCUS_XQ);
        launch_wide_shrink(region_hwc_u8, row_stride_bytes, shrink, [&](auto wide, auto sh) {
            hipLaunchKernelGGL((focus_cells_kernel<wide.value, sh.value>), dim3(g.blocks), dim3(256), 0, S(stream),
                               (const uint8_t*)region_hwc_u8, h_img, W, region_w, row_stride_bytes, bg_level, origin_y, c0, c1, cell, gx,
                               g.n_xc, g.units, (unsigned long long*)cells);
        });
        AY_CHECK_LAUNCH("focus_cells_kernel");
    }
    if (n_rows) {
        hipLaunchKernelGGL(focus_boxes_kernel, dim3(box_walk_blocks(n_rows)), dim3(256), 0, S(stream), (const uint8_t*)region_hwc_u8, h_img,
                           W, row_stride_bytes, shrink, bg_level, origin_y, slide_h, c0, c1, rows, n_rows, (unsigned long long*)boxes, flags);
        AY_CHECK_LAUNCH("focus_boxes_kernel");
    }
    return AY_OK;
}
