// What the slide-level passes over a resident uint8 HWC region share (ay_stain.hip, ay_stain_basis.hip, ay_load.hip, ay_focus.hip; of ay_tissue.hip the
// launcher and check_region; of ay_segment.hip tissue_px, load_bin, check_region and the box edges): the 48-byte item of the read
// stream, the work units, the walk over a unit's tissue pixels, the flush of a workgroup's LDS histogram, the launch of the four (WIDE,
// SHRINK) instances, the place of an item and a unit on the cell grid, the flush of a workgroup's cell table, the box walk and the host
// checks.  Helper functions only: what a pass does with a pixel and how it accumulates (int32 table, uint64 table with spills, LDS
// bins, registers) is its own and stays in its file.
#pragma once
#include <type_traits>

#include "ay_box.h"
#include "ay_common.h"

namespace ay {

// ---- the item: 48 consecutive bytes of a row, 16 whole pixels (8 of the halved image, with the same bytes of the next row), so that
// pixel p of the item sits at the same bytes in every lane: an unrolled pixel loop extracts at constant positions
constexpr int SLIDE_ITEM = 48;
constexpr int SLIDE_MAX_SIDE = 1 << 24;   // H, W of a slide: (float)W is exact (THE LOAD RULE)

// byte j of a row segment held in dwords
__device__ __forceinline__ int byte_of(const uint32_t* w, int j) { return (int)((w[j >> 2] >> (8 * (j & 3))) & 0xffu); }

// bytes [o, o + 48) of one row into w[0..11]; bytes at or behind row_bytes read as 0 (they are never part of a counted pixel)
template <bool WIDE>
__device__ __forceinline__ void load48(const uint8_t* __restrict__ row, unsigned o, unsigned row_bytes, uint32_t w[12]) {
    if (WIDE && o + 48 <= row_bytes) {   // row and o are multiples of 16
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const u32x4 a = *(const u32x4*)(row + o + 16 * k);
            w[4 * k] = a[0], w[4 * k + 1] = a[1], w[4 * k + 2] = a[2], w[4 * k + 3] = a[3];
        }
    } else {
#pragma unroll
        for (int d = 0; d < 12; ++d) {
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

// the item at byte o of row Y of the (halved) image: its source row into w0, for SHRINK == 2 its two source rows into w0 and w1
template <bool WIDE, int SHRINK>
__device__ __forceinline__ void item_load(const uint8_t* __restrict__ reg, size_t stride, int Y, unsigned o, unsigned row_bytes,
                                          uint32_t w0[12], uint32_t w1[12]) {
    load48<WIDE>(reg + (size_t)(SHRINK * Y) * stride, o, row_bytes, w0);
    if (SHRINK == 2) load48<WIDE>(reg + (size_t)(2 * Y + 1) * stride, o, row_bytes, w1);
}

// the three bytes of pixel p of the item (SHRINK == 2: the 2x2 round-half-up means)
template <int SHRINK>
__device__ __forceinline__ void item_pixel(const uint32_t* w0, const uint32_t* w1, int p, int b[3]) {
    const int j = p * 3 * SHRINK;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        b[c] = SHRINK == 1 ? byte_of(w0, j + c)
                           : (byte_of(w0, j + c) + byte_of(w0, j + 3 + c) + byte_of(w1, j + c) + byte_of(w1, j + 3 + c) + 2) >> 2;
}

// THE TISSUE RULE: most of a slide is glass
__device__ __forceinline__ bool tissue_px(const int b[3], int bg) { return min(min(b[0], b[1]), b[2]) < bg; }

// THE STAIN RULE's bin of the chosen stain's concentration (THE LOAD RULE and THE SEGMENT RULE: ay_load.hip, ay_segment.hip)
__device__ __forceinline__ int load_bin(const float* od, const int b[3], float d0, float d1, float d2) {
    const float c = (od[b[0]] * d0 + od[b[1]] * d1) + od[b[2]] * d2;
    return c < 0.0f ? 0 : (c < 8.0f ? (int)(c * 64.0f) : AY_STAIN_BINS - 1);
}

// ---- the work units: a band of BAND rows x up to XQ items of a row; workgroups of 256 take units grid-stride
struct SlideUnits { unsigned nq; int n_xc; long long units; unsigned blocks; };   // items of a row, units across a row, units, workgroups
static inline SlideUnits slide_units(int W, int shrink, int rows, int BAND, int XQ) {
    const unsigned nq = ((unsigned)W * 3 * shrink + SLIDE_ITEM - 1) / SLIDE_ITEM;
    const int n_xc = (int)((nq + XQ - 1) / XQ);
    const long long units = (long long)((rows + BAND - 1) / BAND) * n_xc;
    return {nq, n_xc, units, (unsigned)(units > 256 * 8 ? 256 * 8 : units)};
}
// items q0 .. q0 + wq - 1 of the rows y_lo .. y_hi - 1, ny of them: a kernel reads y_hi or ny, not both, and pays for no subtraction
struct SlideUnit { unsigned q0, wq; int y_lo, y_hi, ny; };
template <int BAND, int XQ>
__device__ __forceinline__ SlideUnit slide_unit(long long u, int n_xc, unsigned nq, int y0, int y1) {   // unit u of the rows y0 .. y1 - 1
    SlideUnit s;
    s.q0 = (unsigned)(u % n_xc) * XQ, s.wq = min((unsigned)XQ, nq - s.q0);
    s.y_lo = y0 + (int)(u / n_xc) * BAND, s.y_hi = min(s.y_lo + BAND, y1), s.ny = min(BAND, y1 - s.y_lo);
    return s;
}

// ---- the tissue-pixel walk of the read stream: the items of unit `un`, one per lane and step.  item(q, Y) once the item q of row Y is
// loaded, before its first pixel; tissue(p, b) for every pixel p of the item that is tissue, b its three bytes (glass and what lies behind
// the last pixel of the row cost a minimum and a compare); item_done() behind the item's last pixel.
template <bool WIDE, int SHRINK, typename Item, typename Tissue, typename ItemDone>
__device__ __forceinline__ void tissue_walk(const uint8_t* __restrict__ reg, size_t stride, unsigned row_bytes, unsigned used,
                                            const SlideUnit& un, int bg, Item item, Tissue tissue, ItemDone item_done) {
    constexpr int BPP = 3 * SHRINK;                          // source bytes of one row per image pixel
    const unsigned items = (unsigned)(un.y_hi - un.y_lo) * un.wq;
    for (unsigned i = threadIdx.x; i < items; i += 256) {
        const unsigned q = un.q0 + i % un.wq, o = q * SLIDE_ITEM;
        const int Y = un.y_lo + (int)(i / un.wq);
        uint32_t w0[12], w1[12];
        item_load<WIDE, SHRINK>(reg, stride, Y, o, row_bytes, w0, w1);
        item(q, Y);
#pragma unroll
        for (int p = 0; p < SLIDE_ITEM / BPP; ++p) {         // the pixels of the item lie at the same bytes in every lane
            if (o + p * BPP >= used) continue;               // behind the last pixel of the row
            int b[3];
            item_pixel<SHRINK>(w0, w1, p, b);
            if (!tissue_px(b, bg)) continue;
            tissue(p, b);
        }
        item_done();
    }
}

// ---- the LDS histogram of the passes that count tissue pixels in int32 bins (ay_stain.hip, ay_stain_basis.hip): units of 16 rows x
// up to 2048 items; a workgroup's bins go to memory when it is done, and every HIST_FLUSH units before that
constexpr int HIST_BAND = 16;      // rows of a work unit
constexpr int HIST_XQ = 2048;      // items of a row in a work unit
constexpr int HIST_FLUSH = 2048;   // units between two flushes of a workgroup: 2048 * 16 * 2048 * 16 pixels = 1.07e9 < 2^31

// The lane's count joins word `total` of the workgroup's `words` LDS words lh; then every word that is not 0 goes to the 64-bit
// histogram in memory with one integer atomic and is zeroed.  It holds two barriers: every lane of the workgroup calls it, or none.
__device__ __forceinline__ void flush_lds_hist(int* lh, int words, int total, int& cnt, unsigned long long* __restrict__ hist) {
    if (cnt) atomicAdd(&lh[total], cnt);
    cnt = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < words; i += 256) {
        const int v = lh[i];
        if (v) {
            atomicAdd(hist + i, (unsigned long long)v);
            lh[i] = 0;
        }
    }
    __syncthreads();
}

// ---- the launch: launch(wide, shrink) launches the kernel's <wide.value, shrink.value> instance; 16-byte loads when base and stride allow
template <typename Launch>
static inline void launch_wide_shrink(const void* region, size_t row_stride_bytes, int shrink, Launch launch) {
    const bool wide = ((uintptr_t)region & 15) == 0 && row_stride_bytes % 16 == 0;
    const std::integral_constant<int, 1> one;
    const std::integral_constant<int, 2> two;
    if (wide && shrink == 1) launch(std::true_type{}, one);
    else if (wide) launch(std::true_type{}, two);
    else if (shrink == 1) launch(std::false_type{}, one);
    else launch(std::false_type{}, two);
}

// ---- the cell grid.  cell >= 16 (AY_LOAD_MIN_CELL, AY_FOCUS_MIN_CELL) and an item holds at most 16 pixels: at most ONE cell boundary
// falls inside an item, so its pixels lie in cell ca and, from pixel xb >= 1 on, in cell ca + 1 (low: bit p is set iff pixel p lies in
// ca); likewise a band of B rows lies in at most B / 16 + 1 cell rows and XQ items in at most XQ + 1 cells: the size of a cell table.
struct ItemCells { int ca, xb; unsigned low; };
template <int PPI>
__device__ __forceinline__ ItemCells item_cells(int X0, int cell) {   // X0: the item's first pixel on the slide
    const int ca = X0 / cell, xb = (ca + 1) * cell - X0;
    return {ca, xb, xb >= PPI ? 0xffffu : (1u << xb) - 1u};
}
struct UnitCells { int cy0, ncy, cx0, ncx; };   // cell rows cy0 .. cy0 + ncy - 1, columns cx0 .. cx0 + ncx - 1
// of the unit that holds rows y_lo .. y_hi - 1 and columns x_lo .. x_hi - 1 of the slide
__device__ __forceinline__ UnitCells unit_cells(int y_lo, int y_hi, int x_lo, int x_hi, int cell) {
    const int cy0 = y_lo / cell, cx0 = x_lo / cell;
    return {cy0, (y_hi - 1) / cell - cy0 + 1, cx0, (x_hi - 1) / cell - cx0 + 1};
}

// The used ncy x ncx x 3 part of the workgroup's table lc[cell rows][CX][3] goes to memory: lanes on consecutive words, one 64-bit
// integer atomic per (cell, sum) that is not 0 (never one per pixel or per lane), and the word is zeroed.  The barriers are the caller's.
template <typename T, int CX>
__device__ __forceinline__ void flush_cell_table(T* lc, int ncy, int ncx, int cy0, int cx0, int gx, unsigned long long* __restrict__ cells) {
    const int per_row = ncx * 3, n = ncy * per_row;
    for (int k = threadIdx.x; k < n; k += 256) {
        const int r = k / per_row, at = k - r * per_row;
        T* s = lc + r * (CX * 3) + at;
        const T v = *s;
        if (v) {
            atomicAdd(cells + ((size_t)(cy0 + r) * gx + cx0) * 3 + at, (unsigned long long)v);
            *s = 0;
        }
    }
}

// ---- the box walk: one wavefront per box, boxes grid-stride, box_walk_blocks(M) workgroups of 256.  THE LOAD RULE's box (ay_box.h): a
// row with a coordinate that is not finite sets `flag` in *flags and gets nothing; the others own pixels ax .. bx - 1, ay .. by - 1 of
// the slide.  rect(ax, bx, ay, by) cuts that, in place, to what this call owns, in the coordinates pixel() takes; the lanes walk the
// rectangle, pixel(X, Y, sums) adds one pixel to the lane's N 64-bit sums (a box may be the whole slide), the wavefront reduces them
// and lane 0 calls emit(m, w, h, sums) with the rectangle's size.  Correct for any box; ONE HUGE BOX RUNS ON ONE WAVE.
template <int N, typename Rect, typename Pixel, typename Emit>
__device__ __forceinline__ void box_walk(const float* __restrict__ rows, int M, int slide_h, int slide_w, int32_t* __restrict__ flags,
                                         int flag, Rect rect, Pixel pixel, Emit emit) {
    const int tid = threadIdx.x, lane = tid & 63;
    const long long n_waves = (long long)gridDim.x * 4;
    for (long long m = (long long)blockIdx.x * 4 + (tid >> 6); m < M; m += n_waves) {   // m is uniform over the wavefront
        const float* r = rows + (size_t)m * 7;
        const float x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
        if (!(load_finite(x1) && load_finite(y1) && load_finite(x2) && load_finite(y2))) {
            if (lane == 0) atomicOr(flags, flag);
            continue;
        }
        int ax = load_edge(x1, slide_w), bx = load_edge(x2, slide_w), ay_ = load_edge(y1, slide_h), by = load_edge(y2, slide_h);
        rect(ax, bx, ay_, by);
        if (ax >= bx || ay_ >= by) continue;                 // empty, inverted, or not this call's
        const int w = bx - ax, h = by - ay_;
        const int dy = 64 / w, dx = 64 % w;                  // a lane's step of 64 pixels, in rows and columns
        int x = lane % w, y = lane / w;
        unsigned long long sums[N] = {};
        while (y < h) {
            pixel(ax + x, ay_ + y, sums);
            x += dx, y += dy;
            if (x >= w) x -= w, ++y;
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1)
#pragma unroll
            for (int i = 0; i < N; ++i) sums[i] += __shfl_down(sums[i], d, 64);
        if (lane == 0) emit(m, w, h, sums);
    }
}
static inline unsigned box_walk_blocks(int M) { return (unsigned)((M + 3) / 4 > 256 * 8 ? 256 * 8 : (M + 3) / 4); }

// ---- the host checks of the entry points: false, with the error set, where the arguments are refused
static inline bool check_region(const char* entry, int region_h, int region_w, size_t row_stride_bytes, int shrink, bool bound_w) {
    const bool fits = !bound_w || region_w <= (1 << 30) / 3;
    if (region_h > 0 && region_w > 0 && fits && row_stride_bytes >= (size_t)region_w * 3 && (shrink == 1 || shrink == 2)) return true;
    set_error("%s: region %dx%d stride %zu shrink %d", entry, region_h, region_w, row_stride_bytes, shrink);
    return false;
}
static inline bool check_bg_level(const char* entry, int bg_level) {   // 256: every pixel is tissue
    if (bg_level >= 0 && bg_level <= 256) return true;
    set_error("%s: bg_level %d outside 0 .. 256", entry, bg_level);
    return false;
}
// the H x W image of the region lies at (origin_y, origin_x) of a slide_h x slide_w slide, inside it
static inline bool check_on_slide(const char* entry, int H, int W, int origin_y, int origin_x, int slide_h, int slide_w) {
    if (slide_h >= 1 && slide_h <= SLIDE_MAX_SIDE && slide_w >= 1 && slide_w <= SLIDE_MAX_SIDE && origin_y >= 0 && origin_x >= 0 &&
        origin_y <= slide_h - H && origin_x <= slide_w - W)
        return true;
    set_error("%s: a %dx%d image at (%d, %d) of a %dx%d slide", entry, H, W, origin_y, origin_x, slide_h, slide_w);
    return false;
}
static inline bool check_cells_boxes(const char* entry, int n_rows, const float* rows, const void* boxes, const int32_t* flags,
                                     const void* cells) {
    if (n_rows >= 0 && (n_rows == 0 || (rows && boxes && flags)) && ((uintptr_t)cells & 7) == 0 && ((uintptr_t)boxes & 7) == 0) return true;
    set_error("%s: %d rows %p, boxes %p, flags %p, cells %p", entry, n_rows, (const void*)rows, boxes, (const void*)flags, cells);
    return false;
}

}  // namespace ay
