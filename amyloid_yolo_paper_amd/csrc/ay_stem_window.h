// The image window of the stem kernels: how stem_s2_fused_v2_kernel (ay_stem_fused.hip), stem_train_fwd_kernel and
// stem_train_wgrad_kernel (ay_stem_train.hip) read the fp32 NCHW image, and where a stem pixel's 27 taps sit in it.
//   * an item's window is IH rows x 3 channels x IW = 72 columns of floats in LDS, stored [row][channel][column].  It arrives by 16-byte
//     buffer DMA (dma16_buf: one wave instruction per 64 pieces, 11 per tile of the fused stem instead of 35 of 4 bytes) and starts 4
//     columns left of the tile, so that every piece is 16-byte aligned in HBM (needs W % 4 == 0: stem_window_ok).  A lane whose
//     piece lies outside the image hands the offset OOB, beyond the descriptor's range, and reads zeros = the convolution's padding
//   * item coordinates come from one multiply-high division per item (stem_item_tile), computed when its tile is issued and kept in a
//     register queue for the later iterations that use them
//   * the 27 taps of a stem pixel are a 9 x 3 grid (rho = 3 kh + ci, kw) in the window, and the K = 32 slots of the reduction over
//     taps are ORDERED so that the 8 taps of lane half 1 are those of half 0 moved down 3 (K-step 0) or 2 (K-step 1) grid rows: every
//     LDS read of the stem is one per-lane base + an immediate; the 5 spare slots carry zero filters and re-read taps of the same or
//     the next pixel row (finite whenever the image is), which is why a window has one row more than its pixels use
//   * filters in slot order: slot s of an output channel takes its filter value tap_kref(slot_tap(s)) if slot_live(s), else zero
// A kernel keeps its own loop over pieces, LDS destinations, scratch line and counted waits.  Where a kernel writes one of these rules
// out itself, the function here changed its instruction stream (profiles/stem_window_codegen.txt) and a comment there names the rule.
#pragma once
#include "ay_conv_common.h"

namespace ay {

struct StemWindowBase {
    static constexpr int IW = 72;                  // columns (tile origin - 4) .. + 67
    static constexpr int ROW_PIECES = IW / 4;      // 16-byte pieces per row
    static constexpr unsigned OOB = 0x80000000u;   // beyond the range of any descriptor stem_window_ok admits
};
// ROWS = the rows the tile's pixels use + 1 that only zero-filter slots read
template <int ROWS>
struct StemWindow : StemWindowBase {
    static constexpr int IH = ROWS;
    static constexpr int IMG_PIECES = IH * 3 * ROW_PIECES;    // [row][channel][column piece]
    static constexpr int IMG_DMAS = (IMG_PIECES + 63) / 64;   // wave-wide DMA instructions per window
    static constexpr int IMG_BYTES = IMG_DMAS * 1024;
};
static_assert(StemWindow<12>::IMG_PIECES == 648 && StemWindow<12>::IMG_DMAS == 11, "fused stem: 12 rows");
static_assert(StemWindow<11>::IMG_PIECES == 594 && StemWindow<11>::IMG_DMAS == 10, "training stem: 11 rows");

// float offset in the window of the tap-grid origin of the pixel in window row `row`, tile column `col`; xoff = window column of the
// leftmost image column that tile column 0 reads
__host__ __device__ constexpr int stem_pixel_off(int row, int col, int xoff) { return row * 3 * StemWindowBase::IW + col + xoff; }

// K slots (forward: the MFMA's K; weight gradient: its N): slot = step*16 + half*8 + e holds grid tap t = rho*3 + kw
__host__ __device__ constexpr int slot_tap(int slot) {
    const int step = slot >> 4, half = (slot >> 3) & 1, e = slot & 7;
    if (step == 0) return e + 9 * half;                                   // rows 0,1,(2,0),(2,1) | rows 3,4,(5,0),(5,1)
    const int c = e < 6 ? 18 + e : (e == 6 ? 8 : 17);                     // rows 6,7,(2,2),(5,2)
    return half ? c + 6 : c;                                              // | row 8, row 9 (spare), (4,2) (spare), (7,2) (spare)
}
__host__ __device__ constexpr bool slot_live(int slot) {
    const int step = slot >> 4, half = (slot >> 3) & 1;
    return !(step == 1 && half == 1) || slot_tap(slot) / 3 == 8;
}
__host__ __device__ constexpr int tap_goff(int t) { return (t / 3) * StemWindowBase::IW + t % 3; }     // float offset of grid tap t from the pixel
__host__ __device__ constexpr int tap_kref(int t) { return ((t / 3) % 3) * 9 + (t / 9) * 3 + t % 3; }  // its filter index ci*9 + kh*3 + kw

constexpr bool stem_slots_cover_filter() {
    for (int k = 0; k < 27; ++k) {
        int hits = 0;
        for (int s = 0; s < 32; ++s) hits += slot_live(s) && tap_kref(slot_tap(s)) == k;
        if (hits != 1) return false;
    }
    return true;
}
constexpr int stem_dead_slots() {
    int n = 0;
    for (int s = 0; s < 32; ++s) n += !slot_live(s);
    return n;
}
constexpr bool stem_half1_is_half0_moved_down() {
    for (int e = 0; e < 8; ++e)
        if (tap_goff(slot_tap(8 + e)) != tap_goff(slot_tap(e)) + 3 * StemWindowBase::IW ||
            tap_goff(slot_tap(24 + e)) != tap_goff(slot_tap(16 + e)) + 2 * StemWindowBase::IW)
            return false;
    return true;
}
constexpr bool stem_slots_within_spare_row() {   // grid row 9 of a tile's last pixel row is channel 0 of the window's spare row
    for (int s = 0; s < 32; ++s)
        if (slot_tap(s) < 0 || slot_tap(s) / 3 > 9) return false;
    return true;
}
static_assert(stem_slots_cover_filter(), "the live slots hit every filter index ci*9 + kh*3 + kw in 0..26 exactly once");
static_assert(stem_dead_slots() == 5, "exactly five slots are dead");
static_assert(stem_half1_is_half0_moved_down(), "half 1 = half 0 + 3 IW (step 0) / + 2 IW (step 1): pbase0 / pbase1 of the kernels");
static_assert(stem_slots_within_spare_row(), "no slot, live or dead, reads beyond grid row 9: IH = used rows + 1");

// item -> image, tile row, tile column: two multiply-high divisions (m_tx, m_tpi: mulhi_divisor), one correction each
struct StemTile {
    int b, ty, tx;
};
__device__ __forceinline__ StemTile stem_item_tile(unsigned it, unsigned tiles_x, unsigned tiles_per_img, unsigned m_tx, unsigned m_tpi) {
    unsigned b = __umulhi(it, m_tpi), r = it - b * tiles_per_img;
    if (r >= tiles_per_img) ++b, r -= tiles_per_img;
    unsigned ty = __umulhi(r, m_tx), tx = r - ty * tiles_x;
    if (tx >= tiles_x) ++ty, tx -= tiles_x;
    return StemTile{(int)b, (int)ty, (int)tx};
}

// piece 64*dma + lane of wave instruction `dma`: does it exist, its window row, the first of its 4 columns, its float offset from the
// window origin's pixel in channel 0
struct StemPiece {
    bool have;
    int row, col, gofs;
};
template <typename WIN>
__device__ __forceinline__ StemPiece stem_piece(int dma, int lane, int plane_elems, int W) {
    const int pu = dma * 64 + lane;
    StemPiece p;
    p.have = dma < WIN::IMG_DMAS && pu < WIN::IMG_PIECES;
    p.col = (pu % WIN::ROW_PIECES) * 4;
    const int ci = (pu / WIN::ROW_PIECES) % 3;
    p.row = pu / (WIN::ROW_PIECES * 3);
    p.gofs = ci * plane_elems + p.row * W + p.col;
    return p;
}
// the byte offset the lane hands to dma16_buf for the window whose origin is image pixel (ybase, xbase)
__device__ __forceinline__ unsigned stem_piece_voff(const StemPiece& p, int ybase, int xbase, int H, int W) {
    const bool ok = p.have && (unsigned)(ybase + p.row) < (unsigned)H && (unsigned)(xbase + p.col) < (unsigned)W;
    return ok ? (unsigned)((p.gofs + ybase * W + xbase) * 4) : StemWindowBase::OOB;
}

// one block of 32 pixels x 32 filters: wa = the filters in slot order, p0 / p1 = the lane's pixel in the window (stem_pixel_off), moved
// down for lane half 1 by the 3 / 2 grid rows of K-step 0 / 1
template <typename DT>
__device__ __forceinline__ f32x16 stem_pixel_mfma(const float* p0, const float* p1, const typename DT::vec8 (&wa)[2]) {
    typedef typename DT::vec8 vec8;
    f32x2 v0[4], v1[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        v0[jj] = f32x2{p0[tap_goff(slot_tap(2 * jj))], p0[tap_goff(slot_tap(2 * jj + 1))]};
        v1[jj] = f32x2{p1[tap_goff(slot_tap(16 + 2 * jj))], p1[tap_goff(slot_tap(16 + 2 * jj + 1))]};
    }
    const uint4 b0 = make_uint4(DT::pack2(v0[0]), DT::pack2(v0[1]), DT::pack2(v0[2]), DT::pack2(v0[3]));
    const uint4 b1 = make_uint4(DT::pack2(v1[0]), DT::pack2(v1[1]), DT::pack2(v1[2]), DT::pack2(v1[3]));
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    acc = DT::mfma32(wa[0], __builtin_bit_cast(vec8, b0), acc);
    acc = DT::mfma32(wa[1], __builtin_bit_cast(vec8, b1), acc);
    return acc;
}

// host: can this image take the window (pieces aligned in HBM, every byte offset below OOB)?
inline bool stem_window_ok(const float* x, int h, int w) {
    return w % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && 3LL * h * w * 4 < 0x7fffffffLL;
}

}  // namespace ay
