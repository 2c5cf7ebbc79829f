// The whole-slide cut kernels, shared by ay_ingest.hip (the grid, step and list entry points), ay_views.hip (the views entry point)
// and ay_stain.hip (the same kernels with the stain colour stage): each file instantiates the colour stages it launches.
#pragma once
#include "ay_common.h"

namespace ay {

// WSI -> tile streaming (crop.py:13-25,44-47): the tiles dzsave(layout='google', tile_size=1536) cuts out of a
// slide -- edge tiles padded to the full size with the background 255 -- taken straight out of a resident uint8 HWC region
// (a full-width strip of the slide: one contiguous upload), optionally after the 40x -> 20x halving, then the N1 chain
// (/255, nearest resize to the network size).  The halving is a 2x2 mean with round-half-up in uint8: pyvips' resize(0.5) is a
// lanczos3 reduce and the reference then goes through JPEG Q=90, neither is restated (parity unpinned).
//
// ONE cut for every region entry point.  Tile t has its origin at Origins::at(t) on the (halved) slide and a side of `tile`; a thread
// produces V consecutive output pixels of one row (region_tap of ay_common.h per pixel) and stores them as one V-float vector per
// channel plane: the kernel is bound by its 12 B of stores per output pixel, and a 16-byte store per lane moves them in a quarter of
// the store instructions of the scalar form.
struct GridOrigins {   // tile (ty, tx) of a tiles_x-wide grid starts at (tx * step, ty * step); step == tile: dzsave's abutting grid
    int tiles_x, step;
    __device__ __forceinline__ void at(size_t t, unsigned& x, unsigned& y) const {
        x = (unsigned)(t % tiles_x) * (unsigned)step;
        y = (unsigned)(t / tiles_x) * (unsigned)step;
    }
};
struct ListOrigins {   // tile t starts at xy[t] = (x, y), any int32 pair (wsi.RegionTileStream(tile_mask=...): only the wanted tiles)
    const int32_t* __restrict__ xy;
    __device__ __forceinline__ void at(size_t t, unsigned& x, unsigned& y) const {
        x = (unsigned)xy[2 * t];
        y = (unsigned)xy[2 * t + 1];
    }
};

// The colour stage (ay_common.h) turns the tap's bytes into the stored value: PlainColour (byte / 255) for the ingest entry points,
// StainColour (THE STAIN RULE) for ay_ingest_region_tiles_stain_u8.
template <int V, typename Origins, typename Colour>
__global__ void __launch_bounds__(256) region_tiles_cut_u8_kernel(const uint8_t* __restrict__ reg, int RH, int RW, size_t stride, int shrink,
                                                                   int tile, Origins origins, size_t n, int S, Colour colour,
                                                                   float* __restrict__ out) {
    typedef float vec __attribute__((ext_vector_type(V)));
    __shared__ typename Colour::Tables tab;
    colour.load(tab);
    const int H = RH / shrink, W = RW / shrink;  // the (halved) image the tiles lie on
    const float scale = (float)tile / (float)S;
    const size_t plane = (size_t)S * S;
    const int SV = S / V;   // S % V == 0 (launch_cut)
    const size_t total = n * S * SV;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x0 = (int)(i % SV) * V, y = (int)((i / SV) % S);
        const size_t t = i / ((size_t)SV * S);
        unsigned ox, oy;
        origins.at(t, ox, oy);
        const unsigned Y = oy + (unsigned)min((int)floorf(y * scale), tile - 1);
        vec v[3];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            float px[3];
            region_tap(colour, tab, reg, stride, shrink, H, W, ox + (unsigned)min((int)floorf((x0 + k) * scale), tile - 1), Y, px);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][k] = px[c];
        }
        float* o = out + t * 3 * plane + (size_t)y * S + x0;
#pragma unroll
        for (int c = 0; c < 3; ++c) *(vec*)(o + c * plane) = v[c];
    }
}

// the launch of the region entry points: 16-byte stores where every row of every plane starts on 16 bytes, scalar ones otherwise
template <typename Origins, typename Colour = PlainColour>
static int launch_cut(const void* reg, int RH, int RW, size_t stride, int shrink, int tile, Origins origins, size_t n, int out_size,
                      float* out, ay_stream_t stream, Colour colour = Colour{}) {
    const bool vec4 = out_size % 4 == 0 && ((uintptr_t)out & 15) == 0;
    const size_t total = n * out_size * (out_size / (vec4 ? 4 : 1));
    size_t blocks = (total + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    if (vec4)
        hipLaunchKernelGGL((region_tiles_cut_u8_kernel<4, Origins, Colour>), dim3((unsigned)blocks), dim3(256), 0, S(stream), (const uint8_t*)reg, RH,
                           RW, stride, shrink, tile, origins, n, out_size, colour, out);
    else
        hipLaunchKernelGGL((region_tiles_cut_u8_kernel<1, Origins, Colour>), dim3((unsigned)blocks), dim3(256), 0, S(stream), (const uint8_t*)reg, RH,
                           RW, stride, shrink, tile, origins, n, out_size, colour, out);
    AY_CHECK_LAUNCH("region_tiles_cut_u8_kernel");
    return AY_OK;
}

// ---- the cut in dihedral views (THE VIEW RULE; the kernel is described at the top of ay_views.hip) ----
constexpr int VIEW_BLOCK = 32;   // side of the block of I0 a workgroup holds
constexpr int VIEW_PITCH = 33;   // floats between its rows in LDS

struct ViewList {
    int n;
    int v[8];
};

// 1 <= n_views <= 8, distinct ids in 0 .. 7
static bool take_views(const int* views, int n_views, ViewList* out) {
    if (!views || n_views < 1 || n_views > 8) return false;
    unsigned seen = 0;
    out->n = n_views;
    for (int i = 0; i < 8; ++i) out->v[i] = 0;
    for (int i = 0; i < n_views; ++i) {
        const int v = views[i];
        if (v < 0 || v > 7 || (seen >> v & 1u)) return false;
        seen |= 1u << v;
        out->v[i] = v;
    }
    return true;
}

template <int V, typename Colour>
__global__ void __launch_bounds__(256) region_tiles_views_u8_kernel(const uint8_t* __restrict__ reg, int RH, int RW, size_t stride, int shrink,
                                                                     int tile, const int32_t* __restrict__ origins, int n, ViewList views,
                                                                     int S, Colour colour, float* __restrict__ out) {
    typedef float vec __attribute__((ext_vector_type(V)));
    __shared__ float blk[3][VIEW_BLOCK][VIEW_PITCH];
    __shared__ typename Colour::Tables tab;   // the colour stage of the cut (ay_common.h): nothing for PlainColour
    colour.load(tab);
    const int H = RH / shrink, W = RW / shrink;
    const float scale = (float)tile / (float)S;
    const size_t plane = (size_t)S * S;
    const int nb = (S + VIEW_BLOCK - 1) / VIEW_BLOCK;
    const size_t per_tile = (size_t)nb * nb;
    const size_t total = (size_t)n * per_tile;
    const int tid = threadIdx.x;
    for (size_t b = blockIdx.x; b < total; b += gridDim.x) {   // the same trip count for the whole workgroup: the barriers are safe
        const size_t t = b / per_tile;
        const int rem = (int)(b % per_tile);
        const int r0 = (rem / nb) * VIEW_BLOCK, c0 = (rem % nb) * VIEW_BLOCK;      // the block of I0: rows r0 .., columns c0 ..
        const int h = min(VIEW_BLOCK, S - r0), w = min(VIEW_BLOCK, S - c0);
        const unsigned ox = (unsigned)origins[2 * t], oy = (unsigned)origins[2 * t + 1];
        // ---- I0: the tap of the cut kernel (region_tap, ay_common.h) ----
        for (int i = tid; i < VIEW_BLOCK * VIEW_BLOCK; i += 256) {
            const int ly = i >> 5, lx = i & 31;
            if (ly >= h || lx >= w) continue;
            float px[3];
            region_tap(colour, tab, reg, stride, shrink, H, W, ox + (unsigned)min((int)floorf((c0 + lx) * scale), tile - 1),
                       oy + (unsigned)min((int)floorf((r0 + ly) * scale), tile - 1), px);
#pragma unroll
            for (int c = 0; c < 3; ++c) blk[c][ly][lx] = px[c];
        }
        __syncthreads();
        // ---- the block in every view: a rows x cols rectangle at (Y0, X0), lanes along its rows ----
        for (int vi = 0; vi < views.n; ++vi) {
            const int v = views.v[vi];
            const bool FX = v & 1, FY = (v >> 1) & 1, T = (v >> 2) & 1;
            const int xs = FX ? S - (c0 + w) : c0;      // where the block's columns / rows land along the axis they map to
            const int ys = FY ? S - (r0 + h) : r0;
            const int rows = T ? w : h, cols = T ? h : w;
            const int Y0 = T ? xs : ys, X0 = T ? ys : xs;
            float* o = out + ((t * views.n + vi) * 3) * plane + (size_t)Y0 * S + X0;
            constexpr int QPR = VIEW_BLOCK / V;                      // lane groups per row
            constexpr int ITEMS = 3 * VIEW_BLOCK * QPR;
#pragma unroll 1
            for (int item = tid; item < ITEMS; item += 256) {
                const int xo = (item % QPR) * V, ro = (item / QPR) % VIEW_BLOCK, c = item / (QPR * VIEW_BLOCK);
                if (ro >= rows || xo >= cols) continue;              // cols % V == 0 (V == 4 only when S % 4 == 0)
                vec val;
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const int a = T ? ro : xo + k, bb = T ? xo + k : ro;   // (a, b) of the rule, relative to the rectangle
                    const int lx = FX ? w - 1 - a : a, ly = FY ? h - 1 - bb : bb;
                    val[k] = blk[c][ly][lx];
                }
                *(vec*)(o + c * plane + (size_t)ro * S + xo) = val;
            }
        }
        __syncthreads();
    }
}

// the launch of the views cut behind the entry points' argument checks
template <typename Colour>
static int launch_views(const void* reg, int RH, int RW, size_t stride, int shrink, int tile, const int32_t* origins_xy, int n,
                        const int* views, int n_views, int out_size, float* out, ay_stream_t stream, Colour colour, const char* who) {
    ViewList vl;
    AY_CHECK_ARG(take_views(views, n_views, &vl), "%s: need 1 .. 8 distinct view ids in 0 .. 7 (n_views %d)", who, n_views);
    const bool vec4 = out_size % 4 == 0 && ((uintptr_t)out & 15) == 0;   // every row of every plane of every view then starts on 16 bytes
    const size_t nb = (size_t)(out_size + VIEW_BLOCK - 1) / VIEW_BLOCK;
    size_t blocks = (size_t)n * nb * nb;
    if (blocks > (1u << 20)) blocks = 1u << 20;
    if (vec4)
        hipLaunchKernelGGL((region_tiles_views_u8_kernel<4, Colour>), dim3((unsigned)blocks), dim3(256), 0, S(stream), (const uint8_t*)reg, RH,
                           RW, stride, shrink, tile, origins_xy, n, vl, out_size, colour, out);
    else
        hipLaunchKernelGGL((region_tiles_views_u8_kernel<1, Colour>), dim3((unsigned)blocks), dim3(256), 0, S(stream), (const uint8_t*)reg, RH,
                           RW, stride, shrink, tile, origins_xy, n, vl, out_size, colour, out);
    AY_CHECK_LAUNCH("region_tiles_views_u8_kernel");
    return AY_OK;
}

}  // namespace ay
