// Tile ingest on the device: uint8 HWC RGB tiles -> the float32 CHW tensor the network takes, with the
// reference's preprocessing fused into one pass:
//   ToTensor            x / 255                                      (utils/transforms.py:96, torchvision ToTensor)
//   pad_to_square       centre zero padding, short side             (utils/datasets.py:22-32; PadSquare transforms.py:83-90)
//   resize              F.interpolate(mode="nearest"): src = min(floor(dst * (float)in / out), in - 1)   (utils/datasets.py:35-37)
// so the host uploads 3 bytes per pixel instead of 12 and never touches the pixels again.
#include "ay_common.h"

namespace ay {

__global__ void __launch_bounds__(256) ingest_u8_kernel(const uint8_t* __restrict__ img, int B, int H, int W, int S, float pad_value,
                                                         float* __restrict__ out) {
    const int D = H > W ? H : W;               // side of the padded square
    const int top = H <= W ? (W - H) / 2 : 0;  // pad1 = diff // 2 goes first (top / left)
    const int left = H > W ? (H - W) / 2 : 0;
    const float scale = (float)D / (float)S;   // ATen's nearest scale for size= (no scale_factor): in / out in fp32
    const size_t plane = (size_t)S * S;
    const size_t total = (size_t)B * plane;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % S), y = (int)((i / S) % S);
        const size_t b = i / plane;
        const int sy = min((int)floorf(y * scale), D - 1) - top;
        const int sx = min((int)floorf(x * scale), D - 1) - left;
        float r = pad_value, g = pad_value, bl = pad_value;
        if (sy >= 0 && sy < H && sx >= 0 && sx < W) {
            const uint8_t* p = img + ((b * H + sy) * (size_t)W + sx) * 3;
            r = (float)p[0] / 255.0f;
            g = (float)p[1] / 255.0f;
            bl = (float)p[2] / 255.0f;
        }
        float* o = out + b * 3 * plane + (size_t)y * S + x;
        o[0] = r;
        o[plane] = g;
        o[2 * plane] = bl;
    }
}

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

template <int V, typename Origins>
__global__ void __launch_bounds__(256) region_tiles_cut_u8_kernel(const uint8_t* __restrict__ reg, int RH, int RW, size_t stride, int shrink,
                                                                   int tile, Origins origins, size_t n, int S, float* __restrict__ out) {
    typedef float vec __attribute__((ext_vector_type(V)));
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
            region_tap(reg, stride, shrink, H, W, ox + (unsigned)min((int)floorf((x0 + k) * scale), tile - 1), Y, px);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][k] = px[c];
        }
        float* o = out + t * 3 * plane + (size_t)y * S + x0;
#pragma unroll
        for (int c = 0; c < 3; ++c) *(vec*)(o + c * plane) = v[c];
    }
}

// the launch of the three region entry points: 16-byte stores where every row of every plane starts on 16 bytes, scalar ones otherwise
template <typename Origins>
static int launch_cut(const void* reg, int RH, int RW, size_t stride, int shrink, int tile, Origins origins, size_t n, int out_size,
                      float* out, ay_stream_t stream) {
    const bool vec4 = out_size % 4 == 0 && ((uintptr_t)out & 15) == 0;
    const size_t total = n * out_size * (out_size / (vec4 ? 4 : 1));
    size_t blocks = (total + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    if (vec4)
        hipLaunchKernelGGL((region_tiles_cut_u8_kernel<4, Origins>), dim3((unsigned)blocks), dim3(256), 0, S(stream), (const uint8_t*)reg, RH,
                           RW, stride, shrink, tile, origins, n, out_size, out);
    else
        hipLaunchKernelGGL((region_tiles_cut_u8_kernel<1, Origins>), dim3((unsigned)blocks), dim3(256), 0, S(stream), (const uint8_t*)reg, RH,
                           RW, stride, shrink, tile, origins, n, out_size, out);
    AY_CHECK_LAUNCH("region_tiles_cut_u8_kernel");
    return AY_OK;
}

}  // namespace ay

extern "C" int ay_ingest_region_tiles_list_u8(const void* region_hwc_u8, int region_h, int region_w, size_t row_stride_bytes, int shrink,
                                              int tile, const int32_t* origins_xy, int n, int out_size, float* out_nchw,
                                              ay_stream_t stream) {
    using namespace ay;
    AY_CHECK_ARG(region_hwc_u8 && out_nchw && origins_xy, "ay_ingest_region_tiles_list_u8: null");
    AY_CHECK_ARG(region_h > 0 && region_w > 0 && row_stride_bytes >= (size_t)region_w * 3 && (shrink == 1 || shrink == 2),
                 "ay_ingest_region_tiles_list_u8: region %dx%d stride %zu shrink %d", region_h, region_w, row_stride_bytes, shrink);
    AY_CHECK_ARG(tile > 0 && tile <= (1 << 24) && n > 0 && out_size > 0, "ay_ingest_region_tiles_list_u8: %d tiles of %d -> %d", n, tile,
                 out_size);
    return launch_cut(region_hwc_u8, region_h, region_w, row_stride_bytes, shrink, tile, ListOrigins{origins_xy}, (size_t)n, out_size,
                      out_nchw, stream);
}

extern "C" int ay_ingest_region_tiles_u8(const void* region_hwc_u8, int region_h, int region_w, size_t row_stride_bytes, int shrink,
                                         int tile, int tiles_y, int tiles_x, int out_size, float* out_nchw, ay_stream_t stream) {
    using namespace ay;
    AY_CHECK_ARG(region_hwc_u8 && out_nchw, "ay_ingest_region_tiles_u8: null");
    AY_CHECK_ARG(region_h > 0 && region_w > 0 && row_stride_bytes >= (size_t)region_w * 3 && (shrink == 1 || shrink == 2),
                 "ay_ingest_region_tiles_u8: region %dx%d stride %zu shrink %d", region_h, region_w, row_stride_bytes, shrink);
    AY_CHECK_ARG(tile > 0 && tiles_y > 0 && tiles_x > 0 && out_size > 0, "ay_ingest_region_tiles_u8: tile grid %dx%d of %d -> %d",
                 tiles_y, tiles_x, tile, out_size);
    return launch_cut(region_hwc_u8, region_h, region_w, row_stride_bytes, shrink, tile, GridOrigins{tiles_x, tile},
                      (size_t)tiles_y * tiles_x, out_size, out_nchw, stream);
}

extern "C" int ay_ingest_region_tiles_step_u8(const void* region_hwc_u8, int region_h, int region_w, size_t row_stride_bytes, int shrink,
                                              int tile, int step, int tiles_y, int tiles_x, int out_size, float* out_nchw,
                                              ay_stream_t stream) {
    using namespace ay;
    AY_CHECK_ARG(region_hwc_u8 && out_nchw, "ay_ingest_region_tiles_step_u8: null");
    AY_CHECK_ARG(region_h > 0 && region_w > 0 && row_stride_bytes >= (size_t)region_w * 3 && (shrink == 1 || shrink == 2),
                 "ay_ingest_region_tiles_step_u8: region %dx%d stride %zu shrink %d", region_h, region_w, row_stride_bytes, shrink);
    AY_CHECK_ARG(tile > 0 && step > 0 && step <= tile && tiles_y > 0 && tiles_x > 0 && out_size > 0,
                 "ay_ingest_region_tiles_step_u8: tile grid %dx%d of %d step %d -> %d", tiles_y, tiles_x, tile, step, out_size);
    return launch_cut(region_hwc_u8, region_h, region_w, row_stride_bytes, shrink, tile, GridOrigins{tiles_x, step},
                      (size_t)tiles_y * tiles_x, out_size, out_nchw, stream);
}

extern "C" int ay_ingest_tiles_u8(const void* img_hwc_u8, int batch, int h, int w, int out_size, float pad_value, float* out_nchw,
                                  ay_stream_t stream) {
    using namespace ay;
    AY_CHECK_ARG(img_hwc_u8 && out_nchw, "ay_ingest_tiles_u8: null");
    AY_CHECK_ARG(batch > 0 && h > 0 && w > 0 && out_size > 0, "ay_ingest_tiles_u8: bad shape %dx%dx%d -> %d", batch, h, w, out_size);
    const size_t total = (size_t)batch * out_size * out_size;
    size_t blocks = (total + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    hipLaunchKernelGGL(ingest_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, S(stream), (const uint8_t*)img_hwc_u8, batch, h, w, out_size,
                       pad_value, out_nchw);
    AY_CHECK_LAUNCH("ingest_u8_kernel");
    return AY_OK;
}
