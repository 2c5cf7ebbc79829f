// Training augmentation fused into the tile ingest: uint8 HWC tiles (a ragged batch in one buffer) -> the float32 NCHW batch of the
// training step with flip, rotation / translation (bilinear, zero outside), sharpen, dropout, hue / brightness applied in ONE pass.
// THE AUGMENTATION RULE (include/amyloid_yolo.h) fixes every fp32 operation and its order; tests/augment_reference.py restates it
// in NumPy and the kernel is compared with it bit for bit.  The library is built with -ffp-contract=off: no a * b + c below is fused.
// Nothing random happens here: the per-image records (ay_aug_params) are drawn on the host (amyloid_yolo_paper_amd/augment.py).
// ay_augment_ingest_window_u8 (THE WINDOW RULE, the training windows wsi.SlideSampler cuts out of a slide) is the same kernel with
// another source of the four taps of step 4 (TileTaps / WindowTaps below); everything else is one body.
//
// Shape: a 256-thread workgroup owns a 16 x 64 block of output pixels of one image.  Phase 1 computes the warped value W (steps 1-4
// of the rule) of that block plus a one-pixel halo, clamped at the edge of the output image, into LDS: 18 x 66 pixels x 3 planes of
// fp32.  One barrier.  Phase 2: a lane takes 4 consecutive pixels of a row, reads their 3 x 6 window per plane (one 16-byte and one
// 8-byte LDS read per row), and does sharpen, dropout, colour, clamp and the stores: one 16-byte vector per lane and channel plane.
#include "ay_common.h"

namespace ay {

constexpr int AUG_BH = 16, AUG_BW = 64;          // output pixels of a workgroup
constexpr int AUG_HH = AUG_BH + 2, AUG_HW = AUG_BW + 2;
// Row pitch in floats: a multiple of 4, so that a lane's window starts on 16 bytes.  ds_read_b128 serves 16 lanes per cycle, taken
// from two rows of the block (4 + 4 lanes of one, 8 of the next), over 64 banks: the 32 dwords of the second row start 68 - 64 = 4
// banks behind the gap the first row leaves, so 4 of the 64 banks see two addresses.  The pitch without that overlap is 128, which
// doubles the LDS of a workgroup and halves the workgroups a CU holds during the gather phase; 68 is the smaller cost.
constexpr int AUG_PITCH = 68;

// Where the four taps of step 4 get their values: the one thing in which the tile rule and THE WINDOW RULE differ.  A source is made
// from the record (`init`, false: the record reads nothing) and called with the floored tap position of a pixel.
struct TileTaps {   // THE AUGMENTATION RULE: the image [h][w][3] at src_offset, 0 outside
    typedef ay_aug_params Rec;
    const uint8_t* img;
    int h, w;
    static __device__ __forceinline__ const ay_aug_params& aug(const Rec& P) { return P; }
    // a record that does not lie inside [src, src + src_bytes) reads nothing: its image is all padding
    __device__ __forceinline__ bool init(const Rec& P, const uint8_t* src, size_t src_bytes) {
        h = P.h, w = P.w;
        img = src + P.src_offset;
        return h > 0 && w > 0 && P.src_offset >= 0 && (uint64_t)P.src_offset <= src_bytes &&
               (uint64_t)h * (uint64_t)w * 3 <= src_bytes - (uint64_t)P.src_offset;
    }
    __device__ __forceinline__ void operator()(float x0f, float y0f, float* a, float* b, float* c, float* d) const {
        // what lies further out than one pixel has no tap inside: clamp before the conversion, so that any float (also inf / NaN of a
        // nonsensical record) gives an int the range checks below reject
        const int x0 = (int)fminf(fmaxf(x0f, -2.0f), (float)w), y0 = (int)fminf(fmaxf(y0f, -2.0f), (float)h);
        const bool vx0 = x0 >= 0 && x0 < w, vx1 = x0 + 1 >= 0 && x0 + 1 < w;
        const bool vy0 = y0 >= 0 && y0 < h, vy1 = y0 + 1 >= 0 && y0 + 1 < h;
        // every load goes to an address inside the image (clamped), a tap outside is then replaced by 0: no divergent loads
        const int xa = min(max(x0, 0), w - 1), xb = min(max(x0 + 1, 0), w - 1);
        const int ya = min(max(y0, 0), h - 1), yb = min(max(y0 + 1, 0), h - 1);
        const uint8_t* pa = img + ((size_t)ya * w + xa) * 3;
        const uint8_t* pb = img + ((size_t)ya * w + xb) * 3;
        const uint8_t* pc = img + ((size_t)yb * w + xa) * 3;
        const uint8_t* pd = img + ((size_t)yb * w + xb) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            a[k] = vy0 && vx0 ? (float)pa[k] : 0.0f;
            b[k] = vy0 && vx1 ? (float)pb[k] : 0.0f;
            c[k] = vy1 && vx0 ? (float)pc[k] : 0.0f;
            d[k] = vy1 && vx1 ? (float)pd[k] : 0.0f;
        }
    }
};

__device__ const uint8_t aug_no_pixels[4] = {0, 0, 0, 0};   // what a block without pixels points at: its taps are all outside

struct WindowTaps {   // THE WINDOW RULE: the h x w window at (x0, y0) of a bh x bw block with rows row_stride bytes apart
    typedef ay_aug_window_params Rec;
    const uint8_t* blk;
    size_t stride;
    int h, w, bh, bw, ox, oy;
    bool context;
    float fill;
    static __device__ __forceinline__ const ay_aug_params& aug(const Rec& P) { return P.aug; }
    // the block has to lie inside [src, src + src_bytes): src_offset + (bh - 1) * row_stride + 3 * bw <= src_bytes, term by term so
    // that nothing overflows; a block without pixels (bh <= 0 or bw <= 0) reads nothing and needs no room
    __device__ __forceinline__ bool init(const Rec& P, const uint8_t* src, size_t src_bytes) {
        h = P.aug.h, w = P.aug.w, ox = P.x0, oy = P.y0, context = P.context != 0, fill = P.fill;
        bh = P.bh > 0 && P.bw > 0 ? P.bh : 0;
        bw = P.bh > 0 && P.bw > 0 ? P.bw : 0;
        if (!(h > 0 && w > 0 && P.src_offset >= 0 && P.row_stride >= 0)) return false;
        if (bh == 0) {
            blk = aug_no_pixels, stride = 0;
            return true;
        }
        blk = src + P.src_offset, stride = (size_t)P.row_stride;
        if ((uint64_t)P.src_offset > src_bytes) return false;
        const uint64_t room = src_bytes - (uint64_t)P.src_offset, last = (uint64_t)bw * 3;
        uint64_t rows;
        if (last > room || __builtin_mul_overflow((uint64_t)(bh - 1), (uint64_t)P.row_stride, &rows)) return false;
        return rows <= room - last;
    }
    __device__ __forceinline__ void operator()(float x0f, float y0f, float* a, float* b, float* c, float* d) const {
        // the tap position in window coordinates as an integer no sum with an int32 origin can overflow (beyond +-1e10 there is no
        // block; inf and NaN land there too), then in block coordinates, clamped to what has no tap inside: [-2, bw]
        const long long tx = (long long)fminf(fmaxf(x0f, -1.0e10f), 1.0e10f), ty = (long long)fminf(fmaxf(y0f, -1.0e10f), 1.0e10f);
        const bool wx0 = context || (tx >= 0 && tx < w), wx1 = context || (tx + 1 >= 0 && tx + 1 < w);
        const bool wy0 = context || (ty >= 0 && ty < h), wy1 = context || (ty + 1 >= 0 && ty + 1 < h);
        const int bx = (int)min(max(tx + ox, -2LL), (long long)bw), by = (int)min(max(ty + oy, -2LL), (long long)bh);
        const bool vx0 = bx >= 0 && bx < bw, vx1 = bx + 1 >= 0 && bx + 1 < bw;
        const bool vy0 = by >= 0 && by < bh, vy1 = by + 1 >= 0 && by + 1 < bh;
        // every load goes to an address inside the block (index 0 of aug_no_pixels for a block without pixels)
        const int xa = max(min(bx, bw - 1), 0), xb = max(min(bx + 1, bw - 1), 0);
        const int ya = max(min(by, bh - 1), 0), yb = max(min(by + 1, bh - 1), 0);
        const uint8_t* pa = blk + (size_t)ya * stride + (size_t)xa * 3;
        const uint8_t* pb = blk + (size_t)ya * stride + (size_t)xb * 3;
        const uint8_t* pc = blk + (size_t)yb * stride + (size_t)xa * 3;
        const uint8_t* pd = blk + (size_t)yb * stride + (size_t)xb * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float ra = (float)pa[k], rb = (float)pb[k], rc = (float)pc[k], rd = (float)pd[k];
            a[k] = wy0 && wx0 ? (vy0 && vx0 ? ra : fill) : 0.0f;
            b[k] = wy0 && wx1 ? (vy0 && vx1 ? rb : fill) : 0.0f;
            c[k] = wy1 && wx0 ? (vy1 && vx0 ? rc : fill) : 0.0f;
            d[k] = wy1 && wx1 ? (vy1 && vx1 ? rd : fill) : 0.0f;
        }
    }
};

// steps 1-4 of the rule for output pixel (x, y), 0 <= x, y < S: the three channels of W in 0..255
template <class Taps>
__device__ __forceinline__ void aug_warp(const Taps& taps, int h, int w, int D, int left, int top, float scale, float cx, float cy,
                                         const float* inv, int flip, int x, int y, float* W) {
    int qx = min((int)floorf(x * scale), D - 1) - left;
    const int qy = min((int)floorf(y * scale), D - 1) - top;
    if (flip) qx = w - 1 - qx;
    const float xc = (float)qx - cx, yc = (float)qy - cy;
    const float sx = ((inv[0] * xc + inv[1] * yc) + inv[2]) + cx;
    const float sy = ((inv[3] * xc + inv[4] * yc) + inv[5]) + cy;
    const float x0f = floorf(sx), y0f = floorf(sy);
    const float fx = sx - x0f, fy = sy - y0f;
    float a[3], b[3], c[3], d[3];
    taps(x0f, y0f, a, b, c, d);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float t = a[k] + fx * (b[k] - a[k]);
        const float u = c[k] + fx * (d[k] - c[k]);
        W[k] = t + fy * (u - t);
    }
}

template <bool VEC4, class Taps>
__global__ void __launch_bounds__(256) augment_ingest_u8_kernel(const uint8_t* __restrict__ src, size_t src_bytes,
                                                                 const typename Taps::Rec* __restrict__ params, int S,
                                                                 float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float lds[3][AUG_HH][AUG_PITCH];
    const ay_aug_params& P = Taps::aug(params[blockIdx.z]);   // the same record for the whole workgroup: scalar loads
    const int h = P.h, w = P.w;
    Taps taps;
    const bool ok = taps.init(params[blockIdx.z], src, src_bytes);
    const int bx = blockIdx.x * AUG_BW, by = blockIdx.y * AUG_BH;
    if (ok) {
        const int D = h > w ? h : w;               // the square pixel of ay_ingest_tiles_u8
        const int top = h <= w ? (w - h) / 2 : 0;
        const int left = h > w ? (h - w) / 2 : 0;
        const float scale = (float)D / (float)S;
        const float cx = (float)(w - 1) / 2.0f, cy = (float)(h - 1) / 2.0f;
        float inv[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) inv[k] = P.inv[k];
        const int flip = P.flip;
        for (int i = threadIdx.x; i < AUG_HH * AUG_HW; i += 256) {
            const int hy = i / AUG_HW, hx = i - hy * AUG_HW;
            const int x = min(max(bx + hx - 1, 0), S - 1), y = min(max(by + hy - 1, 0), S - 1);   // the sharpen ring clamps at the edge
            float W[3];
            aug_warp(taps, h, w, D, left, top, scale, cx, cy, inv, flip, x, y, W);
#pragma unroll
            for (int k = 0; k < 3; ++k) lds[k][hy][hx] = W[k];
        }
    } else {
        for (int i = threadIdx.x; i < AUG_HH * AUG_HW; i += 256) {
            const int hy = i / AUG_HW, hx = i - hy * AUG_HW;
#pragma unroll
            for (int k = 0; k < 3; ++k) lds[k][hy][hx] = 0.0f;
        }
    }
    __syncthreads();

    const int ty = threadIdx.x >> 4, tx = (threadIdx.x & 15) * 4;
    const int x = bx + tx, y = by + ty;
    if (y >= S || x >= S) return;
    const float alpha = P.sharpen_alpha, bright = P.bright;
    const uint32_t thr = P.drop_threshold, seed = P.drop_seed;
    float M[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) M[k] = P.color[k];
    float v[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float win[3][6];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const f32x4 a = *(const f32x4*)&lds[c][ty + r][tx];
            const f32x2 b = *(const f32x2*)&lds[c][ty + r][tx + 4];
            win[r][0] = a[0]; win[r][1] = a[1]; win[r][2] = a[2]; win[r][3] = a[3]; win[r][4] = b[0]; win[r][5] = b[1];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float ring = win[0][k];              // rows top to bottom, left to right, centre skipped
            ring = ring + win[0][k + 1];
            ring = ring + win[0][k + 2];
            ring = ring + win[1][k];
            ring = ring + win[1][k + 2];
            ring = ring + win[2][k];
            ring = ring + win[2][k + 1];
            ring = ring + win[2][k + 2];
            const float Wc = win[1][k + 1];
            v[c][k] = Wc + alpha * (8.0f * Wc - ring);
        }
    }
    float o[3][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t hsh = seed ^ (((uint32_t)y * (uint32_t)S + (uint32_t)(x + k)) * 0x9E3779B9u);
        hsh ^= hsh >> 16;
        hsh *= 0x7feb352du;
        hsh ^= hsh >> 15;
        hsh *= 0x846ca68bu;
        hsh ^= hsh >> 16;
        const bool drop = hsh < thr;
        const float r = drop ? 0.0f : v[0][k], g = drop ? 0.0f : v[1][k], b = drop ? 0.0f : v[2][k];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float q = ((M[3 * c] * r + M[3 * c + 1] * g) + M[3 * c + 2] * b) + bright;
            q = q > 0.0f ? q : 0.0f;             // min(max(q, 0), 255); a NaN becomes 0
            q = q < 255.0f ? q : 255.0f;
            o[c][k] = q / 255.0f;
        }
    }
    const size_t plane = (size_t)S * S;
    float* dst = out + (size_t)blockIdx.z * 3 * plane + (size_t)y * S + x;
    if (VEC4) {   // S % 4 == 0 and x % 4 == 0: the four pixels lie inside the row, on 16 bytes
#pragma unroll
        for (int c = 0; c < 3; ++c) *(f32x4*)(dst + c * plane) = f32x4{o[c][0], o[c][1], o[c][2], o[c][3]};
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x + k < S) {
#pragma unroll
                for (int c = 0; c < 3; ++c) dst[c * plane + k] = o[c][k];
            }
    }
}

// the argument checks, the grid and the VEC4 choice of both entry points
template <class Taps>
static int augment_launch(const char* name, const void* src_u8, size_t src_bytes, const typename Taps::Rec* params_device, int batch,
                          int out_size, float* out_nchw, ay_stream_t stream) {
    AY_CHECK_ARG(src_u8 && params_device && out_nchw, "%s: null", name);
    AY_CHECK_ARG(src_bytes > 0 && batch > 0 && batch <= 65535 && out_size > 0 && out_size <= 32768,
                 "%s: %zu source bytes, batch %d (1..65535) -> %d (1..32768)", name, src_bytes, batch, out_size);
    const bool vec4 = out_size % 4 == 0 && ((uintptr_t)out_nchw & 15) == 0;   // every row of every plane then starts on 16 bytes
    const dim3 grid((unsigned)((out_size + AUG_BW - 1) / AUG_BW), (unsigned)((out_size + AUG_BH - 1) / AUG_BH), (unsigned)batch);
    if (vec4)
        hipLaunchKernelGGL((augment_ingest_u8_kernel<true, Taps>), grid, dim3(256), 0, S(stream), (const uint8_t*)src_u8, src_bytes,
                           params_device, out_size, out_nchw);
    else
        hipLaunchKernelGGL((augment_ingest_u8_kernel<false, Taps>), grid, dim3(256), 0, S(stream), (const uint8_t*)src_u8, src_bytes,
                           params_device, out_size, out_nchw);
    AY_CHECK_LAUNCH("augment_ingest_u8_kernel");
    return AY_OK;
}

}  // namespace ay

extern "C" int ay_augment_ingest_u8(const void* src_u8, size_t src_bytes, const ay_aug_params* params_device, int batch, int out_size,
                                    float* out_nchw, ay_stream_t stream) {
    return ay::augment_launch<ay::TileTaps>("ay_augment_ingest_u8", src_u8, src_bytes, params_device, batch, out_size, out_nchw, stream);
}

extern "C" int ay_augment_ingest_window_u8(const void* src_u8, size_t src_bytes, const ay_aug_window_params* params_device, int batch,
                                           int out_size, float* out_nchw, ay_stream_t stream) {
    return ay::augment_launch<ay::WindowTaps>("ay_augment_ingest_window_u8", src_u8, src_bytes, params_device, batch, out_size, out_nchw,
                                              stream);
}
