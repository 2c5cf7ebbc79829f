// Training augmentation fused into the tile ingest: uint8 HWC tiles (a ragged batch in one buffer) -> the float32 NCHW batch of the
// training step with flip, rotation / translation (bilinear, zero outside), sharpen, dropout, hue / brightness applied in ONE pass.
// THE AUGMENTATION RULE (include/amyloid_yolo.h) fixes every fp32 operation and its order; tests/augment_reference.py restates it
// in NumPy and the kernel is compared with it bit for bit.  The library is built with -ffp-contract=off: no a * b + c below is fused.
// Nothing random happens here: the per-image records (ay_aug_params) are drawn on the host (amyloid_yolo_paper_amd/augment.py).
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

// steps 1-4 of the rule for output pixel (x, y), 0 <= x, y < S: the three channels of W in 0..255
__device__ __forceinline__ void aug_warp(const uint8_t* __restrict__ img, int h, int w, int D, int left, int top, float scale, float cx,
                                         float cy, const float* inv, int flip, int x, int y, float* W) {
    int qx = min((int)floorf(x * scale), D - 1) - left;
    const int qy = min((int)floorf(y * scale), D - 1) - top;
    if (flip) qx = w - 1 - qx;
    const float xc = (float)qx - cx, yc = (float)qy - cy;
    const float sx = ((inv[0] * xc + inv[1] * yc) + inv[2]) + cx;
    const float sy = ((inv[3] * xc + inv[4] * yc) + inv[5]) + cy;
    const float x0f = floorf(sx), y0f = floorf(sy);
    const float fx = sx - x0f, fy = sy - y0f;
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
        const float a = vy0 && vx0 ? (float)pa[k] : 0.0f;
        const float b = vy0 && vx1 ? (float)pb[k] : 0.0f;
        const float c = vy1 && vx0 ? (float)pc[k] : 0.0f;
        const float d = vy1 && vx1 ? (float)pd[k] : 0.0f;
        const float t = a + fx * (b - a);
        const float u = c + fx * (d - c);
        W[k] = t + fy * (u - t);
    }
}

template <bool VEC4>
__global__ void __launch_bounds__(256) augment_ingest_u8_kernel(const uint8_t* __restrict__ src, size_t src_bytes,
                                                                 const ay_aug_params* __restrict__ params, int S,
                                                                 float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float lds[3][AUG_HH][AUG_PITCH];
    const ay_aug_params& P = params[blockIdx.z];   // the same record for the whole workgroup: scalar loads
    const int h = P.h, w = P.w;
    // a record that does not lie inside [src, src + src_bytes) reads nothing: its image is all padding
    const bool ok = h > 0 && w > 0 && P.src_offset >= 0 && (uint64_t)P.src_offset <= src_bytes &&
                    (uint64_t)h * (uint64_t)w * 3 <= src_bytes - (uint64_t)P.src_offset;
    const int bx = blockIdx.x * AUG_BW, by = blockIdx.y * AUG_BH;
    if (ok) {
        const uint8_t* img = src + P.src_offset;
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
            aug_warp(img, h, w, D, left, top, scale, cx, cy, inv, flip, x, y, W);
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

}  // namespace ay

extern "C" int ay_augment_ingest_u8(const void* src_u8, size_t src_bytes, const ay_aug_params* params_device, int batch, int out_size,
                                    float* out_nchw, ay_stream_t stream) {
    using namespace ay;
    AY_CHECK_ARG(src_u8 && params_device && out_nchw, "ay_augment_ingest_u8: null");
    AY_CHECK_ARG(src_bytes > 0 && batch > 0 && batch <= 65535 && out_size > 0 && out_size <= 32768,
                 "ay_augment_ingest_u8: %zu source bytes, batch %d (1..65535) -> %d (1..32768)", src_bytes, batch, out_size);
    const bool vec4 = out_size % 4 == 0 && ((uintptr_t)out_nchw & 15) == 0;   // every row of every plane then starts on 16 bytes
    const dim3 grid((unsigned)((out_size + AUG_BW - 1) / AUG_BW), (unsigned)((out_size + AUG_BH - 1) / AUG_BH), (unsigned)batch);
    if (vec4)
        hipLaunchKernelGGL(augment_ingest_u8_kernel<true>, grid, dim3(256), 0, S(stream), (const uint8_t*)src_u8, src_bytes, params_device,
                           out_size, out_nchw);
    else
        hipLaunchKernelGGL(augment_ingest_u8_kernel<false>, grid, dim3(256), 0, S(stream), (const uint8_t*)src_u8, src_bytes,
                           params_device, out_size, out_nchw);
    AY_CHECK_LAUNCH("augment_ingest_u8_kernel");
    return AY_OK;
}
