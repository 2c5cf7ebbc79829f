// The index map of the three packed-filter layouts (include/amyloid_yolo.h): which OIHW fp32 filter value element i of an image
// holds.  The single-call packers (ay_layout.hip, ay_train_bf16.hip) and the batched packer (ay_train_bf16.hip) all go through it.
#pragma once
#include "ay_common.h"

namespace ay {

struct PackJob {             // mirrors ay_pack_job (include/amyloid_yolo.h)
    const float* src;        // OIHW fp32 filters
    uint16_t* dst;           // packed 16-bit image
    int32_t kind;            // 0: forward image (ay_pack_conv_weights_*), 1: data gradient (ay_pack_dgrad_weights_bf16), 2: stride-2 parity classes
    int32_t cout, cout_pad, cin, cin_pad, ksize;
    uint64_t total;          // elements of dst
};

// the fp32 source value of element i of job jb's image, 0 for padding
__device__ __forceinline__ float packed_filter_value(const PackJob& jb, size_t i) {
    const float* w = jb.src;
    if (jb.kind == 0) {   // [cin/16][tap][half][cout_pad][8]; cin here = channels of the source tensor (multiple of 16)
        const int kk2 = jb.ksize * jb.ksize;
        const int j = (int)(i % 8);
        size_t t = i / 8;
        const int co = (int)(t % jb.cout_pad);
        t /= jb.cout_pad;
        const int half = (int)(t % 2);
        t /= 2;
        const int tap = (int)(t % kk2);
        const int chunk = (int)(t / kk2);
        const int ci = chunk * 16 + half * 8 + j;
        return co < jb.cout ? w[((size_t)co * jb.cin + ci) * kk2 + tap] : 0.f;
    }
    if (jb.kind == 1) {   // [cout_pad/16][tap][half][cin_pad][8], flipped taps, transposed channels: the forward kernel computes
                          // dx = conv(dz, W') with W'[ci][co][kh][kw] = W[co][ci][k-1-kh][k-1-kw]
        const int ks = jb.ksize, kk2 = ks * ks;
        const int j = (int)(i % 8);
        size_t t = i / 8;
        const int ci = (int)(t % jb.cin_pad);
        t /= jb.cin_pad;
        const int half = (int)(t % 2);
        t /= 2;
        const int tap = (int)(t % kk2);
        const int chunk = (int)(t / kk2);
        const int co = chunk * 16 + half * 8 + j;
        const int kh = tap / ks, kw = tap % ks;
        return co < jb.cout && ci < jb.cin ? w[(((size_t)co * jb.cin + ci) * ks + (ks - 1 - kh)) * ks + (ks - 1 - kw)] : 0.f;
    }
    // kind 2: [class py*2+px][cout_pad/16][window tap oy*2+ox][half][cin_pad][8]; window row oy of class py holds filter row kh:
    // py = 0: oy 0 -> kh 1, oy 1 -> none; py = 1: oy 0 -> kh 2, oy 1 -> kh 0 (columns alike)
    const size_t per_class = (size_t)(jb.cout_pad / 16) * 4 * 2 * jb.cin_pad * 8;
    const int cls = (int)(i / per_class);
    size_t t = i % per_class;
    const int j = (int)(t % 8);
    t /= 8;
    const int ci = (int)(t % jb.cin_pad);
    t /= jb.cin_pad;
    const int half = (int)(t % 2);
    t /= 2;
    const int tap = (int)(t % 4);
    const int chunk = (int)(t / 4);
    const int co = chunk * 16 + half * 8 + j;
    const int py = cls >> 1, px = cls & 1, oy = tap >> 1, ox = tap & 1;
    const int kh = py ? (oy ? 0 : 2) : (oy ? -1 : 1);
    const int kw = px ? (ox ? 0 : 2) : (ox ? -1 : 1);
    return co < jb.cout && ci < jb.cin && kh >= 0 && kw >= 0 ? w[(((size_t)co * jb.cin + ci) * 3 + kh) * 3 + kw] : 0.f;
}

// one image per launch (ay_layout.hip): the single-call packers fill a PackJob on the host; act_dtype AY_DT_BF16 | AY_DT_F16
void launch_pack_filter(const PackJob& jb, int act_dtype, unsigned grid, hipStream_t stream);

}  // namespace ay
