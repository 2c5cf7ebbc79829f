// Box arithmetic that several files must agree on bit for bit: the reference's +1-pixel IoU and the finiteness test of the
// slide-level kernels.  Merge-NMS, ay_box_iou mode 0, the view votes, ay_match_detections, the slide match and the loss metrics
// all take their `> threshold` decisions on this one function.
#pragma once
#include "ay_common.h"

namespace ay {

// bbox_iou(x1y1x2y2=True) of the reference (utils/utils.py:202-232) on corner boxes, in its operation order.  The library is built
// with -ffp-contract=off, so the operations are the ones written here: do not reorder them.
__device__ __forceinline__ float iou_p1(float ax1, float ay1, float ax2, float ay2, float bx1, float by1, float bx2,
                                        float by2) {
    const float ix1 = fmaxf(ax1, bx1), iy1 = fmaxf(ay1, by1);
    const float ix2 = fminf(ax2, bx2), iy2 = fminf(ay2, by2);
    const float inter = fmaxf(ix2 - ix1 + 1.0f, 0.0f) * fmaxf(iy2 - iy1 + 1.0f, 0.0f);
    const float a1 = (ax2 - ax1 + 1.0f) * (ay2 - ay1 + 1.0f);
    const float a2 = (bx2 - bx1 + 1.0f) * (by2 - by1 + 1.0f);
    return inter / (a1 + a2 - inter + 1e-16f);
}

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.0e38f; }   // false for NaN and +-inf

// THE LOAD RULE's box ownership (ay_load.hip, ay_focus.hip): a coordinate counts iff it is finite, up to FLT_MAX
__device__ __forceinline__ bool load_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }   // false for NaN and +-inf

// THE LOAD RULE's edge of a box: the first pixel whose centre is not left of (above) v, clamped into 0 .. n
__device__ __forceinline__ int load_edge(float v, int n) { return (int)fminf(fmaxf(ceilf(v - 0.5f), 0.0f), (float)n); }

}  // namespace ay
