// Plaque segmentation (wsi.segment_boxes, wsi.quantify_region(segment=True); THE SEGMENT RULE is stated in include/amyloid_yolo.h and
// restated in NumPy by tests/segment_reference.py): the 8-connected stain-positive component under every detection, out of a resident
// region of the slide.  One workgroup of 256 per OWNED row, rows grid-stride; a row that is not owned costs its four fp32 edges.
//
//   box_segments_kernel<SIDE>   everything of a window of at most SIDE x SIDE pixels happens in LDS:
//     1. classify   a wavefront takes 64 consecutive pixels of a window row (byte loads: region_tap_u8's), od in LDS, the tissue test
//                   before the unmixing, and two ballots make the POSITIVE and the CORE bit plane, [SIDE rows][WPR words].
//     2. runs       the unit of the labelling is the RUN, a maximal row segment of positive pixels: a row of SIDE pixels has at most
//                   RPR = (SIDE + 1) / 2 of them, so run (y, k) has the id y * RPR + k, ids grow in raster order of the runs' first
//                   pixels, and the run of a pixel is a prefix count of run starts (pre[y][word] + a popcount).  parent[id] is 32 bits
//                   wide, which is what an LDS atomicMin takes; 255 * 128 ids are 127.5 KiB, what 16-bit pixel labels would need.
//     3. unions     a union-find over the runs: for every word of a row, the contacts with the row above come from bit operations (the
//                   first pixel of every overlap, and the diagonal contacts at the ends of the upper runs that no overlap covers), and
//                   each is one union: find both roots, atomicMin the smaller into the larger root's parent, follow what the atomic
//                   returns.  ONE pass, no sweeps to convergence: a spiral costs what a disc costs.  Parents only ever decrease and
//                   stay inside the component, so concurrent unions and the path halving of find are safe.
//     4. flatten    parent[id] = its root; the root of a component is its lowest id: the run that holds its lowest raster index,
//                   which is the rule's tie-break.
//     5. areas      the root's word becomes (ROOT | IN_BOX | area): every word of a row adds its segments' pixels to the root.
//     6. select     one LDS atomicMax over (area << 15 | 32767 - id) of the candidates, a count of them.
//     7. sums       one pass over the selected component: core, perimeter, bounding box, sides and in-box pixels from the bit planes,
//                   and the only second read of the image, for the bins.
//   Every find and every union is a loop whose variable strictly decreases, and carries a cap of RUNS steps on top of that; a thread
//   that hits the cap sets an LDS word, the workgroup reads it behind a barrier and writes AY_SEG_INTERNAL.  No loop iterates to
//   convergence, and every barrier sits in control flow that depends on the row's numbers and on LDS words read behind a barrier only.
//
// Two instances, launched one after the other over the same rows: SIDE = 96 (22 KiB of LDS: the ordinary plaque, several workgroups
// per CU; it also writes the rows that need no window: NONFINITE, EMPTY, LARGE) and SIDE = 255 (147 KiB: one workgroup per CU) for
// the windows with a side above 96.  profiles/segment_codegen.txt has the figures.
//
// Integers and order-free integer atomics only: the same bytes every run.  Kernel launches only: no allocation, no memset node, no
// host read, no scratch, no workspace beyond `out`.
#include "ay_slide_pass.h"

namespace ay {

constexpr int SEG_SMALL = 96;     // the cut between the two instances
constexpr uint32_t SEG_ROOT = 0x80000000u, SEG_IN_BOX = 0x40000000u, SEG_AREA = 0x0003ffffu;   // a root's word behind phase 5
enum { SA_POS, SA_CAND, SA_AREA, SA_CORE, SA_BINS, SA_PERIM, SA_SX, SA_SY, SA_X0, SA_Y0, SA_X1, SA_Y1, SA_SIDES, SA_IN, SA_N };

__device__ __forceinline__ uint32_t seg_ld(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// the root of run i, with path halving.  parent[] only holds ids <= the index: i strictly decreases.
__device__ __forceinline__ uint32_t seg_find(uint32_t* parent, uint32_t i, int cap, int* err) {
    uint32_t p = seg_ld(parent + i);
    for (int it = 0; p != i; ++it) {
        if (it >= cap) { *err = 1; break; }
        const uint32_t g = seg_ld(parent + p);
        if (g != p) atomicMin(parent + i, g);
        i = p, p = g;
    }
    return i;
}

// max(a, b) strictly decreases from one iteration to the next
__device__ __forceinline__ void seg_union(uint32_t* parent, uint32_t a, uint32_t b, int cap, int* err) {
    for (int it = 0;; ++it) {
        a = seg_find(parent, a, cap, err), b = seg_find(parent, b, cap, err);
        if (a == b) break;
        if (a < b) { const uint32_t t = a; a = b, b = t; }
        const uint32_t old = atomicMin(parent + a, b);
        if (old == a) break;                                 // a was a root and now hangs under b
        if (it >= cap) { *err = 1; break; }
        a = old;                                             // somebody else linked a first: join what it hangs under with b
    }
}

// bit k is set iff a <= x0 + k < b
__device__ __forceinline__ uint32_t seg_range_mask(int a, int b, int x0) {
    const int lo = min(max(a - x0, 0), 32), hi = min(max(b - x0, 0), 32);
    return hi > lo ? (hi == 32 ? 0xffffffffu : (1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
}

template <int SIDE>
__global__ void __launch_bounds__(256) box_segments_kernel(const uint8_t* __restrict__ reg, int H, int W, size_t stride, int shrink, int bg,
                                                            int oy, int ox, int slide_h, int slide_w, int own_y0, int own_y1,
                                                            const ay_stain_params* __restrict__ params, int stain, int thres_bin,
                                                            int core_bin, int margin, int min_area, int above, bool plain_rows,
                                                            const float* __restrict__ rows, int M, int32_t* __restrict__ out,
                                                            int32_t* __restrict__ flags) {
    constexpr int WPR = 2 * ((SIDE + 63) / 64);              // words of a plane row: what the ballots of a row's chunks fill
    constexpr int RPR = (SIDE + 1) / 2;                      // runs a row can hold
    constexpr int RUNS = SIDE * RPR;
    static_assert(RUNS <= 32768 && SIDE * SIDE <= (int)SEG_AREA, "a run id takes 15 bits, an area 18");
    __shared__ float od[256];
    __shared__ uint32_t pos[SIDE * WPR], core[SIDE * WPR], parent[RUNS];
    __shared__ uint8_t pre[SIDE * WPR];                      // run starts of the row in the words before this one
    __shared__ int acc[SA_N];
    __shared__ uint32_t best;
    __shared__ int err;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    od[tid] = params->od[tid];
    const float d0 = params->D[stain], d1 = params->D[3 + stain], d2 = params->D[6 + stain];

    for (long long m = blockIdx.x; m < M; m += gridDim.x) {   // m and everything derived from the row is workgroup-uniform
        const float* r = rows + (size_t)m * 7;
        const float x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
        int status = 0, wx0 = 0, wy0 = 0, ww = 0, wh = 0, lo_x = 0, hi_x = 0, lo_y = 0, hi_y = 0;
        if (!(load_finite(x1) && load_finite(y1) && load_finite(x2) && load_finite(y2))) {
            status = AY_SEG_NONFINITE;
        } else {
            lo_x = load_edge(x1, slide_w), hi_x = load_edge(x2, slide_w), lo_y = load_edge(y1, slide_h), hi_y = load_edge(y2, slide_h);
            if (lo_x >= hi_x || lo_y >= hi_y) {
                status = AY_SEG_EMPTY;
            } else {
                wx0 = max(lo_x - margin, 0), wy0 = max(lo_y - margin, 0);
                ww = min(hi_x + margin, slide_w) - wx0, wh = min(hi_y + margin, slide_h) - wy0;
                if (ww > AY_SEG_MAX_SIDE || wh > AY_SEG_MAX_SIDE) status = AY_SEG_LARGE;
                else if (wx0 < ox || wx0 + ww > ox + W || wy0 < oy || wy0 + wh > oy + H) status = AY_SEG_NOT_RESIDENT;
            }
        }
        if (wy0 < own_y0 || wy0 >= own_y1) continue;         // the owner row: wy0, or 0 without a window
        const bool window = status == 0 || status == AY_SEG_NOT_RESIDENT;
        if (window ? !(max(ww, wh) > above && max(ww, wh) <= SIDE) : !plain_rows) continue;   // the other instance's
        int32_t* o = out + (size_t)m * AY_SEG_COLS;
        if (status) {
            if (tid < AY_SEG_COLS) o[tid] = tid == 0 ? status : tid == 1 ? wx0 : tid == 2 ? wy0 : tid == 3 ? ww : tid == 4 ? wh : 0;
            if (tid == 0) atomicOr(flags, status);
            continue;
        }

        __syncthreads();                                     // the last row's reads of the tables are over (first row: od is there)
        if (tid < SA_N) acc[tid] = tid == SA_X0 || tid == SA_Y0 ? 0x7fffffff : tid == SA_X1 || tid == SA_Y1 ? -1 : 0;
        if (tid == 0) best = 0, err = 0;
        // 1. classify: a wavefront per 64 pixels of a row; the window is resident, so every tap is inside the region
        const int nch = (ww + 63) >> 6, nw = (ww + 31) >> 5;
        for (int it = wave; it < wh * nch; it += 4) {        // `it` is uniform over the wavefront: all 64 lanes vote
            const int y = it / nch, c = it - y * nch, x = c * 64 + lane;
            bool p = false, k = false;
            int b[3];
            if (x < ww && region_tap_u8(reg, stride, shrink, H, W, (unsigned)(wx0 - ox + x), (unsigned)(wy0 - oy + y), b) && tissue_px(b, bg)) {
                const int q = load_bin(od, b, d0, d1, d2);
                p = q >= thres_bin, k = p && q >= core_bin;
            }
            const unsigned long long pm = __ballot(p), km = __ballot(k);
            if (lane == 0) {
                uint32_t* pw = pos + y * WPR + 2 * c;
                uint32_t* kw = core + y * WPR + 2 * c;
                pw[0] = (uint32_t)pm, pw[1] = (uint32_t)(pm >> 32), kw[0] = (uint32_t)km, kw[1] = (uint32_t)(km >> 32);
            }
        }
        __syncthreads();
        // 2. per row: the run starts before every word, and the positive pixels
        for (int y = tid; y < wh; y += 256) {
            int cnt = 0, n_pos = 0;
            uint32_t carry = 0;
            for (int w = 0; w < nw; ++w) {
                const uint32_t c = pos[y * WPR + w];
                pre[y * WPR + w] = (uint8_t)cnt;
                cnt += __builtin_popcount(c & ~((c << 1) | carry)), n_pos += __builtin_popcount(c), carry = c >> 31;
            }
            if (n_pos) atomicAdd(acc + SA_POS, n_pos);
        }
        __syncthreads();
        // run of the positive pixel (x, y)
        auto run_of = [&](int y, int x) -> uint32_t {
            const int w = x >> 5;
            const uint32_t c = pos[y * WPR + w], carry = w ? pos[y * WPR + w - 1] >> 31 : 0u;
            const uint32_t s = c & ~((c << 1) | carry);
            return (uint32_t)(y * RPR + pre[y * WPR + w] + __builtin_popcount(s & (0xffffffffu >> (31 - (x & 31)))) - 1);
        };
        // the words of the window; f(y, w, c, carry, first): the word, bit 31 of the word before it, the id of its first run start
        const int n_items = wh * nw;
        auto each_word = [&](auto f) {
            for (int i = tid; i < n_items; i += 256) {
                const int y = i / nw, w = i - y * nw;
                const uint32_t c = pos[y * WPR + w];
                if (c) f(y, w, c, w ? pos[y * WPR + w - 1] >> 31 : 0u, (uint32_t)(y * RPR + pre[y * WPR + w]));
            }
        };
        auto each_start = [&](auto f) {                      // f(id) for every run
            each_word([&](int, int, uint32_t c, uint32_t carry, uint32_t first) {
                const int n = __builtin_popcount(c & ~((c << 1) | carry));
                for (int k = 0; k < n; ++k) f(first + k);
            });
        };
        each_start([&](uint32_t id) { parent[id] = id; });
        __syncthreads();
        // 3. unions with the row above
        each_word([&](int y, int w, uint32_t c, uint32_t carry, uint32_t) {
            if (y == 0) return;
            const uint32_t* up = pos + (y - 1) * WPR;
            const uint32_t p0 = up[w];
            const uint32_t pl = (p0 << 1) | (w ? up[w - 1] >> 31 : 0u);            // bit k: the pixel above-left of x0 + k
            const uint32_t pr = (p0 >> 1) | (w + 1 < nw ? up[w + 1] << 31 : 0u);   // above-right
            const uint32_t cl = (c << 1) | carry;
            const uint32_t cr = (c >> 1) | (w + 1 < nw ? pos[y * WPR + w + 1] << 31 : 0u);
            const uint32_t m0 = c & p0 & ~(cl & pl);         // the first pixel of every overlap of a run with a run above
            const uint32_t ml = c & pl & ~p0 & ~cl;          // the end of a run above, diagonally, where no overlap says the same
            const uint32_t mr = c & pr & ~p0 & ~cr;          // the start of a run above, likewise
            for (uint32_t t = m0 | ml | mr; t; t &= t - 1) {
                const int bit = __builtin_ctz(t), x = w * 32 + bit;
                const uint32_t a = run_of(y, x);
                if (m0 >> bit & 1) seg_union(parent, a, run_of(y - 1, x), RUNS, &err);
                if (ml >> bit & 1) seg_union(parent, a, run_of(y - 1, x - 1), RUNS, &err);
                if (mr >> bit & 1) seg_union(parent, a, run_of(y - 1, x + 1), RUNS, &err);
            }
        });
        __syncthreads();
        // 4. flatten: nothing is joined any more, so the roots are final
        each_start([&](uint32_t id) {
            const uint32_t root = seg_find(parent, id, RUNS, &err);
            if (root != id) atomicMin(parent + id, root);
        });
        __syncthreads();
        if (err) {                                           // read behind the barrier: uniform
            if (tid < AY_SEG_COLS) o[tid] = tid == 0 ? AY_SEG_INTERNAL : tid == 1 ? wx0 : tid == 2 ? wy0 : tid == 3 ? ww : tid == 4 ? wh : 0;
            if (tid == 0) atomicOr(flags, AY_SEG_INTERNAL);
            continue;
        }
        // 5. a root's word becomes ROOT | IN_BOX | area
        each_start([&](uint32_t id) { if (parent[id] == id) parent[id] = SEG_ROOT; });
        __syncthreads();
        const int bx_lo = lo_x - wx0, bx_hi = hi_x - wx0, by_lo = lo_y - wy0, by_hi = hi_y - wy0;   // the box proper, in the window
        auto root_of = [&](uint32_t id) -> uint32_t { const uint32_t e = seg_ld(parent + id); return e & SEG_ROOT ? id : e; };
        auto each_segment = [&](auto f) {                    // f(y, w, segment mask, root): the pieces of runs inside a word
            each_word([&](int y, int w, uint32_t c, uint32_t, uint32_t) {
                for (uint32_t rem = c; rem;) {
                    const int b0 = __builtin_ctz(rem);
                    const uint32_t t = ~(rem >> b0);
                    const int len = t ? __builtin_ctz(t) : 32;
                    const uint32_t seg = (len == 32 ? 0xffffffffu : (1u << len) - 1u) << b0;
                    rem &= ~seg;
                    f(y, w, seg, root_of(run_of(y, w * 32 + b0)));
                }
            });
        };
        each_segment([&](int y, int w, uint32_t seg, uint32_t root) {
            const bool in_box = y >= by_lo && y < by_hi && (seg & seg_range_mask(bx_lo, bx_hi, w * 32));
            atomicAdd(parent + root, (uint32_t)__builtin_popcount(seg));
            if (in_box) atomicOr(parent + root, SEG_IN_BOX);
        });
        __syncthreads();
        // 6. the candidates; the largest, among equals the lowest id
        each_start([&](uint32_t id) {
            const uint32_t e = parent[id], area = e & SEG_AREA;
            if ((e & SEG_ROOT) && (e & SEG_IN_BOX) && (long long)area >= (long long)min_area) {
                atomicAdd(acc + SA_CAND, 1);
                atomicMax(&best, area << 15 | (32767u - id));
            }
        });
        __syncthreads();
        const uint32_t chosen = best;                        // uniform
        if (chosen) {
            // 7. one pass over the selected component
            const uint32_t sel = 32767u - (chosen & 32767u);
            int s[SA_N] = {};
            s[SA_X0] = s[SA_Y0] = 0x7fffffff, s[SA_X1] = s[SA_Y1] = -1;
            uint32_t word = 0;                               // the selected pixels of the word being walked
            int at_y = -1, at_w = -1;
            auto flush = [&]() {
                if (!word) return;
                const int y = at_y, w = at_w, n = __builtin_popcount(word);
                const uint32_t c = pos[y * WPR + w];
                const uint32_t cl = (c << 1) | (w ? pos[y * WPR + w - 1] >> 31 : 0u);
                const uint32_t cr = (c >> 1) | (w + 1 < nw ? pos[y * WPR + w + 1] << 31 : 0u);
                const uint32_t cu = y ? pos[(y - 1) * WPR + w] : 0u, cd = y + 1 < wh ? pos[(y + 1) * WPR + w] : 0u;
                s[SA_AREA] += n, s[SA_CORE] += __builtin_popcount(word & core[y * WPR + w]), s[SA_SY] += n * y;
                s[SA_PERIM] += 4 * n - __builtin_popcount(word & cl) - __builtin_popcount(word & cr) - __builtin_popcount(word & cu) -
                               __builtin_popcount(word & cd);
                const int xa = w * 32 + __builtin_ctz(word), xb = w * 32 + 31 - __builtin_clz(word);
                s[SA_X0] = min(s[SA_X0], xa), s[SA_X1] = max(s[SA_X1], xb), s[SA_Y0] = min(s[SA_Y0], y), s[SA_Y1] = max(s[SA_Y1], y);
                s[SA_SIDES] |= (xa == 0 ? 1 : 0) | (y == 0 ? 2 : 0) | (xb == ww - 1 ? 4 : 0) | (y == wh - 1 ? 8 : 0);
                if (y >= by_lo && y < by_hi) s[SA_IN] += __builtin_popcount(word & seg_range_mask(bx_lo, bx_hi, w * 32));
                for (uint32_t t = word; t; t &= t - 1) {     // the bins: the image again, at the selected pixels only
                    const int x = w * 32 + __builtin_ctz(t);
                    int b[3];
                    if (region_tap_u8(reg, stride, shrink, H, W, (unsigned)(wx0 - ox + x), (unsigned)(wy0 - oy + y), b))
                        s[SA_BINS] += load_bin(od, b, d0, d1, d2), s[SA_SX] += x;
                }
                word = 0;
            };
            each_segment([&](int y, int w, uint32_t seg, uint32_t root) {
                if (y != at_y || w != at_w) flush(), at_y = y, at_w = w;
                if (root == sel) word |= seg;
            });
            flush();
            if (s[SA_AREA]) {
                for (int k = SA_AREA; k <= SA_SY; ++k) atomicAdd(acc + k, s[k]);
                atomicMin(acc + SA_X0, s[SA_X0]), atomicMin(acc + SA_Y0, s[SA_Y0]);
                atomicMax(acc + SA_X1, s[SA_X1]), atomicMax(acc + SA_Y1, s[SA_Y1]);
                atomicOr(acc + SA_SIDES, s[SA_SIDES]), atomicAdd(acc + SA_IN, s[SA_IN]);
            }
            __syncthreads();
        }
        if (tid < AY_SEG_COLS) {
            int v = 0;
            switch (tid) {
                case 1: v = wx0; break;
                case 2: v = wy0; break;
                case 3: v = ww; break;
                case 4: v = wh; break;
                case 5: v = acc[SA_POS]; break;
                case 6: v = acc[SA_CAND]; break;
                default: break;
            }
            if (chosen) {
                switch (tid) {
                    case 7: v = acc[SA_AREA]; break;
                    case 8: v = acc[SA_CORE]; break;
                    case 9: v = acc[SA_BINS]; break;
                    case 10: v = acc[SA_PERIM]; break;
                    case 11: v = acc[SA_SX]; break;
                    case 12: v = acc[SA_SY]; break;
                    case 13: v = wx0 + acc[SA_X0]; break;
                    case 14: v = wy0 + acc[SA_Y0]; break;
                    case 15: v = wx0 + acc[SA_X1] + 1; break;
                    case 16: v = wy0 + acc[SA_Y1] + 1; break;
                    case 17: v = acc[SA_SIDES]; break;
                    case 18: v = acc[SA_IN]; break;
                    default: break;
                }
            }
            o[tid] = v;
        }
    }
}

}  // namespace ay

extern "C" int ay_box_segments_u8(const void* region_hwc_u8, int region_h, int region_w, size_t row_stride_bytes, int shrink, int origin_y,
                                  int origin_x, int slide_h, int slide_w, int own_y0, int own_y1, int bg_level,
                                  const ay_stain_params* params_device, int stain, int thres_bin, int core_bin, int margin, int min_area,
                                  const float* rows, int n_rows, int32_t* out, int32_t* flags, ay_stream_t stream) {
    using namespace ay;
    AY_CHECK_ARG(region_hwc_u8 && params_device, "ay_box_segments_u8: null");
    if (!check_region("ay_box_segments_u8", region_h, region_w, row_stride_bytes, shrink, true)) return AY_ERR_ARG;
    if (!check_bg_level("ay_box_segments_u8", bg_level)) return AY_ERR_ARG;
    AY_CHECK_ARG((stain == 0 || stain == 1) && thres_bin >= 0 && thres_bin <= core_bin && core_bin <= AY_STAIN_BINS && margin >= 0 &&
                     margin <= AY_SEG_MAX_MARGIN && min_area >= 1,
                 "ay_box_segments_u8: stain %d, thres_bin %d, core_bin %d, margin %d, min_area %d", stain, thres_bin, core_bin, margin, min_area);
    const int H = region_h / shrink, W = region_w / shrink;
    if (!check_on_slide("ay_box_segments_u8", H, W, origin_y, origin_x, slide_h, slide_w)) return AY_ERR_ARG;
    AY_CHECK_ARG(own_y0 >= 0 && own_y0 <= own_y1 && own_y1 <= slide_h, "ay_box_segments_u8: owner rows %d .. %d of %d", own_y0, own_y1, slide_h);
    AY_CHECK_ARG(n_rows >= 0 && (n_rows == 0 || (rows && out && flags)), "ay_box_segments_u8: %d rows %p, out %p, flags %p", n_rows,
                 (const void*)rows, (const void*)out, (const void*)flags);
    if (n_rows == 0) return AY_OK;
    const unsigned blocks = (unsigned)(n_rows > 256 * 8 ? 256 * 8 : n_rows);
    hipLaunchKernelGGL(box_segments_kernel<SEG_SMALL>, dim3(blocks), dim3(256), 0, S(stream), (const uint8_t*)region_hwc_u8, H, W,
                       row_stride_bytes, shrink, bg_level, origin_y, origin_x, slide_h, slide_w, own_y0, own_y1, params_device, stain,
                       thres_bin, core_bin, margin, min_area, 0, true, rows, n_rows, out, flags);
    AY_CHECK_LAUNCH("box_segments_kernel<96>");
    hipLaunchKernelGGL(box_segments_kernel<AY_SEG_MAX_SIDE>, dim3(blocks), dim3(256), 0, S(stream), (const uint8_t*)region_hwc_u8, H, W,
                       row_stride_bytes, shrink, bg_level, origin_y, origin_x, slide_h, slide_w, own_y0, own_y1, params_device, stain,
                       thres_bin, core_bin, margin, min_area, SEG_SMALL, false, rows, n_rows, out, flags);
    AY_CHECK_LAUNCH("box_segments_kernel<255>");
    return AY_OK;
}
