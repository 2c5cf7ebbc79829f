// The column runs of THE PAIR WINDOW RULE as first built (csrc/ay_spatial.hip now reads the words of `bits` directly and keeps no runs:
// profiles/spatial_window.txt): per mask cell the nearest OUT row at or above and at or below it in its column.  Two ways to build
// them, timed on a blob-shaped mask of G x G cells (G = 547: a 70 000-px slide on 128-px cells; G = 4 375: on 16-px cells):
//   chunks:  one lane per (chunk of 64 rows, column): the chunk's OUT cells as one word (pair_window_bits_kernel's loop), then
//            (up, down) from the word and, for the carry, from the nearest chunk of the column that has an OUT cell
//   columns: one lane per column, a sweep down (up) and a sweep up (down); G lanes in all
// Both are coalesced across the columns and write the same 8 bytes per cell; the program checks that they agree.
//   hipcc -O3 --offload-arch=gfx950 scripts/micro/window_runs.hip -o scripts/micro/window_runs && scripts/micro/window_runs
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

constexpr int THREADS = 256, CHUNK = 64;

__global__ void __launch_bounds__(THREADS) bits_kernel(const uint8_t* __restrict__ mask, int gx, int gy, unsigned long long* __restrict__ bits) {
    const int n_chunks = (gy + CHUNK - 1) / CHUNK, t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= n_chunks * gx) return;
    const int c = t / gx, g = t - c * gx, y0 = c * CHUNK, n = min(CHUNK, gy - y0);
    unsigned long long w = 0;
#pragma unroll 8
    for (int r = 0; r < n; ++r) w |= (unsigned long long)(mask[(y0 + r) * gx + g] == 0) << r;
    bits[t] = w;
}

__global__ void __launch_bounds__(THREADS) runs_kernel(const unsigned long long* __restrict__ bits, int gx, int gy, int2* __restrict__ runs) {
    const int n_chunks = (gy + CHUNK - 1) / CHUNK, t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= n_chunks * gx) return;
    const int c = t / gx, g = t - c * gx, y0 = c * CHUNK, n = min(CHUNK, gy - y0);
    const unsigned long long w = bits[t];
    int up = -1, down = gy;
    for (int cc = c - 1; cc >= 0; --cc) {
        const unsigned long long v = bits[cc * gx + g];
        if (v) {
            up = cc * CHUNK + 63 - __clzll((long long)v);
            break;
        }
    }
    for (int cc = c + 1; cc < n_chunks; ++cc) {
        const unsigned long long v = bits[cc * gx + g];
        if (v) {
            down = cc * CHUNK + __ffsll((long long)v) - 1;
            break;
        }
    }
    for (int r = 0; r < n; ++r) {
        const unsigned long long at_or_above = w & (~0ull >> (63 - r)), at_or_below = w >> r;
        const int u = at_or_above ? y0 + 63 - __clzll((long long)at_or_above) : up;
        const int d = at_or_below ? y0 + r + __ffsll((long long)at_or_below) - 1 : down;
        runs[(y0 + r) * gx + g] = make_int2(u, d);
    }
}

__global__ void __launch_bounds__(THREADS) columns_kernel(const uint8_t* __restrict__ mask, int gx, int gy, int2* __restrict__ runs) {
    const int g = blockIdx.x * THREADS + threadIdx.x;
    if (g >= gx) return;
    int up = -1, down = gy;
#pragma unroll 8
    for (int y = 0; y < gy; ++y) {
        if (mask[y * gx + g] == 0) up = y;
        runs[y * gx + g].x = up;
    }
#pragma unroll 8
    for (int y = gy - 1; y >= 0; --y) {
        if (mask[y * gx + g] == 0) down = y;
        runs[y * gx + g].y = down;
    }
}

int main() {
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    const int sizes[] = {547, 4375};
    for (int G : sizes) {
        std::vector<uint8_t> m((size_t)G * G);
        for (int y = 0; y < G; ++y)
            for (int x = 0; x < G; ++x) {   // a wavy ellipse with a lattice of round holes
                const float fy = (y + 0.5f) / G - 0.5f, fx = (x + 0.5f) / G - 0.5f, ang = atan2f(fy, fx);
                const float rad = 1.0f + 0.12f * sinf(3 * ang + 1.0f) + 0.08f * sinf(7 * ang + 2.0f);
                const float hy = fmodf(fy + 0.5f, 0.125f) - 0.0625f, hx = fmodf(fx + 0.5f, 0.125f) - 0.0625f;
                m[(size_t)y * G + x] = (fy / 0.40f) * (fy / 0.40f) + (fx / 0.44f) * (fx / 0.44f) <= rad * rad && hy * hy + hx * hx > 0.02f * 0.02f;
            }
        const size_t cells = (size_t)G * G;
        const int n_chunks = (G + CHUNK - 1) / CHUNK;
        uint8_t* mask;
        unsigned long long* bits;
        int2 *ra, *rb;
        CK(hipMalloc((void**)&mask, cells));
        CK(hipMalloc((void**)&bits, (size_t)n_chunks * G * 8));
        CK(hipMalloc((void**)&ra, cells * 8));
        CK(hipMalloc((void**)&rb, cells * 8));
        CK(hipMemcpy(mask, m.data(), cells, hipMemcpyHostToDevice));
        const unsigned cb = (unsigned)(((size_t)n_chunks * G + THREADS - 1) / THREADS), lb = (unsigned)((G + THREADS - 1) / THREADS);
        for (int variant = 0; variant < 2; ++variant) {
            float ms[9], lo = 1e9f, hi = 0;
            for (int rep = -2; rep < 9; ++rep) {   // two warm launches
                CK(hipEventRecord(e0, 0));
                if (variant == 0) {
                    hipLaunchKernelGGL(bits_kernel, dim3(cb), dim3(THREADS), 0, 0, mask, G, G, bits);
                    hipLaunchKernelGGL(runs_kernel, dim3(cb), dim3(THREADS), 0, 0, bits, G, G, ra);
                } else {
                    hipLaunchKernelGGL(columns_kernel, dim3(lb), dim3(THREADS), 0, 0, mask, G, G, rb);
                }
                CK(hipEventRecord(e1, 0));
                CK(hipEventSynchronize(e1));
                CK(hipGetLastError());
                if (rep >= 0) {
                    CK(hipEventElapsedTime(&ms[rep], e0, e1));
                    lo = fminf(lo, ms[rep]), hi = fmaxf(hi, ms[rep]);
                }
            }
            for (int i = 0; i < 9; ++i)
                for (int j = i + 1; j < 9; ++j)
                    if (ms[j] < ms[i]) {
                        const float t = ms[i];
                        ms[i] = ms[j], ms[j] = t;
                    }
            printf("G = %4d (%8zu cells), %-38s median %8.3f ms  [%.3f, %.3f] over 9\n", G, cells,
                   variant == 0 ? "chunks of 64 rows (two kernels):" : "one lane per column (one kernel):", ms[4], lo, hi);
        }
        std::vector<int2> ha(cells), hb(cells);
        CK(hipMemcpy(ha.data(), ra, cells * 8, hipMemcpyDeviceToHost));
        CK(hipMemcpy(hb.data(), rb, cells * 8, hipMemcpyDeviceToHost));
        printf("G = %4d: the two agree: %s\n", G, memcmp(ha.data(), hb.data(), cells * 8) == 0 ? "yes" : "NO");
        CK(hipFree(mask));
        CK(hipFree(bits));
        CK(hipFree(ra));
        CK(hipFree(rb));
    }
    return 0;
}
