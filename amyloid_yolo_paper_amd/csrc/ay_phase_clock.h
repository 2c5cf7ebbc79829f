// The instrumented build of the persistent conv kernels, all of it: experiment switches and the in-kernel phase clock.  `AY_PHASE_CLOCK=1
// python build.py --force` compiles with -DAY_PHASE_CLOCK; at run time AY_DBG (conv_dbg(), `dbg` of a kernel's argument block) is a sum of the
// bits below.  In the product build every hook is empty and AY_DBGBIT() a compile-time 0: run-time branches inside the unrolled MFMA loops
// cost the register-saturated kernels 20-30 VGPRs of spills.
#pragma once
#include "ay_common.h"
namespace ay {
// AY_DBG bits and the kernels that honour them (ring = conv_bf16_ring_kernel, m16 = conv3x3_m16_ring_kernel, stem / stem v2 =
// stem_s2_fused_kernel / stem_s2_fused_v2_kernel, wgrad = wgrad_bf16_kernel).  Only DBG_CLOCK leaves the results intact.
enum DbgBit {
    DBG_NO_STAGING = 1,    // ring: the stage loop issues no DMA
    DBG_NO_MFMA = 2,       // ring: no MFMA phase (neither fragment reads nor MFMAs)
    DBG_NO_STORES = 4,     // conv_epilogue of a launch that hands conv_dbg() on (ay_conv_fwd_*, stem, stem v2): no output stores
    DBG_CLOCK = 8,         // ring (ay_conv_fwd_* launches), m16, stem, stem v2, wgrad: the phase clock runs, every launch reports
    DBG_NO_STEM = 16,      // stem v2: the producer waves skip the stem phase
    DBG_NO_LAYER1 = 32,    // stem v2: the consumer waves skip layer 1 and its epilogue
    DBG_NO_PREFETCH = 64,  // ring: no fragment prefetch inside the MFMA loop (with 1: the MFMA instructions alone)
};
// Host side (ay_conv_host.hip), after an instrumented launch: with DBG_CLOCK set it waits for `st`, reads the n counters of the tick array
// `ticks` (a HIP_SYMBOL; null in the product build) into t and zeroes the array; false: nothing to report.  The launcher formats t itself.
bool phase_clock_read(hipStream_t st, const void* ticks, unsigned long long* t, int n);
// Device side: AY_PCLK_BEGIN(g, on, AY_PCLK_V(name), ...) gives a kernel its tick counters and time marks, one AY_PCLK_V per name, in 100 MHz
// ticks (wall_clock64), owned by the wave(s) for which `on` = AY_DBGBIT(a, DBG_CLOCK) && <its wave test> holds; all values are wave-uniform.
// A counter's name is its index in the kernel's tick array g (AY_PHASE_TICKS), written out; a mark's name is any word (names are pasted).
// The hooks are macros over plain locals, not member functions: in the instrumented build they expand to the statements these kernels
// carried before, in the same order, so that the ring and m16 kernels stay instruction-identical there too (profiles/phase_clock_codegen.txt).
//   Owning wave: AY_PCLK_MARK(m) mark m = now.  AY_PCLK_TICK(m, k) counter k += now - mark m.  AY_PCLK_LAP(m, k) the same and mark m = now.
//   AY_PCLK_COUNT(k, n) counter k += n.  Every wave: AY_PCLK_SET(m) mark m = now.  Inside if (AY_PCLK_ON) { }, for a site that needs more:
//   AY_PCLK_SINCE(m) now - mark m.  AY_PCLK_LAPV(m, k) LAP, gives the interval.  AY_PCLK_ADD(k, v) counter k += v.  Lane 0: AY_PCLK_FLUSH(k),
//   AY_PCLK_FLUSH_V(k, v), AY_PCLK_FLUSH_MAX(k, v): g[k] += counter k / g[k] += v / g[k] = max(g[k], v), atomically.
#ifdef AY_PHASE_CLOCK
#define AY_DBGBIT(a, bit) ((a).dbg & (bit))
#define AY_PHASE_TICKS(name, n) __device__ unsigned long long name[n]
#define AY_PCLK_V(name) ay_clk_##name = 0
#define AY_PCLK_BEGIN(g, on, ...) unsigned long long* const ay_clk_g = g; const bool ay_clk = (on); unsigned long long __VA_ARGS__
#define AY_PCLK_ON ay_clk
#define AY_PCLK_SINCE(m) (wall_clock64() - ay_clk_##m)
#define AY_PCLK_LAPV(m, k) ({ const unsigned long long t_ = wall_clock64(), d_ = t_ - ay_clk_##m; ay_clk_##k += d_; ay_clk_##m = t_; d_; })
#define AY_PCLK_ADD(k, v) (ay_clk_##k += (v))
#define AY_PCLK_SET(m) ay_clk_##m = wall_clock64()
#define AY_PCLK_FLUSH(k) atomicAdd(&ay_clk_g[k], ay_clk_##k)
#define AY_PCLK_FLUSH_V(k, v) atomicAdd(&ay_clk_g[k], v)
#define AY_PCLK_FLUSH_MAX(k, v) atomicMax(&ay_clk_g[k], v)
#else
#define AY_DBGBIT(a, bit) 0
#define AY_PHASE_TICKS(name, n) constexpr unsigned long long* name = nullptr
#define AY_PCLK_BEGIN(g, on, ...)
#define AY_PCLK_ON false
#define AY_PCLK_SINCE(m) 0ull
#define AY_PCLK_LAPV(m, k) 0ull
#define AY_PCLK_ADD(k, v) ((void)(v))
#define AY_PCLK_SET(m) ((void)0)
#define AY_PCLK_FLUSH(k) ((void)0)
#define AY_PCLK_FLUSH_V(k, v) ((void)(v))
#define AY_PCLK_FLUSH_MAX(k, v) ((void)(v))
#endif
#define AY_PCLK_MARK(m) if (AY_PCLK_ON) AY_PCLK_SET(m)
#define AY_PCLK_TICK(m, k) if (AY_PCLK_ON) AY_PCLK_ADD(k, AY_PCLK_SINCE(m))
#define AY_PCLK_COUNT(k, n) if (AY_PCLK_ON) AY_PCLK_ADD(k, n)
#define AY_PCLK_LAP(m, k) if (AY_PCLK_ON) (void)AY_PCLK_LAPV(m, k)
}  // namespace ay
