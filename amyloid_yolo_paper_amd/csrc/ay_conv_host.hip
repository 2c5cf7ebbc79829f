// Host side of every persistent conv launch (declared in ay_conv_common.h and ay_phase_clock.h): CU count, counter sets of the dynamic
// item dealing (the kernels reach g_deal only through ConvArgs::deal), ConvArgs initialiser, traversal, AY_DBG, grid, phase-clock read-out.
#include <stdlib.h>

#include <atomic>
#include <mutex>

#include "ay_conv_common.h"

namespace ay {
// dynamic item dealing: 64 rotating sets of {8 per-XCD item counters, exit counter}; zero at load, reset by the last workgroup
constexpr int DEAL_SETS = 64, DEAL_STREAMS = 16;
__device__ unsigned g_deal[DEAL_STREAMS * DEAL_SETS][16];

static int current_device() {
    int dev = 0;
    (void)hipGetDevice(&dev);
    return dev < 0 || dev >= 64 ? 0 : dev;
}
int conv_num_cus() {
    static std::atomic<int> cus[64];  // per device
    const int dev = current_device();
    int n = cus[dev].load(std::memory_order_relaxed);
    if (!n) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, dev) == hipSuccess) n = p.multiProcessorCount;
        if (n < 8) n = 256;
        if (getenv("AY_CUS")) n = atoi(getenv("AY_CUS"));  // timing experiments only
        n -= n % 8;
        cus[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}

// Counter set of the next ring-kernel launch on `st` (nullptr: static dealing).  The sets of one stream are used in rotation
// by launches that the stream serialises -- the last workgroup of a launch hands its set back zeroed before the next launch
// on that stream starts -- so a set must never be shared by two streams, whose launches may overlap: every (device, stream)
// pair owns DEAL_SETS sets of its own, up to DEAL_STREAMS streams per device; further streams deal statically.  A set pointer
// baked into a captured graph node stays valid under the same rule: replay the graph on the stream it was captured on, or on
// any stream as long as nothing else on the CAPTURE stream runs concurrently.  The owners' table is at file scope so that
// ay_conv_deal_probe reads it under the same mutex.
namespace {
struct DealTable {  // of one device; guarded by g_deal_mu
    unsigned* base = nullptr;
    hipStream_t streams[DEAL_STREAMS] = {};
    unsigned seq[DEAL_STREAMS] = {};
    int n = 0;
};
std::mutex g_deal_mu;
DealTable g_deal_tables[64];
}  // namespace

unsigned* next_deal_set(hipStream_t st) {
    std::lock_guard<std::mutex> lock(g_deal_mu);
    DealTable& pd = g_deal_tables[current_device()];
    if (!pd.base) {
        void* p = nullptr;
        if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_deal)) != hipSuccess) return nullptr;  // this device's copy of the symbol
        pd.base = (unsigned*)p;
    }
    int k = 0;
    while (k < pd.n && pd.streams[k] != st) ++k;
    if (k == pd.n) {
        if (pd.n == DEAL_STREAMS) return nullptr;
        pd.streams[pd.n++] = st;
    }
    return pd.base + ((size_t)k * DEAL_SETS + (pd.seq[k]++ % DEAL_SETS)) * 16;
}

void fill_args(ConvArgs& a, const ay_conv_desc* d, const void* src, const void* w, const float* scale, const float* shift,
               const void* residual, void* out, int TH, int TW, int BN) {
    a = ConvArgs{};
    a.src = (const uint8_t*)src;
    a.w = (const uint8_t*)w;
    a.scale = scale;
    a.shift = shift;
    a.residual = (const uint8_t*)residual;
    a.out = (uint8_t*)out;
    a.batch = d->batch;
    a.cin = d->cin;
    a.cout_pad = d->cout_pad;
    a.hin = d->hin;
    a.win = d->win;
    a.hout = d->hout;
    a.wout = d->wout;
    a.tiles_x = (d->wout + TW - 1) / TW;
    a.tiles_y = (d->hout + TH - 1) / TH;
    a.n_cgroups = d->cout_pad / BN;
    a.leaky = d->leaky;
    a.dbg = 0;
    a.src1 = nullptr;
    a.c1 = 0;
    a.deal = nullptr;
    a.canvas_gx = 0;
    a.w_class_stride = 0;
    a.reverse = conv_traversal_reverse();
}

// Per host thread: a launch takes the direction in force on the thread that issues it (a captured launch keeps it in its node)
static thread_local int t_traversal_reverse = 0;
int conv_traversal_reverse() { return t_traversal_reverse; }
}  // namespace ay

// Tests and debugging only (synchronous): the dealing state of the current device as next_deal_set left it.  Reads the table, never
// registers `stream`, never advances a rotation.
extern "C" int ay_conv_deal_probe(ay_stream_t stream, int32_t* slot, uint32_t* launches, int32_t* nonzero_words) {
    using namespace ay;
    AY_CHECK_ARG(slot && launches && nonzero_words, "ay_conv_deal_probe: null argument");
    if (hipDeviceSynchronize() != hipSuccess) {
        set_error("ay_conv_deal_probe: device synchronisation failed");
        return AY_ERR_LAUNCH;
    }
    static unsigned host[DEAL_STREAMS * DEAL_SETS][16];  // 64 KiB: under the mutex, not on the stack
    std::lock_guard<std::mutex> lock(g_deal_mu);
    const DealTable& pd = g_deal_tables[current_device()];
    int k = 0;
    while (k < pd.n && pd.streams[k] != (hipStream_t)stream) ++k;
    *slot = k < pd.n ? k : -1;
    *launches = k < pd.n ? pd.seq[k] : 0u;
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_deal), sizeof(host)) != hipSuccess) {
        set_error("ay_conv_deal_probe: reading the counter sets failed");
        return AY_ERR_LAUNCH;
    }
    int nz = 0;
    for (int i = 0; i < DEAL_STREAMS * DEAL_SETS; ++i)
        for (int j = 0; j < 16; ++j) nz += host[i][j] != 0;
    *nonzero_words = nz;
    return AY_OK;
}
extern "C" void ay_conv_set_traversal(int reverse) { ay::t_traversal_reverse = reverse != 0; }
extern "C" int ay_conv_get_traversal(void) { return ay::t_traversal_reverse; }
namespace ay {
int conv_dbg() {
    static const int dbg = getenv("AY_DBG") ? atoi(getenv("AY_DBG")) : 0;
    return dbg;
}

unsigned persistent_grid(long long n_items, int wgs_per_cu) {
    if (n_items <= 0 || n_items > 0x7fffffffLL) return 0;
    const long long per_xcd = (n_items + 7) / 8;
    const long long cu_slots = (long long)wgs_per_cu * (conv_num_cus() / 8);
    return (unsigned)(8 * (per_xcd < cu_slots ? per_xcd : cu_slots));
}

unsigned mulhi_divisor(unsigned d) { return d <= 1 ? 0xffffffffu : (unsigned)(0x100000000ULL / d); }

bool phase_clock_read(hipStream_t st, const void* ticks, unsigned long long* t, int n) {  // synchronous: timing experiments only
    void* dev = nullptr;  // this device's copy of the tick array
    if (!ticks || !(conv_dbg() & DBG_CLOCK) || hipGetSymbolAddress(&dev, ticks) != hipSuccess) return false;
    (void)hipStreamSynchronize(st);
    const bool ok = hipMemcpy(t, dev, n * sizeof(*t), hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipMemset(dev, 0, n * sizeof(*t));
    return ok;
}
}  // namespace ay
