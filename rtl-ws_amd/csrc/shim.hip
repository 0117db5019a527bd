// shim.hip -- the extern-"C" layer declared in include/rtlws_hip.h.
//
// Host C code (rtl-ws_amd/host/*.c) and the Python test/bench plumbing reach
// the kernels only through these functions.  The twiddle tables come from
// twiddle_tables.cpp, uploaded once per engine and N.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "rtlws_hip.h"
#include "rtlws_internal.h"
#include "twiddle_tables.h"

using rtlws::is_fused_n;

namespace {

thread_local std::string g_err;

void set_err(const char* what, hipError_t e)
{
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    g_err = buf;
}

#define HIP_TRY(expr, ret)                      \
    do {                                        \
        hipError_t _e = (expr);                 \
        if (_e != hipSuccess) {                 \
            set_err(#expr, _e);                 \
            return ret;                         \
        }                                       \
    } while (0)

#define NEED_ENGINE(e, ret)                                   \
    do {                                                      \
        if (!(e)) {                                           \
            g_err = std::string(__func__) + ": null engine";  \
            return ret;                                       \
        }                                                     \
    } while (0)

struct DevFree {
    void operator()(void* p) const { (void)hipFree(p); }
};

// The device copies of one size's rtlws::HostTables (null where that table is empty); `mem` owns them.
struct Tables {
    float2 *tw1 = nullptr, *tw1_128 = nullptr, *tw2 = nullptr, *hann_cs = nullptr;
    float* hann = nullptr;
    double2 *tw64 = nullptr, *tw1_64 = nullptr, *tw1u_64 = nullptr, *tw2_64 = nullptr, *hann_cs64 = nullptr,
            *twxa_64 = nullptr, *twxb_64 = nullptr;
    double* hann64 = nullptr;
    std::vector<std::unique_ptr<void, DevFree>> mem;
};

enum class Prec { F32, F64 };

// Kernel-selection switches (experiments, A/B runs, tests).  Read from the environment ONCE, when
// the engine is created, and changed afterwards only through rtlws_engine_set_option: nothing on a
// launch path calls getenv (tests/test_abi_cpu.py checks the library's imports per function).
struct EngineOpts {
    int v2, blocks_per_cu, f64_fused, f64_blocks_per_cu, f64_x1024, f64_x_waves, cic_direct, cic_round;
};

int norm_tristate(int v) { return v < 0 ? -1 : v != 0; }
int norm_flag(int v) { return v != 0; }
int norm_count(int v) { return v > 0 ? v : 0; }
int norm_waves(int v) { return v == 1 || v == 8 ? v : 0; }
int norm_round(int v) { return v == 1 || v == 2 || v == 4 ? v : 0; }

// include/rtlws_hip.h documents each; the environment and rtlws_engine_set_option both go through `norm`
struct OptionDef {
    const char* name;
    const char* env;
    int EngineOpts::*field;
    int dflt;
    int (*norm)(int);
};
const OptionDef kOptions[] = {
    {"v2", "RTLWS_V2", &EngineOpts::v2, -1, norm_tristate},                     // -1: the default rule (use_v2)
    {"blocks_per_cu", "RTLWS_BLOCKS_PER_CU", &EngineOpts::blocks_per_cu, 0, norm_count},
    {"f64_fused", "RTLWS_F64_FUSED", &EngineOpts::f64_fused, 1, norm_flag},
    {"f64_blocks_per_cu", "RTLWS_F64_BLOCKS_PER_CU", &EngineOpts::f64_blocks_per_cu, 0, norm_count},
    {"f64_x1024", "RTLWS_F64_X1024", &EngineOpts::f64_x1024, 1, norm_flag},
    {"f64_x_waves", "RTLWS_F64_X_WAVES", &EngineOpts::f64_x_waves, 0, norm_waves},   // 0: by batch size
    {"cic_direct", "RTLWS_CIC_DIRECT", &EngineOpts::cic_direct, 0, norm_flag},
    {"cic_round", "RTLWS_CIC_ROUND", &EngineOpts::cic_round, 0, norm_round},
};

const OptionDef* find_option(const char* name)
{
    for (const OptionDef& o : kOptions)
        if (name && std::strcmp(o.name, name) == 0) return &o;
    return nullptr;
}

}  // namespace

struct rtlws_engine {
    int device = 0;
    int cu_count = 256;
    hipStream_t stream = nullptr;
    EngineOpts opt;
    bool x_waves8_ok = true;     // the device's LDS limit per workgroup holds spectrum_f64_1024x.hip's eight-wavefront form (136 KiB)
    std::mutex mu;
    std::map<std::pair<Prec, int>, Tables> tables;   // by precision and n_fft
};

namespace {

template <typename D, typename H>
bool upload(Tables& tb, const std::vector<H>& host, D** dev)
{
    static_assert(sizeof(D) == sizeof(H), "host and device table layouts differ");
    if (host.empty()) return true;
    hipError_t err = hipMalloc(dev, host.size() * sizeof(H));
    if (err == hipSuccess) {
        tb.mem.emplace_back(*dev);
        err = hipMemcpy(*dev, host.data(), host.size() * sizeof(H), hipMemcpyHostToDevice);
    }
    if (err != hipSuccess) set_err("twiddle table upload", err);
    return err == hipSuccess;
}

// The tables of one precision and N, built and uploaded once per engine: nullptr on failure.
const Tables* get_tables(rtlws_engine* e, Prec prec, int n_fft)
{
    std::lock_guard<std::mutex> lk(e->mu);
    const auto key = std::make_pair(prec, n_fft);
    auto it = e->tables.find(key);
    if (it != e->tables.end()) return &it->second;
    HIP_TRY(hipSetDevice(e->device), nullptr);
    const rtlws::HostTables h = prec == Prec::F64 ? rtlws::tables_f64(n_fft) : rtlws::tables_f32(n_fft);
    // spectrum_f64_1024x.hip reads its inner twiddles [slot][lane]: a wave-instruction then covers 1 KiB contiguous
    // (eight 128-byte lines), where the host table's [lane][slot] puts its 64 lanes on 64 different lines
    std::vector<rtlws::D2> twxb_t(h.twxb_64.size());
    for (size_t i = 0; i < twxb_t.size(); ++i) twxb_t[(i % 16) * (twxb_t.size() / 16) + i / 16] = h.twxb_64[i];
    Tables tb;
    if (!upload(tb, h.tw1, &tb.tw1) || !upload(tb, h.tw1_128, &tb.tw1_128) || !upload(tb, h.tw2, &tb.tw2) ||
        !upload(tb, h.hann_cs, &tb.hann_cs) || !upload(tb, h.hann, &tb.hann) || !upload(tb, h.tw64, &tb.tw64) ||
        !upload(tb, h.hann64, &tb.hann64) || !upload(tb, h.tw1_64, &tb.tw1_64) || !upload(tb, h.tw1u_64, &tb.tw1u_64) ||
        !upload(tb, h.tw2_64, &tb.tw2_64) || !upload(tb, h.hann_cs64, &tb.hann_cs64) ||
        !upload(tb, h.twxa_64, &tb.twxa_64) || !upload(tb, twxb_t, &tb.twxb_64))
        return nullptr;
    return &(e->tables[key] = std::move(tb));
}

// include/rtlws_hip.h "Streams": NULL = the engine's own non-blocking stream,
// RTLWS_STREAM_DEFAULT = HIP's legacy default stream, anything else = that stream.
hipStream_t pick_stream(rtlws_engine* e, void* stream)
{
    if (stream == RTLWS_STREAM_DEFAULT) return hipStreamLegacy;
    return stream ? reinterpret_cast<hipStream_t>(stream) : e->stream;
}

bool desc_ok(const rtlws_spectra_desc* d)
{
    if (!d) return false;
    if (d->n_fft < 2 || d->k_avg < 1) return false;
    if (d->input < RTLWS_IN_CU8 || d->input > RTLWS_IN_RF32) return false;
    if (d->window != RTLWS_WIN_RECT && d->window != RTLWS_WIN_HANN) return false;
    if (d->output < RTLWS_OUT_POWER_SUM || d->output > RTLWS_OUT_PAYLOAD_U8) return false;
    if (d->cic_r < 0) return false;
    if (d->cic_r > 1 && d->input != RTLWS_IN_CU8) return false;
    if (!is_fused_n(d->n_fft) && d->n_fft > 8192) return false;   // direct kernel: frame in <=64 KiB LDS
    return true;
}

// spectrum_fused_v2.hip (two virtual threads per lane) for the descriptors it covers.  By
// default only K = 1 rows take it: measured +4..8 % there (rect_4096pt 0.532 -> 0.577 of the HBM
// roofline, Hann K = 1 0.471 -> 0.496) and -1..-4 % with K = 8 accumulators, where both kernels
// deliver the same points per second (DESIGN.md, configs[2]).  RTLWS_V2=0|1 forces either
// kernel for every K at engine creation (rtlws_engine_set_option(e, "v2", ...) afterwards: A/B
// runs, tests/test_v2_gpu.py).
bool use_v2(const rtlws_engine* e, int n_fft, int in_kind, int k_avg)
{
    if (!rtlws::fused_v2_kind(n_fft, in_kind)) return false;
    return e->opt.v2 >= 0 ? (e->opt.v2 != 0) : (RTLWS_V2_DEFAULT != 0 && k_avg == 1);
}

// Input stage of the fused kernels for a CIC factor.  For A/B experiments
// (tools/cic_fused_rates.py): option cic_direct keeps every R != 8 on the
// per-lane direct loads, cic_round = 1|2|4 forces the LDS staging depth
// where R fits it.
int cic_in_kind(const rtlws_engine* e, int R)
{
    if (R == 8) return rtlws::IN_CU8_CIC8;
    if (e->opt.cic_direct) return rtlws::cicr_direct_kind(R);
    if (e->opt.cic_round) {
        const int k = rtlws::cicr_lds_kind(R, e->opt.cic_round);
        if (k >= 0) return k;
    }
    return rtlws::cicr_kind(R);
}

// The f32 kernel a descriptor takes and its grid: rtlws_spectra_batch launches it, rtlws_spectra_grid reports it.
struct PlanF32 {
    int in_kind;
    bool v2;
    int blocks, threads, lds_bytes;
};

PlanF32 plan_f32(const rtlws_engine* e, const rtlws_spectra_desc* d, long ngroups)
{
    const int n = d->n_fft;
    if (!is_fused_n(n))   // the direct kernel: a workgroup per row; it sums the R bytes of a CIC factor itself
        return {d->input, false, (int)ngroups, 256, (int)(sizeof(float2) * n)};
    PlanF32 p;
    p.in_kind = d->cic_r > 1 ? cic_in_kind(e, d->cic_r) : d->input;
    p.v2 = use_v2(e, n, p.in_kind, d->k_avg);
    const bool win = d->window == RTLWS_WIN_HANN;
    const bool kone = d->k_avg == 1 && rtlws::fused_kone_kind(p.in_kind);
    // 4 x waves-per-SIMD wavefronts per CU, n/1024 wavefronts per workgroup.
    // Persistent: each workgroup strides over the output rows.
    int per_cu = p.v2 ? rtlws::v2_blocks_per_cu(n) : 4 * rtlws::fused_waves_per_simd(n, p.in_kind, win, kone) / (n / 1024);
    if (e->opt.blocks_per_cu > 0) per_cu = e->opt.blocks_per_cu;   // experiments only
    const long blocks = std::min((long)e->cu_count * per_cu, ngroups);
    p.blocks = (int)(blocks < 1 ? 1 : blocks);
    p.threads = p.v2 ? n / 32 : n / 16;
    p.lds_bytes = p.v2 ? rtlws::v2_lds_bytes(n) : rtlws::fused_lds_bytes(n, p.in_kind, win);
    return p;
}

// The f64 kernel a descriptor takes: the fused throughput kernel (spectrum_f64_fused.hip) where it exists and
// the pointers suit it, else the row-per-workgroup kernel (spectrum_f64.hip).
struct PlanF64 {
    int in_kind;
    bool fused, x1024;
    int waves, blocks;
};

PlanF64 plan_f64(const rtlws_engine* e, const rtlws_spectra_desc* d, long ngroups, const void* d_in, const void* d_out)
{
    PlanF64 p{d->cic_r > 1 ? cic_in_kind(e, d->cic_r) : d->input, false, false, 0, 0};
    // the fused kernel's vector accesses: 16-byte rows at N = 1024 (either row precision), 16-byte
    // input pieces on the CIC-fused kinds; anything less aligned takes the general kernel
    const bool aligned = !(reinterpret_cast<uintptr_t>(d_out) & 15u) &&
                         (p.in_kind < rtlws::IN_CU8_CIC8 || !(reinterpret_cast<uintptr_t>(d_in) & 15u));
    // option f64_fused = 0 keeps everything on the row-per-workgroup kernel (A/B runs, tests)
    p.fused = rtlws::f64_fused_kind(d->n_fft, p.in_kind) && e->opt.f64_fused && aligned;
    if (!p.fused) return p;
    int per_cu = rtlws::f64_fused_blocks_per_cu(d->n_fft);
    if (e->opt.f64_blocks_per_cu > 0 && e->opt.f64_blocks_per_cu <= 2 * per_cu) per_cu = e->opt.f64_blocks_per_cu;   // experiments only
    p.blocks = (int)std::min((long)e->cu_count * per_cu, ngroups);
    // rectangular 1024-point cmplx_u8 frames: one LDS transposition instead of two
    // (its dB / payload epilogues beside K-frame accumulators would spill: those stay where they were)
    p.x1024 = d->n_fft == 1024 && p.in_kind == rtlws::IN_CU8 && d->window != RTLWS_WIN_HANN && e->opt.f64_x1024 &&
              (d->output == RTLWS_OUT_POWER_SUM || d->k_avg == 1);
    if (p.x1024) {
        // batches with at least four rows per wavefront: one eight-wavefront workgroup per CU whose
        // wavefronts take the workgroup's rows one at a time (spectrum_f64_1024x.hip, WAVES)
        p.waves = e->opt.f64_x_waves;
        if (p.waves == 0) p.waves = (ngroups >= 32L * e->cu_count) ? 8 : 1;
        if (!e->x_waves8_ok) p.waves = 1;
        if (p.waves >= 8) p.blocks = e->cu_count;
    }
    return p;
}

// hipStreamWaitEvent dereferences its stream argument: the hipStreamLegacy token ((hipStream_t)1) crashes it
// (ROCm 7.2).  This library is built with the legacy default-stream semantics, where stream 0 IS that stream.
hipStream_t waitable(hipStream_t st) { return st == hipStreamLegacy ? nullptr : st; }

// The tail of every launching entry point, after its argument checks: hipSetDevice, then `launch` on the
// caller's stream (include/rtlws_hip.h "Streams").  0, or -3 with the error under the name `what`.
template <typename Launch>
int launch_on(rtlws_engine* e, void* stream, const char* what, Launch&& launch)
{
    HIP_TRY(hipSetDevice(e->device), -3);
    const hipError_t err = launch(pick_stream(e, stream));
    if (err != hipSuccess) {
        set_err(what, err);
        return -3;
    }
    return 0;
}

}  // namespace

extern "C" {

int rtlws_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n < 0 ? 0 : n;
}

int rtlws_device_pci_bus_id(int device, char* buf, int len)
{
    g_err.clear();
    if (!buf || len < 16 || device < 0 || device >= rtlws_device_count()) {
        g_err = "rtlws_device_pci_bus_id: bad device or buffer (>= 16 bytes)";
        return -1;
    }
    HIP_TRY(hipDeviceGetPCIBusId(buf, len, device), -3);
    return 0;
}

rtlws_engine* rtlws_engine_create(int device)
{
    g_err.clear();
    int n = rtlws_device_count();
    if (device < 0 || device >= n) {
        g_err = "rtlws_engine_create: no such HIP device (there is no CPU fallback)";
        return nullptr;
    }
    HIP_TRY(hipSetDevice(device), nullptr);
    rtlws_engine* e = new rtlws_engine;
    e->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        e->cu_count = prop.multiProcessorCount;
    // the only place the library reads these variables
    for (const OptionDef& o : kOptions) {
        const char* v = getenv(o.env);
        e->opt.*o.field = (v && *v) ? o.norm(atoi(v)) : o.dflt;
    }
    // the eight-wavefront workgroups of spectrum_f64_1024x.hip need 136 KiB of LDS: where the device cannot give
    // a workgroup that much, large batches keep the one-wavefront form (17 KiB) instead of failing
    int lds_max = 0;
    if (hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess ||
        (size_t)lds_max < rtlws::spectra_f64_1024x_lds_bytes(8))
        e->x_waves8_ok = false;
    hipError_t err = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
    if (err != hipSuccess) {
        set_err("hipStreamCreate", err);
        delete e;
        return nullptr;
    }
    return e;
}

void rtlws_engine_destroy(rtlws_engine* e)
{
    if (!e) return;
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    e->tables.clear();
    (void)hipStreamDestroy(e->stream);
    delete e;
}

int rtlws_engine_device(const rtlws_engine* e) { return e ? e->device : -1; }

void* rtlws_engine_stream(const rtlws_engine* e) { return e ? e->stream : nullptr; }

int rtlws_engine_set_option(rtlws_engine* e, const char* name, int value)
{
    g_err.clear();
    NEED_ENGINE(e, -1);
    const OptionDef* o = find_option(name);
    if (!o) {
        g_err = std::string("rtlws_engine_set_option: unknown option '") + (name ? name : "") + "'";
        return -1;
    }
    std::lock_guard<std::mutex> lk(e->mu);
    e->opt.*o->field = o->norm(value);
    return 0;
}

int rtlws_engine_get_option(const rtlws_engine* e, const char* name)
{
    if (!e || !name) return -2;
    if (std::strcmp(name, "cu_count") == 0) return e->cu_count;
    const OptionDef* o = find_option(name);
    return o ? e->opt.*o->field : -2;
}

int rtlws_engine_prepare(rtlws_engine* e, int n_fft)
{
    g_err.clear();
    rtlws_spectra_desc d;
    std::memset(&d, 0, sizeof d);
    d.n_fft = n_fft;
    d.k_avg = 1;
    if (!e || !desc_ok(&d)) {
        g_err = "rtlws_engine_prepare: unsupported size";
        return -1;
    }
    return get_tables(e, Prec::F32, n_fft) ? 0 : -3;
}

int rtlws_engine_prepare_f64(rtlws_engine* e, int n_fft)
{
    g_err.clear();
    rtlws_spectra_desc d;
    std::memset(&d, 0, sizeof d);
    d.n_fft = n_fft;
    d.k_avg = 1;
    if (!e || !desc_ok(&d)) {
        g_err = "rtlws_engine_prepare_f64: unsupported size (2 <= n_fft <= 8192)";
        return -1;
    }
    if (!get_tables(e, Prec::F64, n_fft)) return -3;
    // Kernels that need more than 64 KiB of LDS opt in once per kernel and device: every launcher that can take
    // this size does that NOW, so that a launch -- under hipGraph capture too -- makes no other runtime call.
    HIP_TRY(hipSetDevice(e->device), -3);
    hipError_t err = rtlws::prepare_spectra_f64(n_fft, e->device);
    if (err == hipSuccess && n_fft == 1024) err = rtlws::prepare_spectra_f64_fused_1024(e->device);
    if (err == hipSuccess && n_fft == 1024 && e->x_waves8_ok) err = rtlws::prepare_spectra_f64_1024x(e->device);
    if (err == hipSuccess && n_fft == 2048) err = rtlws::prepare_spectra_f64_fused_2048(e->device);
    if (err == hipSuccess && n_fft == 4096) err = rtlws::prepare_spectra_f64_fused_4096(e->device);
    if (err != hipSuccess) {
        set_err("rtlws_engine_prepare_f64: hipFuncSetAttribute", err);
        return -3;
    }
    return 0;
}

const char* rtlws_last_error(void) { return g_err.c_str(); }

void* rtlws_dev_alloc(rtlws_engine* e, size_t bytes)
{
    NEED_ENGINE(e, nullptr);
    void* p = nullptr;
    HIP_TRY(hipSetDevice(e->device), nullptr);
    HIP_TRY(hipMalloc(&p, bytes ? bytes : 1), nullptr);
    return p;
}

void rtlws_dev_free(rtlws_engine* e, void* dptr)
{
    if (!dptr || !e) return;
    (void)hipSetDevice(e->device);
    (void)hipFree(dptr);
}

void* rtlws_pinned_alloc(size_t bytes)
{
    void* p = nullptr;
    // Portable | Mapped, explicitly: the zero-copy paths have kernels of ANY engine's device read
    // and write these buffers (stream rows, the drop-in staging buffers), whatever device was
    // current on the allocating thread
    HIP_TRY(hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable | hipHostMallocMapped), nullptr);
    return p;
}

void rtlws_pinned_free(void* hptr)
{
    if (hptr) (void)hipHostFree(hptr);
}

int rtlws_copy_h2d(rtlws_engine* e, void* dst, const void* src, size_t bytes, void* stream)
{
    NEED_ENGINE(e, -1);
    HIP_TRY(hipSetDevice(e->device), -3);
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, pick_stream(e, stream)), -3);
    return 0;
}

int rtlws_copy_d2h(rtlws_engine* e, void* dst, const void* src, size_t bytes, void* stream)
{
    NEED_ENGINE(e, -1);
    HIP_TRY(hipSetDevice(e->device), -3);
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, pick_stream(e, stream)), -3);
    return 0;
}

int rtlws_memset_dev(rtlws_engine* e, void* dst, int value, size_t bytes, void* stream)
{
    NEED_ENGINE(e, -1);
    HIP_TRY(hipSetDevice(e->device), -3);
    HIP_TRY(hipMemsetAsync(dst, value, bytes, pick_stream(e, stream)), -3);
    return 0;
}

int rtlws_stream_sync(rtlws_engine* e, void* stream)
{
    NEED_ENGINE(e, -1);
    HIP_TRY(hipSetDevice(e->device), -3);
    HIP_TRY(hipStreamSynchronize(pick_stream(e, stream)), -3);
    return 0;
}

// An event handle is {hipEvent_t, device}: the HIP event is created on the
// device of the engine it is first recorded on (a HIP event belongs to the
// device that was current when it was created, which need not be the engine's
// on a multi-GPU host), and re-created if it is later recorded on another one.
struct rtlws_event {
    hipEvent_t ev = nullptr;
    int device = -1;
    unsigned flags = hipEventDefault;
};

void* rtlws_event_create(void)
{
    return new rtlws_event;
}

void* rtlws_event_create_blocking(void)
{
    rtlws_event* x = new rtlws_event;
    x->flags = hipEventBlockingSync | hipEventDisableTiming;
    return x;
}

void* rtlws_queue_create(rtlws_engine* e)
{
    NEED_ENGINE(e, nullptr);
    HIP_TRY(hipSetDevice(e->device), nullptr);
    hipStream_t q = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&q, hipStreamNonBlocking), nullptr);
    return q;
}

void rtlws_queue_destroy(rtlws_engine* e, void* queue)
{
    if (!e || !queue || queue == RTLWS_STREAM_DEFAULT) return;
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(reinterpret_cast<hipStream_t>(queue));
    (void)hipStreamDestroy(reinterpret_cast<hipStream_t>(queue));
}

int rtlws_queue_wait_event(rtlws_engine* e, void* stream, void* ev)
{
    NEED_ENGINE(e, -1);
    rtlws_event* x = reinterpret_cast<rtlws_event*>(ev);
    if (!x || !x->ev) { g_err = "rtlws_queue_wait_event: event was never recorded"; return -1; }
    if (x->device != e->device) { g_err = "rtlws_queue_wait_event: event belongs to another device"; return -1; }
    HIP_TRY(hipSetDevice(e->device), -3);
    HIP_TRY(hipStreamWaitEvent(waitable(pick_stream(e, stream)), x->ev, 0), -3);
    return 0;
}

void rtlws_event_destroy(void* ev)
{
    rtlws_event* x = reinterpret_cast<rtlws_event*>(ev);
    if (!x) return;
    if (x->ev) {
        (void)hipSetDevice(x->device);
        (void)hipEventDestroy(x->ev);
    }
    delete x;
}

int rtlws_event_record(void* ev, rtlws_engine* e, void* stream)
{
    NEED_ENGINE(e, -1);
    rtlws_event* x = reinterpret_cast<rtlws_event*>(ev);
    if (!x) { g_err = "rtlws_event_record: null event"; return -1; }
    HIP_TRY(hipSetDevice(e->device), -3);
    if (x->ev && x->device != e->device) {
        (void)hipEventDestroy(x->ev);
        x->ev = nullptr;
    }
    if (!x->ev) {
        HIP_TRY(hipEventCreateWithFlags(&x->ev, x->flags), -3);
        x->device = e->device;
    }
    HIP_TRY(hipEventRecord(x->ev, pick_stream(e, stream)), -3);
    return 0;
}

int rtlws_event_sync(void* ev)
{
    rtlws_event* x = reinterpret_cast<rtlws_event*>(ev);
    if (!x || !x->ev) { g_err = "rtlws_event_sync: event was never recorded"; return -1; }
    HIP_TRY(hipSetDevice(x->device), -3);
    HIP_TRY(hipEventSynchronize(x->ev), -3);
    return 0;
}

float rtlws_event_elapsed_ms(void* start, void* stop)
{
    rtlws_event* a = reinterpret_cast<rtlws_event*>(start);
    rtlws_event* b = reinterpret_cast<rtlws_event*>(stop);
    float ms = -1.0f;
    if (!a || !b || !a->ev || !b->ev || a->device != b->device ||
        ((a->flags | b->flags) & hipEventDisableTiming)) {
        g_err = "rtlws_event_elapsed_ms: events must both be recorded, on the same device, with timing";
        return -1.0f;
    }
    HIP_TRY(hipSetDevice(a->device), -1.0f);
    HIP_TRY(hipEventSynchronize(b->ev), -1.0f);
    HIP_TRY(hipEventElapsedTime(&ms, a->ev, b->ev), -1.0f);
    return ms;
}

int rtlws_spectra_kernel_kind(const rtlws_spectra_desc* d)
{
    if (!desc_ok(d)) return 0;
    return is_fused_n(d->n_fft) ? 1 : 2;
}

int rtlws_spectra_grid(rtlws_engine* e, const rtlws_spectra_desc* d, long nframes, int* blocks,
                       int* threads, int* lds_bytes)
{
    if (!e || !desc_ok(d) || nframes < 0 || nframes % d->k_avg) return -1;
    if (d->flags & RTLWS_FLAG_F64) {   // rtlws_spectra_batch_f64's plan, for 16-byte aligned buffers
        const long ngroups = nframes / d->k_avg;
        const PlanF64 k = plan_f64(e, d, ngroups, nullptr, nullptr);
        if (blocks) *blocks = k.fused ? (k.blocks < 1 ? 1 : k.blocks) : (int)ngroups;
        if (threads) *threads = !k.fused ? 256 : k.x1024 ? 64 * k.waves : d->n_fft / 16;
        if (lds_bytes) *lds_bytes = 0;   // held by the kernels' own launch tables
        return 0;
    }
    const PlanF32 k = plan_f32(e, d, nframes / d->k_avg);
    if (blocks) *blocks = k.blocks;
    if (threads) *threads = k.threads;
    if (lds_bytes) *lds_bytes = k.lds_bytes;
    return 0;
}

int rtlws_spectra_batch(rtlws_engine* e, const rtlws_spectra_desc* d, const void* d_in,
                        long nframes, void* d_out, void* stream)
{
    g_err.clear();
    if (!e || !desc_ok(d) || !d_in || !d_out || nframes < 0 || nframes % d->k_avg) {
        g_err = "rtlws_spectra_batch: bad descriptor, pointer or frame count";
        return -1;
    }
    if (nframes == 0) return 0;
    // The kernels use 16-byte vector accesses (CIC input, N = 1024 output rows):
    // refuse pointers the hardware would fault on rather than launch.
    if ((reinterpret_cast<uintptr_t>(d_in) & 15u) || (reinterpret_cast<uintptr_t>(d_out) & 15u)) {
        g_err = "rtlws_spectra_batch: d_in and d_out must be 16-byte aligned";
        return -1;
    }
    const Tables* tb = get_tables(e, Prec::F32, d->n_fft);
    if (!tb) return -3;

    const bool fused = is_fused_n(d->n_fft);
    rtlws::SpectraParams p;
    std::memset(&p, 0, sizeof p);
    p.in = d_in;
    p.out = d_out;
    p.ngroups = nframes / d->k_avg;
    p.k_avg = d->k_avg;
    p.cic_r = d->cic_r > 1 ? d->cic_r : 1;
    p.n_fft = d->n_fft;
    p.out_mode = d->output;
    const bool scaled = (d->input != RTLWS_IN_RF32);
    p.tw1 = (fused && scaled) ? tb->tw1_128 : tb->tw1;
    p.tw2 = tb->tw2;
    p.in_scale = scaled ? 0.0078125f : 1.0f;
    p.window = (d->window == RTLWS_WIN_HANN) ? tb->hann : nullptr;
    p.hann_cs = tb->hann_cs;
    p.db_offset = (float)(-10.0 * std::log10((double)d->k_avg));
    // reference src/cbb_main.c:112: pow(10, gain_db/10) with C integer division
    p.lin_gain = (float)(std::pow(10.0, (double)(d->gain_db / 10)) / (double)d->k_avg);

    const PlanF32 k = plan_f32(e, d, p.ngroups);
    return launch_on(e, stream, "spectra kernel launch", [&](hipStream_t s) {
        if (!fused) return rtlws::launch_spectra_direct(p, k.in_kind, s);
        if (k.v2) return rtlws::launch_spectra_fused_v2(p, k.blocks, s);
        switch (d->n_fft) {
        case 1024: return rtlws::launch_spectra_fused_1024(p, k.in_kind, k.blocks, s);
        case 2048: return rtlws::launch_spectra_fused_2048(p, k.in_kind, k.blocks, s);
        default: return rtlws::launch_spectra_fused_4096(p, k.in_kind, k.blocks, s);
        }
    });
}

int rtlws_payload_from_sums(rtlws_engine* e, const float* d_sums, int n, int count, int gain_db,
                            void* d_out, void* stream)
{
    g_err.clear();
    if (!e || n < 0 || count <= 0 || (n > 0 && (!d_sums || !d_out))) {
        g_err = "rtlws_payload_from_sums: bad argument";
        return -1;
    }
    return launch_on(e, stream, "payload kernel launch", [&](hipStream_t s) {
        const float lin = (float)(std::pow(10.0, (double)(gain_db / 10)) / (double)count);
        return rtlws::launch_payload(d_sums, n, lin, reinterpret_cast<uint8_t*>(d_out), s);
    });
}

int rtlws_spectra_batch_f64(rtlws_engine* e, const rtlws_spectra_desc* d, const void* d_in,
                            long nframes, void* d_out, void* stream)
{
    g_err.clear();
    if (!e || !desc_ok(d) || !d_in || !d_out || nframes < 0 || nframes % d->k_avg) {
        g_err = "rtlws_spectra_batch_f64: bad descriptor (2 <= n_fft <= 8192), pointer or frame count";
        return -1;
    }
    if (nframes == 0) return 0;
    const unsigned out_align = ((d->flags & RTLWS_FLAG_ROWS_F32) || d->output == RTLWS_OUT_PAYLOAD_U8) ? 3u : 7u;
    if ((reinterpret_cast<uintptr_t>(d_in) & 7u) || (reinterpret_cast<uintptr_t>(d_out) & out_align)) {
        g_err = "rtlws_spectra_batch_f64: d_in must be 8-byte aligned, d_out 8-byte (4-byte for f32 rows and payload bytes)";
        return -1;
    }
    const Tables* tb = get_tables(e, Prec::F64, d->n_fft);
    if (!tb) return -3;

    rtlws::SpectraParamsF64 p;
    std::memset(&p, 0, sizeof p);
    p.in = d_in;
    p.out = d_out;
    p.ngroups = nframes / d->k_avg;
    p.k_avg = d->k_avg;
    p.cic_r = d->cic_r > 1 ? d->cic_r : 1;
    p.n_fft = d->n_fft;
    p.log2n = 0;
    if ((d->n_fft & (d->n_fft - 1)) == 0)
        for (int n = d->n_fft; n > 1; n >>= 1) ++p.log2n;
    p.out_mode = d->output;
    p.count = d->k_avg;
    p.tw = tb->tw64;
    p.window = (d->window == RTLWS_WIN_HANN) ? tb->hann64 : nullptr;
    // reference src/cbb_main.c:112: pow(10, gain_db/10) with C integer division
    p.lin_gain = std::pow(10.0, (double)(d->gain_db / 10));
    p.in_scale = (d->input != RTLWS_IN_RF32) ? 0.0078125 : 1.0;

    p.tw1f = (d->input == RTLWS_IN_RF32) ? tb->tw1u_64 : tb->tw1_64;
    p.tw2f = tb->tw2_64;
    p.hann_csf = tb->hann_cs64;
    p.rows_f32 = (d->flags & RTLWS_FLAG_ROWS_F32) && d->output != RTLWS_OUT_PAYLOAD_U8;
    p.twxa = tb->twxa_64;
    p.twxb = tb->twxb_64;

    const PlanF64 k = plan_f64(e, d, p.ngroups, d_in, d_out);
    return launch_on(e, stream, "f64 spectra kernel launch", [&](hipStream_t s) {
        if (!k.fused) return rtlws::launch_spectra_f64(p, d->input, s, e->device);
        if (k.x1024) return rtlws::launch_spectra_f64_1024x(p, k.blocks, k.waves, s, e->device);
        switch (d->n_fft) {
        case 1024: return rtlws::launch_spectra_f64_fused_1024(p, k.in_kind, k.blocks, s, e->device);
        case 2048: return rtlws::launch_spectra_f64_fused_2048(p, k.in_kind, k.blocks, s, e->device);
        default: return rtlws::launch_spectra_f64_fused_4096(p, k.in_kind, k.blocks, s, e->device);
        }
    });
}

int rtlws_payload_from_sums_f64(rtlws_engine* e, const double* d_sums, int n, int count, int gain_db,
                                void* d_out, void* stream)
{
    g_err.clear();
    if (!e || n < 0 || count <= 0 || (n > 0 && (!d_sums || !d_out))) {
        g_err = "rtlws_payload_from_sums_f64: bad argument";
        return -1;
    }
    return launch_on(e, stream, "f64 payload kernel launch", [&](hipStream_t s) {
        return rtlws::launch_payload_f64(d_sums, n, std::pow(10.0, (double)(gain_db / 10)), count,
                                         reinterpret_cast<uint8_t*>(d_out), s);
    });
}

int rtlws_welch_accumulate_f64(rtlws_engine* e, double* d_acc, const double* d_part, int n,
                               long frames_end, double* d_b, void* stream)
{
    g_err.clear();
    if (!e || n < 2 || frames_end < 0 || !d_acc || !d_part || !d_b) {
        g_err = "rtlws_welch_accumulate_f64: bad argument";
        return -1;
    }
    return launch_on(e, stream, "welch accumulate kernel launch", [&](hipStream_t s) {
        return rtlws::launch_welch_accumulate(d_acc, d_part, n, frames_end, d_b, s);
    });
}

int rtlws_welch_finish_f64(rtlws_engine* e, double* d_acc, int n, long total, double* d_b, void* stream)
{
    g_err.clear();
    if (!e || n < 2 || total < 0 || !d_acc || !d_b) {
        g_err = "rtlws_welch_finish_f64: bad argument";
        return -1;
    }
    return launch_on(e, stream, "welch finish kernel launch", [&](hipStream_t s) {
        return rtlws::launch_welch_finish(d_acc, n, total, d_b, s);
    });
}

int rtlws_cic_block_sums(rtlws_engine* e, int R, const void* d_src, long dst_len, void* d_dst,
                         void* stream)
{
    g_err.clear();
    if (!e || R < 1 || R > 128 || dst_len < 0 || (dst_len > 0 && (!d_src || !d_dst))) {
        g_err = "rtlws_cic_block_sums: bad argument (1 <= R <= 128)";
        return -1;
    }
    if ((reinterpret_cast<uintptr_t>(d_src) & 15u) || (reinterpret_cast<uintptr_t>(d_dst) & 7u)) {
        g_err = "rtlws_cic_block_sums: d_src must be 16-byte and d_dst 8-byte aligned";
        return -1;
    }
    return launch_on(e, stream, "cic kernel launch", [&](hipStream_t s) {
        return rtlws::launch_cic_block_sums(R, d_src, dst_len, d_dst, s, e->cu_count);
    });
}

int rtlws_fm_demod(rtlws_engine* e, const void* d_iq, long len, const float* d_prev_in,
                   float* d_prev_out, float* d_out, void* stream)
{
    g_err.clear();
    if (!e || len < 0 || !d_prev_in || !d_prev_out || d_prev_in == d_prev_out ||
        (len > 0 && (!d_iq || !d_out))) {
        g_err = "rtlws_fm_demod: bad argument";
        return -1;
    }
    if ((reinterpret_cast<uintptr_t>(d_iq) & 7u) || (reinterpret_cast<uintptr_t>(d_out) & 3u)) {
        g_err = "rtlws_fm_demod: d_iq must be 8-byte and d_out 4-byte aligned";
        return -1;
    }
    if (len == 0)   // nothing to demodulate: the carried phase passes through
        return launch_on(e, stream, "fm_demod phase copy", [&](hipStream_t s) {
            return hipMemcpyAsync(d_prev_out, d_prev_in, sizeof(float), hipMemcpyDeviceToDevice, s);
        });
    return launch_on(e, stream, "fm_demod kernel launch", [&](hipStream_t s) {
        return rtlws::launch_fm_demod(d_iq, len, d_prev_in, d_prev_out, d_out, s, e->cu_count);
    });
}

int rtlws_clock_stamp(rtlws_engine* e, unsigned long long* d_out, int slots, void* stream)
{
    g_err.clear();
    NEED_ENGINE(e, -1);
    if (!d_out || (reinterpret_cast<uintptr_t>(d_out) & 7u) || slots < 1 || slots > 65536) {
        g_err = "rtlws_clock_stamp: d_out must be an 8-byte aligned device pointer to slots x 4 64-bit words, 1 <= slots <= 65536";
        return -1;
    }
    return launch_on(e, stream, "clock stamp kernel launch", [&](hipStream_t s) {
        return rtlws::launch_clock_stamp(d_out, slots, s);
    });
}

int rtlws_copy_d2d(rtlws_engine* e, void* dst, const void* src, size_t bytes, void* stream)
{
    NEED_ENGINE(e, -1);
    HIP_TRY(hipSetDevice(e->device), -3);
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, pick_stream(e, stream)), -3);
    return 0;
}

int rtlws_halfband(rtlws_engine* e, const float* d_x, float* d_y, long out_len, void* stream)
{
    g_err.clear();
    if (!e || out_len < 0 || (out_len > 0 && (!d_x || !d_y))) {
        g_err = "rtlws_halfband: bad argument";
        return -1;
    }
    return launch_on(e, stream, "halfband kernel launch", [&](hipStream_t s) {
        return rtlws::launch_halfband(d_x, d_y, out_len, s, e->cu_count);
    });
}

}  // extern "C"
