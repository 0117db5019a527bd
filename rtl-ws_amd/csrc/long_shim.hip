// long_shim.hip -- extern "C" glue of include/rtlws_long.h (librtlws_long.so): plans, tables, workspace, launches.
// The engine (device, stream) is librtlws_hip.so's; nothing here reads the environment.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rtlws_long.h"
#include "shim_common.h"
#include "spectrum_long.h"

namespace {

void set_err(const char* what, hipError_t e)
{
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    g_err = buf;
}

int log2_exact(int n)     // log2 of a power of two, else -1
{
    if (n < 1 || (n & (n - 1))) return -1;
    int m = 0;
    while ((1 << m) < n) ++m;
    return m;
}

// why a descriptor is not served, or nullptr
const char* why_not(const rtlws_spectra_desc* d)
{
    using namespace rtlws::lng;
    if (!d) return "null descriptor";
    const int m = log2_exact(d->n_fft);
    if (m < MIN_LOG2N || m > MAX_LOG2N) return "n_fft must be a power of two, 2^14 .. 2^20 (shorter frames: rtlws_spectra_batch_f64)";
    if (d->k_avg < 1) return "k_avg must be >= 1";
    if (d->input < RTLWS_IN_CU8 || d->input > RTLWS_IN_RF32) return "unknown input kind";
    if (d->window == RTLWS_WIN_HANN) return "the Hann window is not built for frames above 8192 points";
    if (d->window != RTLWS_WIN_RECT) return "unknown window";
    if (d->output < RTLWS_OUT_POWER_SUM || d->output > RTLWS_OUT_PAYLOAD_U8) return "unknown output kind";
    if (d->cic_r > 1) return "no CIC stage in front of frames above 8192 points (cic_r must be 0 or 1)";
    if (d->cic_r < 0) return "cic_r must be 0 or 1";
    if (d->flags & ~RTLWS_FLAG_ROWS_F32) return "unknown flag (only RTLWS_FLAG_ROWS_F32)";
    return nullptr;
}

}  // namespace

struct rtlws_long_plan {
    rtlws_engine* eng = nullptr;
    int device = 0;
    rtlws_spectra_desc desc;
    int log2n = 0, rows_kind = 0;
    long frames_in_flight = 0;                  // a multiple of k_avg
    size_t ws_bytes = 0;
    double2 *ws = nullptr, *twc = nullptr, *twl = nullptr, *twh = nullptr;
};

namespace {

bool upload(double2** dst, const std::vector<double2>& src)
{
    hipError_t e = hipMalloc(reinterpret_cast<void**>(dst), src.size() * sizeof(double2));
    if (e == hipSuccess) e = hipMemcpy(*dst, src.data(), src.size() * sizeof(double2), hipMemcpyHostToDevice);
    if (e != hipSuccess) set_err("rtlws_long_open: twiddle table", e);
    return e == hipSuccess;
}

void destroy(rtlws_long_plan* p)
{
    (void)hipSetDevice(p->device);
    (void)hipFree(p->ws);
    (void)hipFree(p->twc);
    (void)hipFree(p->twl);
    (void)hipFree(p->twh);
    delete p;
}

}  // namespace

extern "C" {

const char* rtlws_long_last_error(void) { return g_err.c_str(); }

int rtlws_long_supported(const rtlws_spectra_desc* desc)
{
    return supported("rtlws_long", why_not(desc));
}

rtlws_long_plan* rtlws_long_open(rtlws_engine* e, const rtlws_spectra_desc* desc, long max_frames)
{
    using namespace rtlws::lng;
    g_err.clear();
    if (!e) {
        g_err = "rtlws_long_open: null engine (no usable HIP device: there is no CPU path)";
        return nullptr;
    }
    if (const char* why = why_not(desc)) {
        g_err = std::string("rtlws_long_open: ") + why;
        return nullptr;
    }
    rtlws_long_plan* p = new rtlws_long_plan;
    p->eng = e;
    p->device = rtlws_engine_device(e);
    p->desc = *desc;
    p->log2n = log2_exact(desc->n_fft);
    p->rows_kind = desc->output == RTLWS_OUT_PAYLOAD_U8 ? ROWS_U8 : (desc->flags & RTLWS_FLAG_ROWS_F32) ? ROWS_F32 : ROWS_F64;
    const long N = desc->n_fft, K = desc->k_avg;
    const size_t frame_bytes = sizeof(double2) * (size_t)N;
    long cap_rows = (long)(RTLWS_LONG_WORKSPACE_CAP / frame_bytes) / K;
    if (cap_rows < 1) cap_rows = 1;                                      // always one row's k_avg frames
    long rows = max_frames < 1 ? 1 : (max_frames + K - 1) / K;
    if (rows > cap_rows) rows = cap_rows;
    p->frames_in_flight = rows * K;
    if (p->frames_in_flight > (long)(INT_MAX >> (p->log2n - 13))) {      // pass A's grid: frames * N / 8192 workgroups
        g_err = "rtlws_long_open: k_avg too large for one launch";
        delete p;
        return nullptr;
    }
    p->ws_bytes = frame_bytes * (size_t)p->frames_in_flight;

    hipError_t err = hipSetDevice(p->device);
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&p->ws), p->ws_bytes);
    if (err != hipSuccess) {
        set_err("rtlws_long_open: workspace", err);
        destroy(p);
        return nullptr;
    }
    // W_1024^e for the sub-transforms; W_N^j = twh[j >> 10] * twl[j & 1023]
    if (!upload(&p->twc, roots(1024, 1, 1024)) || !upload(&p->twl, roots(N, 1, 1 << TW_SPLIT_LOG2)) ||
        !upload(&p->twh, roots(N, 1 << TW_SPLIT_LOG2, (int)(N >> TW_SPLIT_LOG2)))) {
        destroy(p);
        return nullptr;
    }
    // 128 KiB of LDS per workgroup: the opt-in happens here, so that a launch -- under hipGraph capture too --
    // makes no other runtime call
    err = prepare_long(p->log2n, desc->input, p->rows_kind, p->device);
    if (err != hipSuccess) {
        set_err("rtlws_long_open: LDS opt-in", err);
        destroy(p);
        return nullptr;
    }
    return p;
}

size_t rtlws_long_workspace_bytes(const rtlws_long_plan* plan) { return plan ? plan->ws_bytes : 0; }

int rtlws_long_run(rtlws_long_plan* plan, const void* d_in, long nframes, void* d_out, void* stream)
{
    using namespace rtlws::lng;
    g_err.clear();
    if (!plan) {
        g_err = "rtlws_long_run: null plan";
        return -1;
    }
    const rtlws_spectra_desc& d = plan->desc;
    if (nframes < 0 || nframes % d.k_avg) {
        g_err = "rtlws_long_run: nframes must be a non-negative multiple of k_avg";
        return -1;
    }
    if (nframes == 0) return 0;
    if (!d_in || !d_out) {
        g_err = "rtlws_long_run: null pointer";
        return -1;
    }
    const unsigned out_align = plan->rows_kind == ROWS_F64 ? 7u : 3u;
    if ((reinterpret_cast<uintptr_t>(d_in) & 7u) || (reinterpret_cast<uintptr_t>(d_out) & out_align)) {
        g_err = "rtlws_long_run: d_in must be 8-byte aligned, d_out 8-byte (4-byte for f32 rows and payload bytes)";
        return -1;
    }
    hipError_t err = hipSetDevice(plan->device);
    if (err != hipSuccess) {
        set_err("rtlws_long_run: hipSetDevice", err);
        return -3;
    }
    hipStream_t st = stream_of(plan->eng, stream);

    LongParams p;
    std::memset(&p, 0, sizeof p);
    p.ws = plan->ws;
    p.twc = plan->twc;
    p.twl = plan->twl;
    p.twh = plan->twh;
    p.log2n1 = log2_n1(plan->log2n);
    p.log2n2 = log2_n2(plan->log2n);
    p.k_avg = d.k_avg;
    p.out_mode = d.output;
    p.lin_gain = std::pow(10.0, (double)(d.gain_db / 10));               // src/cbb_main.c:112: C integer division
    p.in_scale = d.input != RTLWS_IN_RF32 ? 0.0078125 : 1.0;

    const size_t N = (size_t)d.n_fft;
    const size_t in_bytes = N * (d.input == RTLWS_IN_CU8 ? 2 : d.input == RTLWS_IN_CS32 ? 8 : 4);
    const size_t row_bytes = N * (plan->rows_kind == ROWS_F64 ? 8 : plan->rows_kind == ROWS_F32 ? 4 : 1);
    // groups of whole rows that fit the workspace, one after the other on the stream
    for (long done = 0; done < nframes; done += plan->frames_in_flight) {
        const long frames = nframes - done < plan->frames_in_flight ? nframes - done : plan->frames_in_flight;
        p.in = static_cast<const char*>(d_in) + (size_t)done * in_bytes;
        p.out = static_cast<char*>(d_out) + (size_t)(done / d.k_avg) * row_bytes;
        err = launch_long_pass_a(p, d.input, frames, st);
        if (err == hipSuccess) err = launch_long_pass_b(p, plan->rows_kind, frames / d.k_avg, st);
        if (err != hipSuccess) {
            set_err("rtlws_long_run: kernel launch", err);
            return -3;
        }
    }
    return 0;
}

void rtlws_long_close(rtlws_long_plan* plan)
{
    if (plan) destroy(plan);
}

}  // extern "C"
