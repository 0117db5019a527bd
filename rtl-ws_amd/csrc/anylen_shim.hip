// anylen_shim.hip -- extern "C" glue of include/rtlws_anylen.h (librtlws_anylen.so): plans, tables, workspaces, launches.
// The engine (device, stream) is librtlws_hip.so's; nothing here reads the environment.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rtlws_anylen.h"
#include "shim_common.h"
#include "spectrum_anylen.h"

namespace {

void set_err(const char* what, hipError_t e)
{
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    g_err = buf;
}

// why a descriptor is not served, or nullptr
const char* why_not(const rtlws_spectra_desc* d)
{
    using namespace rtlws::anylen;
    if (!d) return "null descriptor";
    if (d->n_fft < MIN_N) return "n_fft must be at least 2";
    if (d->n_fft > MAX_N) return "n_fft must be at most 2^19 = 524288 (the convolution runs at 2^20 points, the longest transform)";
    if (d->k_avg < 1) return "k_avg must be >= 1";
    if (d->input < RTLWS_IN_CU8 || d->input > RTLWS_IN_RF32) return "unknown input kind";
    if (d->window == RTLWS_WIN_HANN) return "the Hann window is not built for rtlws_anylen.h (rectangular frames only)";
    if (d->window != RTLWS_WIN_RECT) return "unknown window";
    if (d->output < RTLWS_OUT_POWER_SUM || d->output > RTLWS_OUT_PAYLOAD_U8) return "unknown output kind";
    if (d->cic_r > 1) return "no CIC stage in front of rtlws_anylen.h's frames (cic_r must be 0 or 1)";
    if (d->cic_r < 0) return "cic_r must be 0 or 1";
    if (d->flags & ~RTLWS_FLAG_ROWS_F32) return "unknown flag (only RTLWS_FLAG_ROWS_F32)";
    return nullptr;
}

const long double PI_L = 3.141592653589793238462643383279502884L;

// w[n] = exp(-i pi n^2 / N), n < N: the angle from the exact integer q = n^2 mod 2N (n^2 < 2^38), rounded once
std::vector<double2> chirp(long N)
{
    std::vector<double2> w((size_t)N);
    for (long n = 0; n < N; ++n) {
        const long q = (long)((unsigned long long)n * (unsigned long long)n % (unsigned long long)(2 * N));
        const long double a = -PI_L * (long double)q / (long double)N;
        w[(size_t)n] = make_double2((double)cosl(a), (double)sinl(a));
    }
    return w;
}

}  // namespace

struct rtlws_anylen_plan {
    rtlws_engine* eng = nullptr;
    int device = 0;
    rtlws_spectra_desc desc;
    int log2m = 0, rows_kind = 0;
    long frames_in_flight = 0;                  // a multiple of k_avg
    size_t ws_bytes = 0;                        // both workspaces
    double2 *ws1 = nullptr, *ws2 = nullptr, *twc = nullptr, *twl = nullptr, *twh = nullptr, *chirp = nullptr, *bhat = nullptr;
};

namespace {

bool upload(double2** dst, const std::vector<double2>& src, const char* what)
{
    hipError_t e = hipMalloc(reinterpret_cast<void**>(dst), src.size() * sizeof(double2));
    if (e == hipSuccess) e = hipMemcpy(*dst, src.data(), src.size() * sizeof(double2), hipMemcpyHostToDevice);
    if (e != hipSuccess) set_err(what, e);
    return e == hipSuccess;
}

void destroy(rtlws_anylen_plan* p)
{
    (void)hipSetDevice(p->device);
    (void)hipFree(p->ws1);
    (void)hipFree(p->ws2);
    (void)hipFree(p->twc);
    (void)hipFree(p->twl);
    (void)hipFree(p->twh);
    (void)hipFree(p->chirp);
    (void)hipFree(p->bhat);
    delete p;
}

rtlws::anylen::AnyParams params_of(const rtlws_anylen_plan* plan)
{
    using namespace rtlws::lng;
    rtlws::anylen::AnyParams p;
    std::memset(&p, 0, sizeof p);
    const rtlws_spectra_desc& d = plan->desc;
    p.ws1 = plan->ws1;
    p.ws2 = plan->ws2;
    p.twc = plan->twc;
    p.twl = plan->twl;
    p.twh = plan->twh;
    p.chirp = plan->chirp;
    p.bhat = plan->bhat;
    p.log2n1 = log2_n1(plan->log2m);
    p.log2n2 = log2_n2(plan->log2m);
    p.n = d.n_fft;
    p.k_avg = d.k_avg;
    p.out_mode = d.output;
    p.lin_gain = std::pow(10.0, (double)(d.gain_db / 10));               // src/cbb_main.c:112: C integer division
    p.in_scale = d.input != RTLWS_IN_RF32 ? 0.0078125 : 1.0;
    return p;
}

// Bhat = FFT_M(b) / M in natural order, on the device with the plan's own forward passes: conj(b) goes to the second
// workspace (pass 3 loads the conjugate of what it finds there: b), pass 3 and pass 2 run on one frame with a table
// of the constant 1/M in Bhat's place, and pass 2's output -- the second workspace again -- is the table.
bool make_bhat(rtlws_anylen_plan* plan)
{
    using namespace rtlws::anylen;
    const long N = plan->desc.n_fft, M = 1L << plan->log2m;
    const std::vector<double2> w = chirp(N);
    std::vector<double2> cb((size_t)M, make_double2(0.0, 0.0));          // conj(b): b[n] = b[M - n] = conj(w[n])
    for (long n = 0; n < N; ++n) {
        cb[(size_t)n] = w[(size_t)n];
        if (n) cb[(size_t)(M - n)] = w[(size_t)n];
    }
    const std::vector<double2> scale((size_t)M, make_double2(1.0 / (double)M, 0.0));
    double2* d_scale = nullptr;
    if (!upload(&plan->chirp, w, "rtlws_anylen_open: chirp table") || !upload(&d_scale, scale, "rtlws_anylen_open: chirp transform"))
        return false;
    hipError_t err = hipMalloc(reinterpret_cast<void**>(&plan->bhat), (size_t)M * sizeof(double2));
    if (err == hipSuccess) err = hipMemcpy(plan->ws2, cb.data(), (size_t)M * sizeof(double2), hipMemcpyHostToDevice);
    if (err == hipSuccess) {
        hipStream_t st = reinterpret_cast<hipStream_t>(rtlws_engine_stream(plan->eng));
        AnyParams p = params_of(plan);
        p.bhat = d_scale;
        err = launch_pass_a_ws(p, 1, st);
        if (err == hipSuccess) err = launch_pass_b_cplx(p, 1, st);
        if (err == hipSuccess) err = hipMemcpyAsync(plan->bhat, plan->ws2, (size_t)M * sizeof(double2), hipMemcpyDeviceToDevice, st);
        const hipError_t sync = hipStreamSynchronize(st);
        if (err == hipSuccess) err = sync;
    }
    (void)hipFree(d_scale);
    if (err != hipSuccess) set_err("rtlws_anylen_open: chirp transform", err);
    return err == hipSuccess;
}

}  // namespace

extern "C" {

const char* rtlws_anylen_last_error(void) { return g_err.c_str(); }

int rtlws_anylen_supported(const rtlws_spectra_desc* desc)
{
    return supported("rtlws_anylen", why_not(desc));
}

int rtlws_anylen_conv_log2(const rtlws_spectra_desc* desc)
{
    return rtlws_anylen_supported(desc) ? rtlws::anylen::conv_log2(desc->n_fft) : -1;
}

rtlws_anylen_plan* rtlws_anylen_open(rtlws_engine* e, const rtlws_spectra_desc* desc, long max_frames)
{
    using namespace rtlws::lng;
    g_err.clear();
    if (!e) {
        g_err = "rtlws_anylen_open: null engine (no usable HIP device: there is no CPU path)";
        return nullptr;
    }
    if (const char* why = why_not(desc)) {
        g_err = std::string("rtlws_anylen_open: ") + why;
        return nullptr;
    }
    rtlws_anylen_plan* p = new rtlws_anylen_plan;
    p->eng = e;
    p->device = rtlws_engine_device(e);
    p->desc = *desc;
    p->log2m = rtlws::anylen::conv_log2(desc->n_fft);
    p->rows_kind = desc->output == RTLWS_OUT_PAYLOAD_U8 ? ROWS_U8 : (desc->flags & RTLWS_FLAG_ROWS_F32) ? ROWS_F32 : ROWS_F64;
    const long M = 1L << p->log2m, K = desc->k_avg;
    const size_t frame_bytes = 2 * sizeof(double2) * (size_t)M;         // both workspaces
    long cap_rows = (long)(RTLWS_LONG_WORKSPACE_CAP / frame_bytes) / K;
    if (cap_rows < 1) cap_rows = 1;                                      // always one row's k_avg frames
    long rows = max_frames < 1 ? 1 : (max_frames + K - 1) / K;
    if (rows > cap_rows) rows = cap_rows;
    p->frames_in_flight = rows * K;
    if (p->frames_in_flight > (long)(INT_MAX >> (p->log2m - 13))) {      // a pass's grid: frames * M / 8192 workgroups
        g_err = "rtlws_anylen_open: k_avg too large for one launch";
        delete p;
        return nullptr;
    }
    p->ws_bytes = frame_bytes * (size_t)p->frames_in_flight;

    hipError_t err = hipSetDevice(p->device);
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&p->ws1), p->ws_bytes / 2);
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&p->ws2), p->ws_bytes / 2);
    if (err != hipSuccess) {
        set_err("rtlws_anylen_open: workspace", err);
        destroy(p);
        return nullptr;
    }
    // W_1024^e for the sub-transforms; W_M^j = twh[j >> 10] * twl[j & 1023]
    if (!upload(&p->twc, roots(1024, 1, 1024), "rtlws_anylen_open: twiddle table") ||
        !upload(&p->twl, roots(M, 1, 1 << TW_SPLIT_LOG2), "rtlws_anylen_open: twiddle table") ||
        !upload(&p->twh, roots(M, 1 << TW_SPLIT_LOG2, (int)(M >> TW_SPLIT_LOG2)), "rtlws_anylen_open: twiddle table")) {
        destroy(p);
        return nullptr;
    }
    // 128 KiB of LDS per workgroup: the opt-in happens here, so that a launch -- under hipGraph capture too --
    // makes no other runtime call
    err = rtlws::anylen::prepare_anylen(p->log2m, desc->input, p->rows_kind, p->device);
    if (err != hipSuccess) {
        set_err("rtlws_anylen_open: LDS opt-in", err);
        destroy(p);
        return nullptr;
    }
    if (!make_bhat(p)) {
        destroy(p);
        return nullptr;
    }
    return p;
}

size_t rtlws_anylen_workspace_bytes(const rtlws_anylen_plan* plan) { return plan ? plan->ws_bytes : 0; }

int rtlws_anylen_run(rtlws_anylen_plan* plan, const void* d_in, long nframes, void* d_out, void* stream)
{
    using namespace rtlws::lng;
    using namespace rtlws::anylen;
    g_err.clear();
    if (!plan) {
        g_err = "rtlws_anylen_run: null plan";
        return -1;
    }
    const rtlws_spectra_desc& d = plan->desc;
    if (nframes < 0 || nframes % d.k_avg) {
        g_err = "rtlws_anylen_run: nframes must be a non-negative multiple of k_avg";
        return -1;
    }
    if (nframes == 0) return 0;
    if (!d_in || !d_out) {
        g_err = "rtlws_anylen_run: null pointer";
        return -1;
    }
    const size_t sample_bytes = d.input == RTLWS_IN_CU8 ? 2 : d.input == RTLWS_IN_CS32 ? 8 : 4;
    const unsigned out_align = plan->rows_kind == ROWS_F64 ? 7u : 3u;
    if ((reinterpret_cast<uintptr_t>(d_in) & (sample_bytes - 1)) || (reinterpret_cast<uintptr_t>(d_out) & out_align)) {
        g_err = "rtlws_anylen_run: d_in must be aligned to its sample (2, 8 or 4 bytes), d_out to 8 bytes (4 for f32 rows and payload bytes)";
        return -1;
    }
    hipError_t err = hipSetDevice(plan->device);
    if (err != hipSuccess) {
        set_err("rtlws_anylen_run: hipSetDevice", err);
        return -3;
    }
    hipStream_t st = stream_of(plan->eng, stream);

    AnyParams p = params_of(plan);
    const size_t N = (size_t)d.n_fft;
    const size_t in_bytes = N * sample_bytes;
    const size_t row_bytes = N * (plan->rows_kind == ROWS_F64 ? 8 : plan->rows_kind == ROWS_F32 ? 4 : 1);
    // groups of whole rows that fit the workspaces, one after the other on the stream
    for (long done = 0; done < nframes; done += plan->frames_in_flight) {
        const long frames = nframes - done < plan->frames_in_flight ? nframes - done : plan->frames_in_flight;
        p.in = static_cast<const char*>(d_in) + (size_t)done * in_bytes;
        p.out = static_cast<char*>(d_out) + (size_t)(done / d.k_avg) * row_bytes;
        err = launch_pass_a_in(p, d.input, frames, st);
        if (err == hipSuccess) err = launch_pass_b_cplx(p, frames, st);
        if (err == hipSuccess) err = launch_pass_a_ws(p, frames, st);
        if (err == hipSuccess) err = launch_pass_b_pow(p, plan->rows_kind, frames / d.k_avg, st);
        if (err != hipSuccess) {
            set_err("rtlws_anylen_run: kernel launch", err);
            return -3;
        }
    }
    return 0;
}

void rtlws_anylen_close(rtlws_anylen_plan* plan)
{
    if (plan) destroy(plan);
}

}  // extern "C"
