// pfbxc_shim.hip -- extern "C" glue of include/rtlws_pfbxc.h (librtlws_pfbxc.so): argument rules, geometry, the plan
// (pfb_plan.h's text, as librtlws_pfb.so's and librtlws_pfbspec.so's plans), the launch.  The engine (device, stream)
// is librtlws_hip.so's; nothing here reads the environment, and nothing of a run is computed on the host: without a
// device there is no plan.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <cstdio>
#include <string>

#include "pfb_plan.h"
#include "pfbxc.h"
#include "rtlws_pfb.h"
#include "rtlws_pfbxc.h"

struct rtlws_pfbxc_plan {
    rtlws_engine* engine;
    int device;
    int log2_m, taps_per_branch, ninputs;
    int16_t* d_taps;
    float2* d_tw;
};

namespace {

using namespace rtlws::pfbxc;
using rtlws::pfb::MAX_LOG2_M;
using rtlws::pfb::MAX_TAPS;
using rtlws::pfb::MIN_LOG2_M;
using rtlws::pfb::THREADS;

static_assert(MIN_LOG2_M == RTLWS_PFB_MIN_LOG2_CHANNELS && MAX_LOG2_M == RTLWS_PFB_MAX_LOG2_CHANNELS &&
                  MAX_TAPS == RTLWS_PFB_MAX_TAPS && MAX_K_AVG == RTLWS_PFBXC_MAX_K_AVG && MIN_INPUTS == RTLWS_PFBXC_MIN_INPUTS &&
                  MAX_INPUTS == RTLWS_PFBXC_MAX_INPUTS,
              "rtlws_pfbxc.h, rtlws_pfb.h and pfbxc.h disagree");

thread_local std::string g_err;

int fail(const char* fn, const char* why, int rc)
{
    g_err = std::string(fn) + ": " + why;
    return rc;
}

int fail_hip(const char* fn, const char* what, hipError_t e)
{
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s: %s", fn, what, hipGetErrorString(e));
    g_err = buf;
    return -3;
}

// why a plan's shape is not served, or nullptr
const char* why_not_plan(int k, int taps, int ninputs)
{
    if (k < MIN_LOG2_M || k > MAX_LOG2_M) return "log2_channels must be 4 .. 10";
    if (taps < 1 || taps > MAX_TAPS) return "taps_per_branch must be 1 .. 32";
    if (ninputs < MIN_INPUTS || ninputs > MAX_INPUTS) return "ninputs must be 2 .. 4";
    return nullptr;
}

// why a run's shape is not served, or nullptr
const char* why_not(int k, int taps, int hop, int k_avg, int ninputs, long nspectra)
{
    if (const char* why = why_not_plan(k, taps, ninputs)) return why;
    if (hop != 1 << k && hop != 1 << (k - 1)) return "hop must be M or M / 2";
    if (k_avg < 1 || k_avg > MAX_K_AVG) return "k_avg must be 1 .. 65536";
    if (nspectra < 0) return "nspectra must be >= 0";
    if (nspectra > (long)INT_MAX * spectra_per_block(k, k_avg)) return "more spectra than one grid holds";
    return nullptr;
}

}  // namespace

extern "C" {

const char* rtlws_pfbxc_last_error(void) { return g_err.c_str(); }

int rtlws_pfbxc_supported(int log2_channels, int taps_per_branch, int hop, int k_avg, int ninputs)
{
    g_err.clear();
    const char* why = why_not(log2_channels, taps_per_branch, hop, k_avg, ninputs, 0);
    if (why) fail("rtlws_pfbxc", why, 0);
    return why ? 0 : 1;
}

long rtlws_pfbxc_samples_needed(int log2_channels, int taps_per_branch, int hop, int k_avg, long nspectra)
{
    g_err.clear();
    if (const char* why = why_not(log2_channels, taps_per_branch, hop, k_avg, MIN_INPUTS, nspectra))
        return fail("rtlws_pfbxc_samples_needed", why, -1);
    if (nspectra == 0) return 0;
    return (nspectra * k_avg - 1) * hop + (long)taps_per_branch * (1L << log2_channels);
}

int rtlws_pfbxc_pair_index(int ninputs, int a, int b)
{
    if (ninputs < MIN_INPUTS || ninputs > MAX_INPUTS || a < 0 || a >= b || b >= ninputs) return -1;
    // the pairs (a', b') with a' < a come first: sum_{a' < a} (ninputs - 1 - a')
    return a * (2 * ninputs - a - 1) / 2 + (b - a - 1);
}

int rtlws_pfbxc_grid(int log2_channels, int taps_per_branch, int hop, int k_avg, int ninputs, long nspectra, int* blocks,
                     int* threads, int* lds_bytes, int* spectra_per_block_out)
{
    g_err.clear();
    if (const char* why = why_not(log2_channels, taps_per_branch, hop, k_avg, ninputs, nspectra))
        return fail("rtlws_pfbxc_grid", why, -1);
    const int g = spectra_per_block(log2_channels, k_avg);
    if (blocks) *blocks = (int)((nspectra + g - 1) / g);
    if (threads) *threads = THREADS;
    if (lds_bytes) *lds_bytes = rtlws::pfbxc::lds_bytes(log2_channels, ninputs);
    if (spectra_per_block_out) *spectra_per_block_out = g;
    return 0;
}

rtlws_pfbxc_plan* rtlws_pfbxc_open(rtlws_engine* e, int log2_channels, int taps_per_branch, const int16_t* taps, int ninputs)
{
    const char* fn = "rtlws_pfbxc_open";
    g_err.clear();
    if (const char* why = why_not_plan(log2_channels, taps_per_branch, ninputs)) {
        fail(fn, why, -1);
        return nullptr;
    }
    if (!taps) {
        fail(fn, "null taps", -1);
        return nullptr;
    }
    if (!e) {
        fail(fn, "null engine (no usable HIP device: there is no CPU path)", -1);
        return nullptr;
    }
    const int device = rtlws_engine_device(e);
    hipError_t err = hipSetDevice(device);
    if (err != hipSuccess) {
        fail_hip(fn, "hipSetDevice", err);
        return nullptr;
    }
    int16_t* d_taps = nullptr;
    float2* d_tw = nullptr;
    err = rtlws::pfb::upload_plan_arrays(log2_channels, taps_per_branch, taps, &d_taps, &d_tw);
    if (err == hipSuccess) {
        err = prepare_pfbxc(log2_channels, ninputs);
        if (err != hipSuccess) rtlws::pfb::free_plan_arrays(d_taps, d_tw);
    }
    if (err != hipSuccess) {
        fail_hip(fn, "the taps, the table or the kernel", err);
        return nullptr;
    }
    return new rtlws_pfbxc_plan{e, device, log2_channels, taps_per_branch, ninputs, d_taps, d_tw};
}

void rtlws_pfbxc_close(rtlws_pfbxc_plan* p)
{
    if (!p) return;
    if (hipSetDevice(p->device) == hipSuccess) rtlws::pfb::free_plan_arrays(p->d_taps, p->d_tw);
    delete p;
}

int rtlws_pfbxc_run(rtlws_pfbxc_plan* p, const void* const* d_iq_cu8, long nspectra, int hop, int k_avg, int shifted,
                    float* d_auto, long auto_stride, float* d_cross, long cross_stride, void* stream)
{
    const char* fn = "rtlws_pfbxc_run";
    g_err.clear();
    // what needs no plan: the hop is a power of two 8 .. 1024, a row holds at least 16 values, a workgroup at most
    // 256 / k_avg spectra
    if (hop < 8 || hop > 1 << MAX_LOG2_M || (hop & (hop - 1))) return fail(fn, "hop must be M or M / 2", -1);
    if (k_avg < 1 || k_avg > MAX_K_AVG) return fail(fn, "k_avg must be 1 .. 65536", -1);
    if (shifted != 0 && shifted != 1) return fail(fn, "shifted must be 0 or 1", -1);
    if (nspectra < 0) return fail(fn, "nspectra must be >= 0", -1);
    if (nspectra > (long)INT_MAX * spectra_per_block(MIN_LOG2_M, k_avg)) return fail(fn, "more spectra than one grid holds", -1);
    if (auto_stride < 1L << MIN_LOG2_M) return fail(fn, "auto_stride must be >= M", -1);
    if (auto_stride % 4) return fail(fn, "auto_stride must be a multiple of 4", -1);
    if (cross_stride < 1L << MIN_LOG2_M) return fail(fn, "cross_stride must be >= M", -1);
    if (cross_stride % 2) return fail(fn, "cross_stride must be a multiple of 2", -1);
    if (nspectra > 0 && (!d_iq_cu8 || !d_auto || !d_cross)) return fail(fn, "null pointer", -1);
    if (reinterpret_cast<uintptr_t>(d_auto) & 15u) return fail(fn, "d_auto must be 16-byte aligned", -1);
    if (reinterpret_cast<uintptr_t>(d_cross) & 15u) return fail(fn, "d_cross must be 16-byte aligned", -1);
    if (!p) return fail(fn, "null plan (no usable HIP device: there is no CPU path)", -1);
    // what the plan decides; still before anything is asked of the device
    if (const char* why = why_not(p->log2_m, p->taps_per_branch, hop, k_avg, p->ninputs, nspectra)) return fail(fn, why, -1);
    if (auto_stride < 1L << p->log2_m) return fail(fn, "auto_stride must be >= M", -1);
    if (cross_stride < 1L << p->log2_m) return fail(fn, "cross_stride must be >= M", -1);
    if (nspectra == 0) return 0;
    for (int a = 0; a < p->ninputs; ++a) {
        if (!d_iq_cu8[a]) return fail(fn, "null pointer among the captures", -1);
        if (reinterpret_cast<uintptr_t>(d_iq_cu8[a]) & 15u) return fail(fn, "every capture must be 16-byte aligned", -1);
    }

    hipError_t err = hipSetDevice(p->device);
    if (err != hipSuccess) return fail_hip(fn, "hipSetDevice", err);
    hipStream_t st = stream == RTLWS_STREAM_DEFAULT ? hipStreamLegacy
                     : stream                       ? reinterpret_cast<hipStream_t>(stream)
                                                    : reinterpret_cast<hipStream_t>(rtlws_engine_stream(p->engine));
    XcParams xp;
    xp.bank.src = nullptr;
    xp.bank.out = nullptr;
    xp.bank.taps = p->d_taps;
    xp.bank.tw = p->d_tw;
    xp.bank.nframes = nspectra * k_avg;
    xp.bank.first = 0;
    xp.bank.out_stride = 0;
    xp.bank.taps_per_branch = p->taps_per_branch;
    xp.bank.half_hop = hop != 1 << p->log2_m;
    xp.bank.layout = 0;
    for (int a = 0; a < MAX_INPUTS; ++a) xp.src[a] = a < p->ninputs ? d_iq_cu8[a] : nullptr;
    xp.autos = d_auto;
    xp.cross = reinterpret_cast<float2*>(d_cross);
    xp.nspectra = nspectra;
    xp.auto_stride = auto_stride;
    xp.cross_stride = cross_stride;
    xp.k_avg = k_avg;
    xp.shift = shifted ? 1 << (p->log2_m - 1) : 0;
    err = launch_pfbxc(p->log2_m, p->ninputs, xp, st);
    if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
    return 0;
}

}  // extern "C"
