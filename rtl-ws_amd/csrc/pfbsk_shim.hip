// pfbsk_shim.hip -- extern "C" glue of include/rtlws_pfbsk.h (librtlws_pfbsk.so): argument rules, geometry, the two
// host helpers, the plan (pfb_plan.h's text, as librtlws_pfb.so's plan), the launch.  The engine (device, stream) is
// librtlws_hip.so's; nothing here reads the environment, and nothing of a run is computed on the host: without a
// device there is no plan.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pfb_plan.h"
#include "pfbsk.h"
#include "rtlws_pfb.h"
#include "rtlws_pfbsk.h"

struct rtlws_pfbsk_plan : rtlws::pfb::Plan {};

namespace {

using namespace rtlws::pfb;
using namespace rtlws::pfbsk;

static_assert(MIN_LOG2_M == RTLWS_PFB_MIN_LOG2_CHANNELS && MAX_LOG2_M == RTLWS_PFB_MAX_LOG2_CHANNELS &&
                  MAX_TAPS == RTLWS_PFB_MAX_TAPS && MAX_K_AVG == RTLWS_PFBSK_MAX_K_AVG && MAX_NSUB == RTLWS_PFBSK_MAX_NSUB &&
                  OUT_SUM == RTLWS_OUT_POWER_SUM && OUT_DB == RTLWS_OUT_MEAN_DB && OUT_PAYLOAD == RTLWS_OUT_PAYLOAD_U8,
              "rtlws_pfbsk.h, rtlws_pfb.h, rtlws_hip.h and pfbsk.h disagree");

// ---- this library's own rules, each worded once ----
const char* why_not_nsub(int nsub) { return nsub < 1 || nsub > MAX_NSUB ? "nsub must be 1 .. 65535" : nullptr; }

const char* why_not_power_scale(float s) { return std::isfinite(s) && s > 0.0f ? nullptr : "power_scale must be finite and > 0"; }

const char* why_not_ratios(float lo, float hi)
{
    return std::isfinite(lo) && lo >= 0.0f && hi >= lo ? nullptr
                                                       : "the ratio bounds must be 0 <= ratio_lo <= ratio_hi, ratio_lo finite";
}

// why a run's shape is not served, or nullptr: the bank, the hop, k_avg, then nsub, then the rows (a workgroup a row)
const char* why_not(int k, int taps, int hop, int k_avg, int nsub, long nspectra)
{
    if (const char* why = why_not_bank(k, taps)) return why;
    if (const char* why = why_not_hop(k, hop)) return why;
    if (const char* why = why_not_k_avg(k_avg)) return why;
    if (const char* why = why_not_nsub(nsub)) return why;
    return why_not_count(nspectra, ROWS_PER_BLOCK, true);
}

bool known_output(int output) { return output == OUT_SUM || output == OUT_DB || output == OUT_PAYLOAD; }

// a buffer's stride before the plan is looked at: a row holds at least 16 values
const char* why_not_stride(long stride, bool bytes, const char* small, const char* multiple)
{
    if (stride < 1L << MIN_LOG2_M) return small;
    return stride % (bytes ? 16 : 4) ? multiple : nullptr;
}

}  // namespace

extern "C" {

const char* rtlws_pfbsk_last_error(void) { return g_err.c_str(); }

int rtlws_pfbsk_supported(int log2_channels, int taps_per_branch, int hop, int k_avg, int nsub, int output)
{
    const char* why = why_not(log2_channels, taps_per_branch, hop, k_avg, nsub, 0);
    if (!why && !known_output(output)) why = "unknown output";
    return supported("rtlws_pfbsk", why);
}

long rtlws_pfbsk_samples_needed(int log2_channels, int taps_per_branch, int hop, int k_avg, int nsub, long nspectra)
{
    g_err.clear();
    if (const char* why = why_not(log2_channels, taps_per_branch, hop, k_avg, nsub, nspectra))
        return fail("rtlws_pfbsk_samples_needed", why, -1);
    if (nspectra == 0) return 0;
    return (nspectra * nsub * k_avg - 1) * hop + (long)taps_per_branch * (1L << log2_channels);
}

int rtlws_pfbsk_grid(int log2_channels, int taps_per_branch, int hop, int k_avg, int nsub, long nspectra, int* blocks,
                     int* threads, int* lds_bytes, int* rows_per_block)
{
    g_err.clear();
    if (const char* why = why_not(log2_channels, taps_per_branch, hop, k_avg, nsub, nspectra))
        return fail("rtlws_pfbsk_grid", why, -1);
    if (blocks) *blocks = (int)((nspectra + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
    if (threads) *threads = THREADS;
    if (lds_bytes) *lds_bytes = rtlws::pfbsk::lds_bytes(log2_channels);
    if (rows_per_block) *rows_per_block = ROWS_PER_BLOCK;
    return 0;
}

float rtlws_pfbsk_power_scale(int log2_channels, int taps_per_branch, const int16_t* taps)
{
    const char* fn = "rtlws_pfbsk_power_scale";
    g_err.clear();
    if (const char* why = why_not_bank(log2_channels, taps_per_branch)) return (float)fail(fn, why, 0);
    if (!taps) return (float)fail(fn, "null taps", 0);
    long sum = 0;                                     // <= 32 * 1024 * 32768 = 2^30
    for (long i = 0, n = (long)taps_per_branch << log2_channels; i < n; ++i) sum += taps[i] < 0 ? -(long)taps[i] : taps[i];
    int e = 0;                                        // ceil(log2(128 sum)): the smallest e with 2^e >= 128 sum
    while ((1L << e) < 128 * sum) ++e;
    return sum ? std::ldexp(1.0f, -2 * e) : 1.0f;
}

int rtlws_pfbsk_bounds(int k_avg, double sk_lo, double sk_hi, float* ratio_lo, float* ratio_hi)
{
    const char* fn = "rtlws_pfbsk_bounds";
    g_err.clear();
    if (k_avg < 2 || k_avg > MAX_K_AVG) return fail(fn, "k_avg must be 2 .. 65536: one frame has no kurtosis", -1);
    if (!(sk_lo >= 0.0 && sk_lo <= sk_hi)) return fail(fn, "the thresholds must be 0 <= sk_lo <= sk_hi", -1);
    const double g = (double)(k_avg - 1) / (double)(k_avg + 1);
    if (ratio_lo) *ratio_lo = (float)(1.0 + sk_lo * g);
    if (ratio_hi) *ratio_hi = (float)(1.0 + sk_hi * g);
    return 0;
}

rtlws_pfbsk_plan* rtlws_pfbsk_open(rtlws_engine* e, int log2_channels, int taps_per_branch, const int16_t* taps)
{
    g_err.clear();
    return open_plan<rtlws_pfbsk_plan>("rtlws_pfbsk_open", why_not_bank(log2_channels, taps_per_branch), e, log2_channels,
                                       taps_per_branch, taps, prepare_pfbsk);
}

void rtlws_pfbsk_close(rtlws_pfbsk_plan* p) { close_plan(p); }

int rtlws_pfbsk_run(rtlws_pfbsk_plan* p, const void* d_iq_cu8, long nspectra, int hop, int k_avg, int nsub, float power_scale,
                    float ratio_lo, float ratio_hi, int output, int shifted, float scale, void* d_clean, long clean_stride,
                    uint32_t* d_kept, long kept_stride, float* d_s1, float* d_s2, long sub_stride, void* stream)
{
    const char* fn = "rtlws_pfbsk_run";
    g_err.clear();
    // what needs no plan: the hop is a power of two 8 .. 1024, a row holds at least 16 values
    if (const char* why = why_not_any_hop(hop)) return fail(fn, why, -1);
    if (const char* why = why_not_k_avg(k_avg)) return fail(fn, why, -1);
    if (const char* why = why_not_nsub(nsub)) return fail(fn, why, -1);
    if (!known_output(output)) return fail(fn, "unknown output", -1);
    if (shifted != 0 && shifted != 1) return fail(fn, "shifted must be 0 or 1", -1);
    if (output != OUT_SUM && !(std::isfinite(scale) && scale > 0.0f)) return fail(fn, "scale must be finite and > 0", -1);
    if (const char* why = why_not_power_scale(power_scale)) return fail(fn, why, -1);
    if (const char* why = why_not_ratios(ratio_lo, ratio_hi)) return fail(fn, why, -1);
    if (const char* why = why_not_count(nspectra, ROWS_PER_BLOCK, true)) return fail(fn, why, -1);
    const bool bytes = output == OUT_PAYLOAD, subs = d_s1 || d_s2;
    if (const char* why = why_not_stride(clean_stride, bytes, "clean_stride must be >= M",
                                         bytes ? "clean_stride must be a multiple of 16 for byte rows"
                                               : "clean_stride must be a multiple of 4 for f32 rows"))
        return fail(fn, why, -1);
    if (d_kept)
        if (const char* why = why_not_stride(kept_stride, false, "kept_stride must be >= M",
                                             "kept_stride must be a multiple of 4 for uint32 rows"))
            return fail(fn, why, -1);
    if (subs)
        if (const char* why = why_not_stride(sub_stride, false, "sub_stride must be >= M",
                                             "sub_stride must be a multiple of 4 for f32 rows"))
            return fail(fn, why, -1);
    if (!d_s1 != !d_s2) return fail(fn, "d_s1 and d_s2 must both be given or both be null", -1);
    if (nspectra > 0 && (!d_iq_cu8 || !d_clean)) return fail(fn, "null pointer", -1);
    if (reinterpret_cast<uintptr_t>(d_iq_cu8) & 15u) return fail(fn, "d_iq_cu8 must be 16-byte aligned", -1);
    if (reinterpret_cast<uintptr_t>(d_clean) & 15u) return fail(fn, "d_clean must be 16-byte aligned", -1);
    if (reinterpret_cast<uintptr_t>(d_kept) & 15u) return fail(fn, "d_kept must be 16-byte aligned", -1);
    if ((reinterpret_cast<uintptr_t>(d_s1) | reinterpret_cast<uintptr_t>(d_s2)) & 15u)
        return fail(fn, "d_s1 and d_s2 must be 16-byte aligned", -1);
    if (!p) return fail(fn, "null plan (no usable HIP device: there is no CPU path)", -1);
    // what the plan's shape decides; still before anything is asked of the device
    if (const char* why = why_not(p->log2_m, p->taps_per_branch, hop, k_avg, nsub, nspectra)) return fail(fn, why, -1);
    const long M = 1L << p->log2_m;
    if (clean_stride < M) return fail(fn, "clean_stride must be >= M", -1);
    if (d_kept && kept_stride < M) return fail(fn, "kept_stride must be >= M", -1);
    if (subs && sub_stride < M) return fail(fn, "sub_stride must be >= M", -1);
    if (nspectra == 0) return 0;

    hipError_t err = hipSetDevice(p->device);
    if (err != hipSuccess) return fail_hip(fn, "hipSetDevice", err);
    SkParams sp;
    sp.bank = bank_params(*p, hop, nspectra * nsub * k_avg);
    sp.bank.src = d_iq_cu8;
    sp.clean = d_clean;
    sp.kept = d_kept;
    sp.s1 = d_s1;
    sp.s2 = d_s2;
    sp.nspectra = nspectra;
    sp.clean_stride = clean_stride;
    sp.kept_stride = kept_stride;
    sp.sub_stride = sub_stride;
    sp.k_avg = k_avg;
    sp.nsub = nsub;
    sp.output = output;
    sp.shift = shifted ? 1 << (p->log2_m - 1) : 0;
    sp.scale = scale;
    sp.power_scale = power_scale;
    sp.ratio_lo = ratio_lo;
    sp.ratio_hi = ratio_hi;
    err = launch_pfbsk(p->log2_m, sp, stream_of(p->engine, stream));
    if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
    return 0;
}

}  // extern "C"
