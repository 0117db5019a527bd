// periodlong_shim.hip -- extern "C" glue of include/rtlws_periodlong.h (librtlws_periodlong.so) over the family's rules
// and long-frame plan (period_plan.h): the geometry, the plan as it is, a run's launches by groups, the period of a bin.
// The engine (device, stream) is librtlws_hip.so's; nothing here reads the environment, and nothing of a run is computed
// on the host: without a device there is no plan.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "period_plan.h"
#include "periodlong.h"
#include "rtlws_periodlong.h"

// The tables and the workspace on the engine's device: the family's long-frame plan as it is (period_plan.h)
struct rtlws_periodlong_plan : rtlws::periodlong::Plan {};

using namespace rtlws::periodlong;

extern "C" {

const char* rtlws_periodlong_last_error(void) { return g_err.c_str(); }

int rtlws_periodlong_supported(int log2n, int levels, int norm, int seg, int klo)
{
    return supported("rtlws_periodlong", why_not_long_plan(log2n, levels, norm, seg, klo));
}

int rtlws_periodlong_geometry(int log2n, int levels, int norm, int seg, int klo, int ntrials, int* blocks, int* threads, int* lds,
                              int* nseg)
{
    const char* fn = "rtlws_periodlong_geometry";
    g_err.clear();
    if (const char* why = why_not_long_plan(log2n, levels, norm, seg, klo)) return fail(fn, why, -1);
    if (const char* why = why_not_ntrials(ntrials)) return fail(fn, why, -1);
    for (int st = 0; st < STAGES; ++st) {
        if (blocks) blocks[st] = stage_blocks(st, log2n) * ntrials;      // at most 512 * 65536
        if (threads) threads[st] = stage_threads(st, log2n);
        if (lds) lds[st] = stage_lds(st, log2n);
    }
    if (nseg) *nseg = (1 << (log2n - 1)) / seg;
    return 0;
}

void rtlws_periodlong_close(rtlws_periodlong_plan* p) { close_plan(p); }

rtlws_periodlong_plan* rtlws_periodlong_open(rtlws_engine* e, int log2n, int levels, int norm, int seg, int klo, int max_trials)
{
    return open_plan<rtlws_periodlong_plan>("rtlws_periodlong_open", why_not_long_plan(log2n, levels, norm, seg, klo), e, log2n, levels, norm, seg, klo,
                                            max_trials, [](rtlws_periodlong_plan&) { return hipSuccess; }, rtlws_periodlong_close);
}

size_t rtlws_periodlong_workspace_bytes(const rtlws_periodlong_plan* p) { return p ? p->ws_bytes : 0; }

int rtlws_periodlong_run(rtlws_periodlong_plan* p, const float* d_in, long in_stride, int ntrials, int nsamp, float* d_best,
                         int32_t* d_at, float* d_power, float* d_white, void* stream)
{
    const char* fn = "rtlws_periodlong_run";
    g_err.clear();
    // what needs no plan
    if (const char* why = why_not_run(ntrials, nsamp, MAX_LOG2N, WHY_LONG_NSAMP, in_stride, d_in, d_best, d_at, d_power, d_white)) return fail(fn, why, -1);
    if (!p) return fail(fn, NULL_PLAN, -1);
    // what the plan decides; still before anything is asked of the device
    if (nsamp > (1 << p->log2n)) return fail(fn, "nsamp must be at most the plan's N", -1);

    hipError_t err = hipSetDevice(p->device);
    if (err != hipSuccess) return fail_hip(fn, "hipSetDevice", err);
    Params kp = run_params(*p, d_in, in_stride, nsamp, d_best, d_at, d_power, d_white);
    const hipStream_t st = stream_of(p->engine, stream);
    err = for_groups(*p, ntrials, [&](int t0, int g) {
        kp.in = d_in + (long)t0 * in_stride;
        kp.trial0 = t0;
        return launch_group(kp, g, st);
    });
    if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
    return 0;
}

double rtlws_periodlong_samples(int log2n, int level, int k) { return samples("rtlws_periodlong_samples", why_not_long_log2n(log2n), log2n, level, k); }

}  // extern "C"
