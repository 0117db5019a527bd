// periodlong_shim.hip -- extern "C" glue of include/rtlws_periodlong.h (librtlws_periodlong.so): argument rules, the
// plan with its tables and workspace, the groups of a run, and the period of a bin.  The engine (device, stream) is
// librtlws_hip.so's; nothing here reads the environment, and nothing of a run is computed on the host: without a device
// there is no plan.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "periodlong.h"
#include "periodlong_plan.h"
#include "rtlws_periodlong.h"
#include "shim_common.h"

// The tables and the workspace on the engine's device
struct rtlws_periodlong_plan {
    rtlws_engine* engine;
    int device;
    int log2n, levels, log2norm, seg, klo;
    int group;                 // trials in flight
    size_t ws_bytes;
    float2* d_tables;          // tw [M], twist [M], tw_row [M2], tw256 [256]
    char* d_ws;                // z [group][M] float2, pw [group][M] float, sums [group][64] double
};

using namespace rtlws::periodlong;

extern "C" {

const char* rtlws_periodlong_last_error(void) { return g_err.c_str(); }

int rtlws_periodlong_supported(int log2n, int levels, int norm, int seg, int klo)
{
    g_err.clear();
    const char* why = why_not_plan(log2n, levels, norm, seg, klo);
    if (why) fail("rtlws_periodlong", why, 0);
    return why ? 0 : 1;
}

int rtlws_periodlong_geometry(int log2n, int levels, int norm, int seg, int klo, int ntrials, int* blocks, int* threads, int* lds,
                              int* nseg)
{
    const char* fn = "rtlws_periodlong_geometry";
    g_err.clear();
    if (const char* why = why_not_plan(log2n, levels, norm, seg, klo)) return fail(fn, why, -1);
    if (const char* why = why_not_ntrials(ntrials)) return fail(fn, why, -1);
    for (int st = 0; st < STAGES; ++st) {
        if (blocks) blocks[st] = stage_blocks(st, log2n) * ntrials;      // at most 512 * 65536
        if (threads) threads[st] = stage_threads(st, log2n);
        if (lds) lds[st] = stage_lds(st, log2n);
    }
    if (nseg) *nseg = (1 << (log2n - 1)) / seg;
    return 0;
}

rtlws_periodlong_plan* rtlws_periodlong_open(rtlws_engine* e, int log2n, int levels, int norm, int seg, int klo, int max_trials)
{
    const char* fn = "rtlws_periodlong_open";
    g_err.clear();
    const char* why = why_not_plan(log2n, levels, norm, seg, klo);
    if (!why && max_trials < 1) why = "max_trials must be >= 1";
    const int device = open_device(fn, why, e);
    if (device < 0) return nullptr;
    const std::vector<float2> t = host_tables(log2n);
    const int group = in_flight(log2n, max_trials);
    const size_t ws_bytes = (size_t)group * trial_bytes(log2n);
    float2* d_tables = nullptr;
    char* d_ws = nullptr;
    hipError_t err = hipMalloc(reinterpret_cast<void**>(&d_tables), t.size() * sizeof(float2));
    if (err == hipSuccess) err = hipMemcpy(d_tables, t.data(), t.size() * sizeof(float2), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&d_ws), ws_bytes);
    if (err == hipSuccess) err = prepare(log2n, device);
    if (err != hipSuccess) {
        if (d_tables) (void)hipFree(d_tables);
        if (d_ws) (void)hipFree(d_ws);
        fail_hip(fn, "the tables, the workspace or the kernels", err);
        return nullptr;
    }
    return new rtlws_periodlong_plan{e, device, log2n, levels, log2_of(norm), seg, klo, group, ws_bytes, d_tables, d_ws};
}

size_t rtlws_periodlong_workspace_bytes(const rtlws_periodlong_plan* p) { return p ? p->ws_bytes : 0; }

void rtlws_periodlong_close(rtlws_periodlong_plan* p)
{
    if (!p) return;
    if (hipSetDevice(p->device) == hipSuccess) {
        (void)hipFree(p->d_tables);
        (void)hipFree(p->d_ws);
    }
    delete p;
}

int rtlws_periodlong_run(rtlws_periodlong_plan* p, const float* d_in, long in_stride, int ntrials, int nsamp, float* d_best,
                         int32_t* d_at, float* d_power, float* d_white, void* stream)
{
    const char* fn = "rtlws_periodlong_run";
    g_err.clear();
    // what needs no plan
    if (const char* why = why_not_ntrials(ntrials)) return fail(fn, why, -1);
    if (nsamp < 1 || nsamp > (1 << MAX_LOG2N)) return fail(fn, "nsamp must be 1 .. 4194304", -1);
    if (in_stride < nsamp) return fail(fn, "in_stride must be >= nsamp", -1);
    if (in_stride % 4) return fail(fn, "in_stride must be a multiple of 4", -1);
    if (!d_in || !d_best || !d_at) return fail(fn, "null pointer", -1);
    if (reinterpret_cast<uintptr_t>(d_in) & 15u) return fail(fn, "d_in must be 16-byte aligned", -1);
    if (reinterpret_cast<uintptr_t>(d_best) & 3u) return fail(fn, "d_best must be 4-byte aligned", -1);
    if (reinterpret_cast<uintptr_t>(d_at) & 3u) return fail(fn, "d_at must be 4-byte aligned", -1);
    if (reinterpret_cast<uintptr_t>(d_power) & 3u) return fail(fn, "d_power must be 4-byte aligned", -1);
    if (reinterpret_cast<uintptr_t>(d_white) & 3u) return fail(fn, "d_white must be 4-byte aligned", -1);
    if (!p) return fail(fn, NULL_PLAN, -1);
    // what the plan decides; still before anything is asked of the device
    if (nsamp > (1 << p->log2n)) return fail(fn, "nsamp must be at most the plan's N", -1);

    hipError_t err = hipSetDevice(p->device);
    if (err != hipSuccess) return fail_hip(fn, "hipSetDevice", err);
    Params kp = plan_params(p->log2n, p->levels, p->log2norm, p->seg, p->klo, p->group, p->d_tables, p->d_ws);
    kp.best = d_best;
    kp.at = d_at;
    kp.power = d_power;
    kp.white = d_white;
    kp.in_stride = in_stride;
    kp.nsamp = nsamp;
    const hipStream_t st = stream_of(p->engine, stream);
    // groups of trials that fit the workspace, one after the other on the stream
    for (int t0 = 0; t0 < ntrials; t0 += p->group) {
        const int g = ntrials - t0 < p->group ? ntrials - t0 : p->group;
        kp.in = d_in + (long)t0 * in_stride;
        kp.trial0 = t0;
        err = launch_group(kp, g, st);
        if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
    }
    return 0;
}

double rtlws_periodlong_samples(int log2n, int level, int k)
{
    const char* fn = "rtlws_periodlong_samples";
    g_err.clear();
    if (log2n < MIN_LOG2N || log2n > MAX_LOG2N) return fail(fn, "log2n must be 16 .. 22", 0);
    if (level < 0 || level >= MAX_LEVELS) return fail(fn, "level must be 0 .. 4", 0);
    if (k < 1 || k > (1 << (log2n - 1)) - 1) return fail(fn, "k must be 1 .. N / 2 - 1", 0);
    return (double)(1L << (log2n + level)) / (double)k;
}

}  // extern "C"
