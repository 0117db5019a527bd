// fold_shim.hip -- extern "C" glue of include/rtlws_fold.h (librtlws_fold.so): argument rules, the block shape a bin
// count takes (fold.h), the plan and its tables, the launch, and the host's helpers (the exact step of a period, the
// phase at a later sample, the epoch-folding statistic).  The engine (device, stream) is librtlws_hip.so's; nothing here
// reads the environment, and nothing of a run is computed on the host: without a device there is no plan.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <limits>

#include "fold.h"
#include "rtlws_fold.h"
#include "search_plan.h"

// The two tables on the engine's device
struct rtlws_fold_plan : rtlws::search::Plan {
    int nperiods, nbins;
    long sub;
    uint64_t* d_tables;        // steps, then phases
};

namespace {

using namespace rtlws::fold;
namespace sp = rtlws::search;

static_assert(MAX_PERIODS == RTLWS_FOLD_MAX_PERIODS && MIN_BINS == RTLWS_FOLD_MIN_BINS && MAX_BINS == RTLWS_FOLD_MAX_BINS &&
                  MIN_SUB == RTLWS_FOLD_MIN_SUB && MAX_SUB == RTLWS_FOLD_MAX_SUB && MAX_TRIALS == RTLWS_FOLD_MAX_TRIALS &&
                  MAX_NSAMP == RTLWS_FOLD_MAX_NSAMP && MIN_BINS == sp::MIN_BINS && MAX_BINS == sp::MAX_BINS &&
                  MAX_TRIALS == sp::MAX_TRIALS && MAX_NSAMP == sp::MAX_NSAMP,
              "rtlws_fold.h, fold.h and search_plan.h disagree");

// ---- the rules, each worded once ----
const char* why_not_nperiods(int nperiods) { return nperiods < 1 || nperiods > MAX_PERIODS ? "nperiods must be 1 .. 4096" : nullptr; }

const char* why_not_shape(int nbins, long sub)
{
    if (const char* why = sp::why_not_nbins(nbins)) return why;
    if (sub < MIN_SUB || sub > MAX_SUB || sub % 4) return "sub must be 64 .. 16777216 and a multiple of 4";
    return nullptr;
}

const char* why_not_tables(int nperiods, const uint64_t* steps, const uint64_t* phases, int nbins, long sub)
{
    if (const char* why = why_not_nperiods(nperiods)) return why;
    if (const char* why = sp::why_not_steps(steps, phases)) return why;
    return why_not_shape(nbins, sub);
}

int groups_of(int nperiods, int nbins) { return (int)sp::ceil_div(nperiods, LANES * waves_per_block(nbins)); }

const char* why_not_grid(int nperiods, int nbins, long sub, int ntrials, long nsamp)
{
    return sp::why_not_grid(sp::ceil_div(nsamp, sub), (long)ntrials * groups_of(nperiods, nbins));
}

}  // namespace

extern "C" {

const char* rtlws_fold_last_error(void) { return g_err.c_str(); }

int rtlws_fold_supported(int nperiods, const uint64_t* steps, const uint64_t* phases, int nbins, long sub)
{
    return supported("rtlws_fold", why_not_tables(nperiods, steps, phases, nbins, sub));
}

int rtlws_fold_geometry(int nperiods, int nbins, long sub, int ntrials, long nsamp, int* blocks, int* threads, int* lds, int* tile,
                        int* wpb, long* nsub)
{
    const char* fn = "rtlws_fold_geometry";
    g_err.clear();
    if (const char* why = why_not_nperiods(nperiods)) return fail(fn, why, -1);
    if (const char* why = why_not_shape(nbins, sub)) return fail(fn, why, -1);
    if (const char* why = sp::why_not_ntrials(ntrials)) return fail(fn, why, -1);
    if (const char* why = sp::why_not_nsamp(nsamp)) return fail(fn, why, -1);
    if (const char* why = why_not_grid(nperiods, nbins, sub, ntrials, nsamp)) return fail(fn, why, -1);
    if (blocks) *blocks = (int)(sp::ceil_div(nsamp, sub) * ntrials * groups_of(nperiods, nbins));
    if (threads) *threads = LANES * waves_per_block(nbins);
    if (lds) *lds = lds_bytes(nbins);
    if (tile) *tile = TILE;
    if (wpb) *wpb = waves_per_block(nbins);
    if (nsub) *nsub = sp::ceil_div(nsamp, sub);
    return 0;
}

rtlws_fold_plan* rtlws_fold_open(rtlws_engine* e, int nperiods, const uint64_t* steps, const uint64_t* phases, int nbins, long sub)
{
    const auto fill = [&](rtlws_fold_plan& p) {
        p.nperiods = nperiods, p.nbins = nbins, p.sub = sub;
        const size_t bytes = (size_t)nperiods * sizeof(uint64_t);
        hipError_t err = hipMalloc(reinterpret_cast<void**>(&p.d_tables), 2 * bytes);
        if (err == hipSuccess) err = hipMemcpy(p.d_tables, steps, bytes, hipMemcpyHostToDevice);
        if (err == hipSuccess) err = hipMemcpy(p.d_tables + nperiods, phases, bytes, hipMemcpyHostToDevice);
        return err == hipSuccess ? prepare_fold(nbins) : err;
    };
    return sp::open_plan<rtlws_fold_plan>("rtlws_fold_open", why_not_tables(nperiods, steps, phases, nbins, sub), e, fill, "the tables or the kernel",
                                          rtlws_fold_close);
}

void rtlws_fold_close(rtlws_fold_plan* p) { sp::close_plan(p, &rtlws_fold_plan::d_tables); }

long rtlws_fold_subints(const rtlws_fold_plan* p, long nsamp)
{
    const char* fn = "rtlws_fold_subints";
    g_err.clear();
    if (const char* why = sp::why_not_nsamp(nsamp)) return fail(fn, why, -1);
    if (!p) return fail(fn, NULL_PLAN, -1);
    return sp::ceil_div(nsamp, p->sub);
}

int rtlws_fold_run(rtlws_fold_plan* p, const float* d_in, long in_stride, int ntrials, long nsamp, float* d_prof, uint32_t* d_hits,
                   void* stream)
{
    const char* fn = "rtlws_fold_run";
    g_err.clear();
    // what needs no plan
    if (const char* why = sp::why_not_ntrials(ntrials)) return fail(fn, why, -1);
    if (const char* why = sp::why_not_nsamp(nsamp)) return fail(fn, why, -1);
    if (in_stride < nsamp) return fail(fn, "in_stride must be >= nsamp", -1);
    if (const char* why = sp::why_not_stride(in_stride)) return fail(fn, why, -1);
    if (nsamp > 0 && (!d_in || !d_prof)) return fail(fn, "null pointer", -1);
    if (sp::misaligned(d_in, 16)) return fail(fn, "d_in must be 16-byte aligned", -1);
    if (sp::misaligned(d_prof, 4)) return fail(fn, "d_prof must be 4-byte aligned", -1);
    if (sp::misaligned(d_hits, 4)) return fail(fn, "d_hits must be 4-byte aligned", -1);
    if (!p) return fail(fn, NULL_PLAN, -1);
    // what the plan decides; still before anything is asked of the device
    if (const char* why = why_not_grid(p->nperiods, p->nbins, p->sub, ntrials, nsamp)) return fail(fn, why, -1);
    if (nsamp == 0) return 0;

    if (sp::use_device(fn, p)) return -3;
    Params kp;
    kp.in = d_in;
    kp.prof = d_prof;
    kp.hits = d_hits;
    kp.steps = p->d_tables;
    kp.phases = p->d_tables + p->nperiods;
    kp.in_stride = in_stride;
    kp.nsamp = nsamp;
    kp.sub = p->sub;
    kp.nsub = sp::ceil_div(nsamp, p->sub);
    kp.nperiods = p->nperiods;
    kp.nbins = p->nbins;
    kp.groups = groups_of(p->nperiods, p->nbins);
    const hipError_t err = launch_fold(kp, ntrials, stream_of(p->engine, stream));
    if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
    return 0;
}

uint64_t rtlws_fold_step(double period_in_samples)
{
    g_err.clear();
    if (!(period_in_samples >= 2.0 && period_in_samples <= 4294967296.0)) return (uint64_t)fail("rtlws_fold_step", "the period must be 2 .. 2^32 samples", 0);
    // P = m 2^e with m an integer below 2^53: 2^64 / P = 2^(64 - e) / m, and 64 - e is 84 .. 115 here
    int exp2;
    const double frac = std::frexp(period_in_samples, &exp2);
    const unsigned __int128 m = (unsigned __int128)(uint64_t)std::ldexp(frac, 53);
    const unsigned __int128 twice = (unsigned __int128)1 << (64 - (exp2 - 53) + 1);
    return (uint64_t)((twice + m) / (2 * m));                  // floor(q + 1/2): halves round up
}

uint64_t rtlws_fold_phase_at(uint64_t step, uint64_t phi0, long n0) { return phi0 + (uint64_t)n0 * step; }

double rtlws_fold_chi2(const float* prof, const uint32_t* hits, int nbins, double sum1, double sum2, long count)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    double mean, var;
    if (nbins < 1 || !prof || !hits || !sp::moments(sum1, sum2, count, &mean, &var)) return nan;
    double chi2 = 0.0;
    for (int b = 0; b < nbins; ++b) {
        if (hits[b] == 0) return nan;
        const double d = (double)prof[b] - (double)hits[b] * mean;
        chi2 = chi2 + d * d / ((double)hits[b] * var);
    }
    return chi2;
}

}  // extern "C"
