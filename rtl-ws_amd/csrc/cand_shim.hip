// cand_shim.hip -- extern "C" glue of include/rtlws_cand.h (librtlws_cand.so): argument rules, the two plans with their
// tables (the cube's steps, phases and delays with the mask folded in; the refinement's two shift tables and its
// workspace), the launches, and the host's helpers (the shifts of a DM grid and of a frequency grid, the chi-square).
// The engine (device, stream) is librtlws_hip.so's; nothing here reads the environment, and nothing of a run is computed
// on the host: without a device there is no plan.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "cand.h"
#include "rtlws_cand.h"
#include "search_plan.h"

struct rtlws_cand_fold_plan : rtlws::search::Plan {
    int ncand, nchan, nbins, max_delay;
    long sub;
    uint64_t* d_tables;        // steps [ncand], phases [ncand], then the delays [ncand][nchan] as int32 (-1: masked)
};

struct rtlws_cand_search_plan : rtlws::search::Plan {
    int ncand, nsub, nchan, nbins, ndm, ntr;
    int32_t* d_shifts;         // a [ncand][ndm][nchan], then g [ncand][ntr][nsub]
    float* d_work;             // T [ncand][ndm][nsub][nbins]
};

namespace {

using namespace rtlws::cand;
namespace sp = rtlws::search;
using sp::why_not_nbins;
using sp::why_not_nchan;
using sp::why_not_nsamp;

static_assert(MAX_CANDS == RTLWS_CAND_MAX_CANDS && MIN_NCHAN == RTLWS_CAND_MIN_NCHAN && MAX_NCHAN == RTLWS_CAND_MAX_NCHAN &&
                  MAX_DELAY == RTLWS_CAND_MAX_DELAY && MIN_BINS == RTLWS_CAND_MIN_BINS && MAX_BINS == RTLWS_CAND_MAX_BINS &&
                  MIN_SUB == RTLWS_CAND_MIN_SUB && MAX_SUB == RTLWS_CAND_MAX_SUB && MAX_NSAMP == RTLWS_CAND_MAX_NSAMP &&
                  MAX_NSUB == RTLWS_CAND_MAX_NSUB && MAX_NDM == RTLWS_CAND_MAX_NDM && MAX_NTR == RTLWS_CAND_MAX_NTR &&
                  MAX_WORKSPACE == RTLWS_CAND_MAX_WORKSPACE && MIN_NCHAN == sp::MIN_NCHAN && MAX_NCHAN == sp::MAX_NCHAN &&
                  MIN_BINS == sp::MIN_BINS && MAX_BINS == sp::MAX_BINS && MAX_NSAMP == sp::MAX_NSAMP,
              "rtlws_cand.h, cand.h and search_plan.h disagree");

// ---- the rules, each worded once ----
const char* why_not_ncand(int ncand) { return ncand < 1 || ncand > MAX_CANDS ? "ncand must be 1 .. 64" : nullptr; }
const char* why_not_sub(long sub) { return sub < MIN_SUB || sub > MAX_SUB ? "sub must be 16 .. 16777216" : nullptr; }
const char* why_not_nsub(int nsub) { return nsub < 1 || nsub > MAX_NSUB ? "nsub must be 1 .. 1024" : nullptr; }
const char* why_not_ndm(int ndm) { return ndm < 1 || ndm > MAX_NDM ? "ndm must be 1 .. 256" : nullptr; }

const char* why_not_cube(int ncand, int nchan, int nbins, long sub)
{
    if (const char* why = why_not_ncand(ncand)) return why;
    if (const char* why = why_not_nchan(nchan)) return why;
    if (const char* why = why_not_nbins(nbins)) return why;
    return why_not_sub(sub);
}

const char* why_not_fold_tables(int ncand, const uint64_t* steps, const uint64_t* phases, int nchan, const int32_t* delays, int nbins, long sub)
{
    if (const char* why = why_not_cube(ncand, nchan, nbins, sub)) return why;
    if (const char* why = sp::why_not_steps(steps, phases)) return why;
    if (delays)
        for (long j = 0; j < (long)ncand * nchan; ++j)
            if (delays[j] < 0 || delays[j] > MAX_DELAY) return "a delay outside 0 .. 65535";
    return nullptr;
}

const char* why_not_grid(int ncand, int nchan, int nbins, long sub, long nsamp)
{
    return sp::why_not_grid(sp::ceil_div(nsamp, sub), (long)ncand * chan_groups(nchan, nbins));
}

long workspace_of(int ncand, int nsub, int nbins, int ndm) { return (long)ncand * ndm * nsub * nbins * (long)sizeof(float); }

const char* why_not_search(int ncand, int nsub, int nchan, int nbins, int ndm, int ntr)
{
    if (const char* why = why_not_ncand(ncand)) return why;
    if (const char* why = why_not_nsub(nsub)) return why;
    if (const char* why = why_not_nchan(nchan)) return why;
    if (const char* why = why_not_nbins(nbins)) return why;
    if (const char* why = why_not_ndm(ndm)) return why;
    if (ntr < 1 || ntr > MAX_NTR) return "ntr must be 1 .. 4096";
    if (workspace_of(ncand, nsub, nbins, ndm) > MAX_WORKSPACE) return "a workspace above 2^30 bytes";
    return nullptr;
}

const char* why_not_shifts(const int32_t* table, long count, int nbins, const char* why)
{
    for (long j = 0; j < count; ++j)
        if (table[j] < 0 || table[j] >= nbins) return why;
    return nullptr;
}

const char* why_not_search_tables(int ncand, int nsub, int nchan, int nbins, int ndm, const int32_t* a, int ntr, const int32_t* g)
{
    if (const char* why = why_not_search(ncand, nsub, nchan, nbins, ndm, ntr)) return why;
    if (!a) return "null a";
    if (!g) return "null g";
    if (const char* why = why_not_shifts(a, (long)ncand * ndm * nchan, nbins, "an entry of a outside 0 .. nbins - 1")) return why;
    return why_not_shifts(g, (long)ncand * ntr * nsub, nbins, "an entry of g outside 0 .. nbins - 1");
}

// rint(v) mod nbins into 0 .. nbins - 1; false where v is not finite or 2^31 bins or more
bool shift_of(double v, int nbins, int32_t* out)
{
    const double r = std::rint(v);
    if (!(std::fabs(r) < 2147483648.0)) return false;
    double m = std::fmod(r, (double)nbins);                    // exact: both are integers below 2^53
    if (m < 0.0) m += (double)nbins;
    *out = (int32_t)m;
    return true;
}

}  // namespace

extern "C" {

const char* rtlws_cand_last_error(void) { return g_err.c_str(); }

int rtlws_cand_fold_supported(int ncand, int nchan, int nbins, long sub) { return supported("rtlws_cand_fold", why_not_cube(ncand, nchan, nbins, sub)); }

int rtlws_cand_fold_geometry(int ncand, int nchan, int nbins, long sub, long nsamp, int* blocks, int* threads, int* lds, int* wpb, long* nsub)
{
    const char* fn = "rtlws_cand_fold_geometry";
    g_err.clear();
    if (const char* why = why_not_cube(ncand, nchan, nbins, sub)) return fail(fn, why, -1);
    if (const char* why = why_not_nsamp(nsamp)) return fail(fn, why, -1);
    if (const char* why = why_not_grid(ncand, nchan, nbins, sub, nsamp)) return fail(fn, why, -1);
    if (blocks) *blocks = (int)(sp::ceil_div(nsamp, sub) * ncand * chan_groups(nchan, nbins));
    if (threads) *threads = LANES * waves_per_block(nbins);
    if (lds) *lds = lds_bytes(nbins);
    if (wpb) *wpb = waves_per_block(nbins);
    if (nsub) *nsub = sp::ceil_div(nsamp, sub);
    return 0;
}

rtlws_cand_fold_plan* rtlws_cand_fold_open(rtlws_engine* e, int ncand, const uint64_t* steps, const uint64_t* phases, int nchan,
                                           const int32_t* delays, const uint8_t* mask, int nbins, long sub)
{
    const auto fill = [&](rtlws_cand_fold_plan& p) {
        p.ncand = ncand, p.nchan = nchan, p.nbins = nbins, p.sub = sub;
        // steps, phases, then the delays as the kernel reads them: -1 where the mask drops the channel
        const size_t cells = (size_t)ncand * nchan;
        std::vector<uint64_t> host(2 * (size_t)ncand + (cells + 1) / 2);
        int32_t* const d = reinterpret_cast<int32_t*>(host.data() + 2 * (size_t)ncand);
        for (int c = 0; c < ncand; ++c) {
            host[c] = steps[c];
            host[(size_t)ncand + c] = phases[c];
            for (int i = 0; i < nchan; ++i) {
                const int32_t v = delays ? delays[(size_t)c * nchan + i] : 0;
                const bool kept = !mask || mask[i];
                d[(size_t)c * nchan + i] = kept ? v : -1;
                if (kept && v > p.max_delay) p.max_delay = v;
            }
        }
        const hipError_t err = sp::upload(&p.d_tables, host.data(), host.size());
        return err == hipSuccess ? prepare_fold(nbins) : err;
    };
    return sp::open_plan<rtlws_cand_fold_plan>("rtlws_cand_fold_open", why_not_fold_tables(ncand, steps, phases, nchan, delays, nbins, sub), e, fill,
                                               "the tables or the kernel", rtlws_cand_fold_close);
}

void rtlws_cand_fold_close(rtlws_cand_fold_plan* p) { sp::close_plan(p, &rtlws_cand_fold_plan::d_tables); }

long rtlws_cand_fold_rows_needed(const rtlws_cand_fold_plan* p, long nsamp)
{
    const char* fn = "rtlws_cand_fold_rows_needed";
    g_err.clear();
    if (const char* why = why_not_nsamp(nsamp)) return fail(fn, why, -1);
    if (!p) return fail(fn, NULL_PLAN, -1);
    return nsamp ? nsamp + p->max_delay : 0;
}

int rtlws_cand_fold_run(rtlws_cand_fold_plan* p, const float* d_rows, long in_stride, long nsamp, float* d_cube, uint32_t* d_hits, void* stream)
{
    const char* fn = "rtlws_cand_fold_run";
    g_err.clear();
    // what needs no plan
    if (const char* why = why_not_nsamp(nsamp)) return fail(fn, why, -1);
    if (const char* why = sp::why_not_stride_of_rows(in_stride)) return fail(fn, why, -1);
    if (!d_rows || !d_cube) return fail(fn, "null pointer", -1);
    if (sp::misaligned(d_rows, 16)) return fail(fn, "d_rows must be 16-byte aligned", -1);
    if (sp::misaligned(d_cube, 4)) return fail(fn, "d_cube must be 4-byte aligned", -1);
    if (sp::misaligned(d_hits, 4)) return fail(fn, "d_hits must be 4-byte aligned", -1);
    if (!p) return fail(fn, NULL_PLAN, -1);
    // what the plan decides; still before anything is asked of the device
    if (const char* why = sp::why_not_row_stride(in_stride, p->nchan)) return fail(fn, why, -1);
    if (const char* why = why_not_grid(p->ncand, p->nchan, p->nbins, p->sub, nsamp)) return fail(fn, why, -1);
    if (nsamp == 0) return 0;

    if (sp::use_device(fn, p)) return -3;
    FoldParams kp;
    kp.rows = d_rows;
    kp.cube = d_cube;
    kp.hits = d_hits;
    kp.steps = p->d_tables;
    kp.phases = p->d_tables + p->ncand;
    kp.delays = reinterpret_cast<const int32_t*>(p->d_tables + 2 * p->ncand);
    kp.in_stride = in_stride;
    kp.nsamp = nsamp;
    kp.sub = p->sub;
    kp.nsub = sp::ceil_div(nsamp, p->sub);
    kp.nchan = p->nchan;
    kp.nbins = p->nbins;
    kp.groups = chan_groups(p->nchan, p->nbins);
    const hipError_t err = launch_fold(kp, p->ncand, stream_of(p->engine, stream));
    if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
    return 0;
}

int rtlws_cand_search_supported(int ncand, int nsub, int nchan, int nbins, int ndm, int ntr)
{
    return supported("rtlws_cand_search", why_not_search(ncand, nsub, nchan, nbins, ndm, ntr));
}

int rtlws_cand_search_geometry(int ncand, int nsub, int nchan, int nbins, int ndm, int ntr, int* blocks1, int* blocks2, int* threads, int* lds1,
                               int* lds2, long* workspace_bytes)
{
    g_err.clear();
    if (const char* why = why_not_search(ncand, nsub, nchan, nbins, ndm, ntr)) return fail("rtlws_cand_search_geometry", why, -1);
    if (blocks1) *blocks1 = ncand * nsub * trial_groups(ndm);
    if (blocks2) *blocks2 = ncand * ndm * trial_groups(ntr);
    if (threads) *threads = WAVES * LANES;
    if (lds1) *lds1 = stage_lds_bytes(nbins, false);
    if (lds2) *lds2 = stage_lds_bytes(nbins, true);
    if (workspace_bytes) *workspace_bytes = workspace_of(ncand, nsub, nbins, ndm);
    return 0;
}

rtlws_cand_search_plan* rtlws_cand_search_open(rtlws_engine* e, int ncand, int nsub, int nchan, int nbins, int ndm, const int32_t* a, int ntr,
                                               const int32_t* g)
{
    const auto fill = [&](rtlws_cand_search_plan& p) {
        p.ncand = ncand, p.nsub = nsub, p.nchan = nchan, p.nbins = nbins, p.ndm = ndm, p.ntr = ntr;
        const size_t na = (size_t)ncand * ndm * nchan, ng = (size_t)ncand * ntr * nsub;
        hipError_t err = hipMalloc(reinterpret_cast<void**>(&p.d_shifts), (na + ng) * sizeof(int32_t));
        if (err == hipSuccess) err = hipMemcpy(p.d_shifts, a, na * sizeof(int32_t), hipMemcpyHostToDevice);
        if (err == hipSuccess) err = hipMemcpy(p.d_shifts + na, g, ng * sizeof(int32_t), hipMemcpyHostToDevice);
        if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&p.d_work), (size_t)workspace_of(ncand, nsub, nbins, ndm));
        return err == hipSuccess ? prepare_stages(nbins) : err;
    };
    return sp::open_plan<rtlws_cand_search_plan>("rtlws_cand_search_open", why_not_search_tables(ncand, nsub, nchan, nbins, ndm, a, ntr, g), e, fill,
                                                 "the tables, the workspace or the kernels", rtlws_cand_search_close);
}

void rtlws_cand_search_close(rtlws_cand_search_plan* p)
{
    sp::close_plan(p, &rtlws_cand_search_plan::d_shifts, &rtlws_cand_search_plan::d_work);
}

int rtlws_cand_search_run(rtlws_cand_search_plan* p, const float* d_cube, double* d_stat, double* d_total, float* d_prof, float* d_tphase,
                          void* stream)
{
    const char* fn = "rtlws_cand_search_run";
    g_err.clear();
    if (!d_cube || !d_stat || !d_total) return fail(fn, "null pointer", -1);
    if (sp::misaligned(d_cube, 4)) return fail(fn, "d_cube must be 4-byte aligned", -1);
    if (sp::misaligned(d_stat, 8)) return fail(fn, "d_stat must be 8-byte aligned", -1);
    if (sp::misaligned(d_total, 8)) return fail(fn, "d_total must be 8-byte aligned", -1);
    if (sp::misaligned(d_prof, 4)) return fail(fn, "d_prof must be 4-byte aligned", -1);
    if (sp::misaligned(d_tphase, 4)) return fail(fn, "d_tphase must be 4-byte aligned", -1);
    if (!p) return fail(fn, NULL_PLAN, -1);

    if (sp::use_device(fn, p)) return -3;
    const hipStream_t st = stream_of(p->engine, stream);
    StageParams s1{};
    s1.in = d_cube;
    s1.shifts = p->d_shifts;
    s1.out = p->d_work;
    s1.copy = d_tphase;
    s1.no = p->nsub, s1.nk = p->nchan, s1.nt = p->ndm, s1.nbins = p->nbins;
    hipError_t err = launch_stage(false, s1, p->ncand, st);
    if (err != hipSuccess) return fail_hip(fn, "kernel launch (stage 1)", err);
    StageParams s2{};
    s2.in = p->d_work;
    s2.shifts = p->d_shifts + (size_t)p->ncand * p->ndm * p->nchan;
    s2.out = d_prof;
    s2.stat = d_stat;
    s2.total = d_total;
    s2.no = p->ndm, s2.nk = p->nsub, s2.nt = p->ntr, s2.nbins = p->nbins;
    err = launch_stage(true, s2, p->ncand, st);
    if (err != hipSuccess) return fail_hip(fn, "kernel launch (stage 2)", err);
    return 0;
}

int rtlws_cand_dm_shifts(int nchan, int shifted, double f_centre_hz, double bandwidth_hz, double row_seconds, double period_rows, int nbins,
                         int ndm, double ddm0, double ddm_step, int32_t* a)
{
    const char* fn = "rtlws_cand_dm_shifts";
    g_err.clear();
    if (const char* why = why_not_nchan(nchan)) return fail(fn, why, -1);
    if (shifted != 0 && shifted != 1) return fail(fn, "shifted must be 0 or 1", -1);
    if (const char* why = sp::why_not_band(nchan, f_centre_hz, bandwidth_hz, row_seconds)) return fail(fn, why, -1);
    const int M = nchan;
    if (!(std::isfinite(period_rows) && period_rows > 0.0)) return fail(fn, "period_rows must be finite and > 0", -1);
    if (const char* why = why_not_nbins(nbins)) return fail(fn, why, -1);
    if (const char* why = why_not_ndm(ndm)) return fail(fn, why, -1);
    if (!std::isfinite(ddm0) || !std::isfinite(ddm_step)) return fail(fn, "the DM offsets must be finite", -1);
    if (!a) return fail(fn, "null table", -1);
    const std::vector<double> excess = sp::excess(M, shifted, f_centre_hz, bandwidth_hz);
    for (int q = 0; q < ndm; ++q) {
        const double ddm = ddm0 + (double)q * ddm_step;
        for (int i = 0; i < M; ++i) {
            const double rows = sp::DISPERSION * ddm * excess[i] / row_seconds;
            if (!shift_of((double)nbins * rows / period_rows, nbins, a + (long)q * M + i)) return fail(fn, "a shift of 2^31 bins or more", -1);
        }
    }
    return 0;
}

int rtlws_cand_drift_shifts(int nbins, long sub, int nsub, int nf, double df0, double df_step, int nfd, double dfd0, double dfd_step, int32_t* g)
{
    const char* fn = "rtlws_cand_drift_shifts";
    g_err.clear();
    if (const char* why = why_not_nbins(nbins)) return fail(fn, why, -1);
    if (const char* why = why_not_sub(sub)) return fail(fn, why, -1);
    if (const char* why = why_not_nsub(nsub)) return fail(fn, why, -1);
    if (nf < 1 || nfd < 1 || (long)nf * nfd > MAX_NTR) return fail(fn, "nf and nfd must be >= 1 and nf * nfd <= 4096", -1);
    if (!std::isfinite(df0) || !std::isfinite(df_step) || !std::isfinite(dfd0) || !std::isfinite(dfd_step))
        return fail(fn, "the offsets must be finite", -1);
    if (!g) return fail(fn, "null table", -1);
    for (int k = 0; k < nfd; ++k)
        for (int j = 0; j < nf; ++j) {
            const double df = df0 + (double)j * df_step, dfd = dfd0 + (double)k * dfd_step;
            for (int s = 0; s < nsub; ++s) {
                const double t = ((double)s + 0.5) * (double)sub;
                if (!shift_of((double)nbins * (df * t + 0.5 * dfd * t * t), nbins, g + ((long)k * nf + j) * nsub + s))
                    return fail(fn, "a shift of 2^31 bins or more", -1);
            }
        }
    return 0;
}

double rtlws_cand_chi2(double stat, double total, int nbins, double bin_variance)
{
    if (nbins < 2 || !(bin_variance > 0.0)) return std::numeric_limits<double>::quiet_NaN();
    return (stat - total * total / (double)nbins) / ((double)(nbins - 1) * bin_variance);
}

}  // extern "C"
