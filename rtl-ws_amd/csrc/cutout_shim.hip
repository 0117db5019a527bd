// cutout_shim.hip -- extern "C" glue of include/rtlws_cutout.h (librtlws_cutout.so): argument rules, the window's rule
// on the host, the plan's tables (cutout.h), the two launches.  The engine (device, stream) is librtlws_hip.so's; nothing
// here reads the environment, and nothing of a run is computed on the host: without a device there is no plan.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <vector>

#include "cutout.h"
#include "dedisp_form.h"
#include "rtlws_cutout.h"
#include "search_plan.h"

// The tables as the kernels read them, on the engine's device
struct rtlws_cutout_plan : rtlws::search::Plan {
    int nchan, ntrials, nwidths, nx, nf, rq, dq, max_delay;
    uint16_t* d_delays;
    uint8_t* d_keep;
    int2* d_shape;
};

namespace {

using namespace rtlws::cutout;
namespace sp = rtlws::search;
namespace dd = rtlws::dedisp;

static_assert(MIN_NCHAN == RTLWS_CUTOUT_MIN_NCHAN && MAX_NCHAN == RTLWS_CUTOUT_MAX_NCHAN && MAX_TRIALS == RTLWS_CUTOUT_MAX_TRIALS && MAX_DELAY == RTLWS_CUTOUT_MAX_DELAY &&
                  MAX_WIDTHS == RTLWS_CUTOUT_MAX_WIDTHS && MAX_WIDTH == RTLWS_CUTOUT_MAX_WIDTH && MAX_BIN == RTLWS_CUTOUT_MAX_BIN && MIN_NX == RTLWS_CUTOUT_MIN_NX &&
                  MAX_NX == RTLWS_CUTOUT_MAX_NX && MAX_NF == RTLWS_CUTOUT_MAX_NF && MAX_RQ == RTLWS_CUTOUT_MAX_RQ && MAX_DQ == RTLWS_CUTOUT_MAX_DQ &&
                  MAX_NSAMP == RTLWS_CUTOUT_MAX_NSAMP && MAX_CAND == RTLWS_CUTOUT_MAX_CAND && CAND_WORDS == RTLWS_CUTOUT_CAND_WORDS && INFO_WORDS == RTLWS_CUTOUT_INFO_WORDS &&
                  MIN_NCHAN == sp::MIN_NCHAN && MAX_NCHAN == sp::MAX_NCHAN && MAX_WIDTHS == sp::MAX_WIDTHS && MAX_NSAMP == sp::MAX_NSAMP,
              "rtlws_cutout.h, cutout.h, dedisp.h, pulse.h, sift.h and search_plan.h disagree");

// ---- the rules, each worded once ----
const char* const WHY_NX = "nx must be 4 .. 256 and a multiple of 4";
const char* const WHY_BIN = "every bin must be 1 .. 1024";
const char* const WHY_WIDTH = "every width must be 1 .. 1024";
const char* const WHY_NSAMP = "nsamp must be 1 .. 2^30";

const char* why_not_nx(int nx) { return nx < MIN_NX || nx > MAX_NX || nx % 4 ? WHY_NX : nullptr; }
const char* why_not_nsamp(long nsamp) { return nsamp < 1 || nsamp > MAX_NSAMP ? WHY_NSAMP : nullptr; }
const char* why_not_max_cand(int max_cand) { return max_cand < 1 || max_cand > MAX_CAND ? "max_cand must be 1 .. 4096" : nullptr; }

// everything of a plan but the table of delays
const char* why_not_shape(int nchan, int ntrials, int nwidths, const int32_t* widths, const int32_t* bins, int nx, int nf, int rq, int dq)
{
    if (const char* why = sp::why_not_nchan(nchan)) return why;
    if (ntrials < 1 || ntrials > MAX_TRIALS) return dd::WHY_NTRIALS;
    if (const char* why = sp::why_not_widths(nwidths, widths, MAX_WIDTH, WHY_WIDTH)) return why;
    if (!bins) return "null bins";
    for (int k = 0; k < nwidths; ++k)
        if (bins[k] < 1 || bins[k] > MAX_BIN) return WHY_BIN;
    if (const char* why = why_not_nx(nx)) return why;
    if (nf < 1 || nf > MAX_NF || nchan % nf) return "nf must be 1 .. nchan and divide nchan";
    if (rq < 0 || rq > MAX_RQ) return "rq must be 0 .. 64";
    if (dq < 1 || dq > MAX_DQ) return "dq must be 1 .. 64";
    return nullptr;
}

// the table's entries, by the dedispersion's rule; *max_delay: the largest over the positions the mask keeps
const char* why_not_table(int nchan, int ntrials, const int32_t* delays, const uint8_t* mask, int* max_delay)
{
    if (!delays) return dd::WHY_NULL_DELAYS;
    int most = 0;
    for (long t = 0; t < ntrials; ++t)
        for (int i = 0; i < nchan; ++i) {
            const int32_t d = delays[t * nchan + i];
            if (d < 0 || d > MAX_DELAY) return dd::WHY_DELAY;
            if ((!mask || mask[i]) && d > most) most = d;
        }
    *max_delay = most;
    return nullptr;
}

const char* why_not_plan(int nchan, int ntrials, const int32_t* delays, const uint8_t* mask, int nwidths, const int32_t* widths, const int32_t* bins, int nx,
                         int nf, int rq, int dq, int* max_delay)
{
    if (const char* why = why_not_shape(nchan, ntrials, nwidths, widths, bins, nx, nf, rq, dq)) return why;
    return why_not_table(nchan, ntrials, delays, mask, max_delay);
}

long xgroups_of(int nx) { return sp::ceil_div(nx, TILE_X); }
long fgroups_of(int nchan, int nf) { return sp::ceil_div(nf, subbands_per_group(nchan / nf)); }

// the two grids of max_cand candidates
const char* why_not_grids(int max_cand, int nchan, int nx, int nf, int rq)
{
    if (const char* why = sp::why_not_grid(max_cand, xgroups_of(nx) * fgroups_of(nchan, nf))) return why;
    return sp::why_not_grid(max_cand, 2 * rq + 1);
}

}  // namespace

extern "C" {

const char* rtlws_cutout_last_error(void) { return g_err.c_str(); }

int rtlws_cutout_supported(int nchan, int ntrials, int nwidths, const int32_t* widths, const int32_t* bins, int nx, int nf, int rq, int dq)
{
    return supported("rtlws_cutout", why_not_shape(nchan, ntrials, nwidths, widths, bins, nx, nf, rq, dq));
}

int rtlws_cutout_geometry(int nchan, int ntrials, const int32_t* delays, const uint8_t* mask, int nwidths, const int32_t* widths, const int32_t* bins, int nx,
                          int nf, int rq, int dq, int max_cand, int* blocks, int* threads, int* lds_bytes, int* ndm, int* max_delay)
{
    const char* fn = "rtlws_cutout_geometry";
    g_err.clear();
    int most = 0;
    if (const char* why = why_not_plan(nchan, ntrials, delays, mask, nwidths, widths, bins, nx, nf, rq, dq, &most)) return fail(fn, why, -1);
    if (const char* why = why_not_max_cand(max_cand)) return fail(fn, why, -1);
    if (const char* why = why_not_grids(max_cand, nchan, nx, nf, rq)) return fail(fn, why, -1);
    if (blocks) blocks[0] = (int)(max_cand * xgroups_of(nx) * fgroups_of(nchan, nf)), blocks[1] = max_cand * (2 * rq + 1);
    if (threads) threads[0] = THREADS, threads[1] = dmt_threads(nx);
    if (lds_bytes) lds_bytes[0] = (int)sizeof(BandLds), lds_bytes[1] = 0;
    if (ndm) *ndm = 2 * rq + 1;
    if (max_delay) *max_delay = most;
    return 0;
}

rtlws_cutout_plan* rtlws_cutout_open(rtlws_engine* e, int nchan, int ntrials, const int32_t* delays, const uint8_t* mask, int nwidths, const int32_t* widths,
                                     const int32_t* bins, int nx, int nf, int rq, int dq)
{
    int most = 0;
    const char* why = why_not_plan(nchan, ntrials, delays, mask, nwidths, widths, bins, nx, nf, rq, dq, &most);
    const auto fill = [&](rtlws_cutout_plan& p) {
        p.nchan = nchan, p.ntrials = ntrials, p.nwidths = nwidths, p.nx = nx, p.nf = nf, p.rq = rq, p.dq = dq, p.max_delay = most;
        const std::vector<uint16_t> table(delays, delays + (long)ntrials * nchan);
        std::vector<uint8_t> keep(nchan, 1);
        for (int i = 0; mask && i < nchan; ++i) keep[i] = mask[i] ? 1 : 0;
        std::vector<int2> shape(nwidths);
        for (int k = 0; k < nwidths; ++k) shape[k] = make_int2(widths[k], bins[k]);
        hipError_t err = sp::upload(&p.d_delays, table.data(), table.size());
        if (err == hipSuccess) err = sp::upload(&p.d_keep, keep.data(), keep.size());
        if (err == hipSuccess) err = sp::upload(&p.d_shape, shape.data(), shape.size());
        return err == hipSuccess ? prepare_cutout() : err;
    };
    return sp::open_plan<rtlws_cutout_plan>("rtlws_cutout_open", why, e, fill, "the tables or the kernels", rtlws_cutout_close);
}

void rtlws_cutout_close(rtlws_cutout_plan* p) { sp::close_plan(p, &rtlws_cutout_plan::d_delays, &rtlws_cutout_plan::d_keep, &rtlws_cutout_plan::d_shape); }

long rtlws_cutout_rows_needed(const rtlws_cutout_plan* p, long nsamp)
{
    const char* fn = "rtlws_cutout_rows_needed";
    g_err.clear();
    if (const char* why = why_not_nsamp(nsamp)) return fail(fn, why, -1);
    if (!p) return fail(fn, NULL_PLAN, -1);
    return nsamp + p->max_delay;
}

int rtlws_cutout_window(long at, int width, int bin, int nx, long nsamp, long* n0, long* inside)
{
    const char* fn = "rtlws_cutout_window";
    g_err.clear();
    if (const char* why = why_not_nsamp(nsamp)) return fail(fn, why, -1);
    if (at < 0 || at >= nsamp) return fail(fn, "at must be 0 .. nsamp - 1", -1);
    if (width < 1 || width > MAX_WIDTH) return fail(fn, WHY_WIDTH, -1);
    if (bin < 1 || bin > MAX_BIN) return fail(fn, WHY_BIN, -1);
    if (const char* why = why_not_nx(nx)) return fail(fn, why, -1);
    const long first = at + width / 2 - (long)(nx / 2) * bin, end = first + (long)nx * bin;
    if (n0) *n0 = first;
    const long rows = (end < nsamp ? end : nsamp) - (first > 0 ? first : 0);
    if (inside) *inside = rows > 0 ? rows : 0;                // a wide boxcar near the end: the centre lies behind the series
    return 0;
}

int rtlws_cutout_run(rtlws_cutout_plan* p, const float* d_rows, long in_stride, const float* d_series, long series_stride, long nsamp, const uint32_t* d_cand,
                     const int32_t* d_count, int max_cand, float* d_ft, float* d_dmt, int32_t* d_info, void* stream)
{
    const char* fn = "rtlws_cutout_run";
    g_err.clear();
    // what needs no plan
    if (const char* why = why_not_nsamp(nsamp)) return fail(fn, why, -1);
    if (const char* why = why_not_max_cand(max_cand)) return fail(fn, why, -1);
    if (const char* why = sp::why_not_stride_of_rows(in_stride)) return fail(fn, why, -1);
    if (series_stride < nsamp) return fail(fn, "series_stride must be >= nsamp", -1);
    if (!d_ft && !d_dmt) return fail(fn, "d_ft and d_dmt must not both be NULL", -1);
    if (!d_cand || !d_count || !d_info || (d_ft && !d_rows) || (d_dmt && !d_series)) return fail(fn, "null pointer", -1);
    if (sp::misaligned(d_rows, 16)) return fail(fn, "d_rows must be 16-byte aligned", -1);
    if (sp::misaligned(d_cand, 16)) return fail(fn, "d_cand must be 16-byte aligned", -1);
    if (sp::misaligned(d_series, 4)) return fail(fn, "d_series must be 4-byte aligned", -1);
    if (sp::misaligned(d_count, 4)) return fail(fn, "d_count must be 4-byte aligned", -1);
    if (sp::misaligned(d_ft, 4)) return fail(fn, "d_ft must be 4-byte aligned", -1);
    if (sp::misaligned(d_dmt, 4)) return fail(fn, "d_dmt must be 4-byte aligned", -1);
    if (sp::misaligned(d_info, 4)) return fail(fn, "d_info must be 4-byte aligned", -1);
    if (!p) return fail(fn, NULL_PLAN, -1);
    // what the plan decides; still before anything is asked of the device
    if (const char* why = sp::why_not_row_stride(in_stride, p->nchan)) return fail(fn, why, -1);
    if (const char* why = why_not_grids(max_cand, p->nchan, p->nx, p->nf, p->rq)) return fail(fn, why, -1);

    if (sp::use_device(fn, p)) return -3;
    Params k;
    k.rows = d_ft ? d_rows : nullptr;
    k.series = d_dmt ? d_series : nullptr;
    k.cand = d_cand;
    k.count = d_count;
    k.delays = p->d_delays;
    k.keep = p->d_keep;
    k.shape = p->d_shape;
    k.ft = d_ft;
    k.dmt = d_dmt;
    k.info = d_info;
    k.in_stride = in_stride;
    k.series_stride = series_stride;
    k.nsamp = (int)nsamp;
    k.nchan = p->nchan;
    k.ntrials = p->ntrials;
    k.K = p->nwidths;
    k.nx = p->nx;
    k.nf = p->nf;
    k.cpb = p->nchan / p->nf;
    k.per = subbands_per_group(k.cpb);
    k.xgroups = (int)xgroups_of(p->nx);
    k.fgroups = (int)fgroups_of(p->nchan, p->nf);
    k.rq = p->rq;
    k.dq = p->dq;
    k.ndm = 2 * p->rq + 1;
    k.max_cand = max_cand;
    k.info_from_dmt = d_ft ? 0 : 1;
    const hipError_t err = launch_cutout(k, stream_of(p->engine, stream));
    if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
    return 0;
}

}  // extern "C"
