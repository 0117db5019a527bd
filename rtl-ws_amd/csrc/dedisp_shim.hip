// dedisp_shim.hip -- extern "C" glue of include/rtlws_dedisp.h (librtlws_dedisp.so): argument rules, the delay
// formula, the plan (the choice of a table's form and the tables of that form: dedisp_form.h), the launch.  The engine
// (device, stream) is librtlws_hip.so's; nothing here reads the environment, and nothing of a run is computed on the
// host: without a device there is no plan.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "dedisp.h"
#include "dedisp_form.h"
#include "rtlws_dedisp.h"
#include "search_plan.h"

// The form the table took and its tables on the engine's device
struct rtlws_dedisp_plan : rtlws::search::Plan {
    int nchan, ntrials, max_delay;
    rtlws::dedisp::Layout layout;
    int2* d_units;
    int* d_rel;
};

namespace {

using namespace rtlws::dedisp;
namespace sp = rtlws::search;

static_assert(MIN_NCHAN == RTLWS_DEDISP_MIN_NCHAN && MAX_NCHAN == RTLWS_DEDISP_MAX_NCHAN && MAX_TRIALS == RTLWS_DEDISP_MAX_TRIALS &&
                  MAX_DELAY == RTLWS_DEDISP_MAX_DELAY && MIN_NCHAN == sp::MIN_NCHAN && MAX_NCHAN == sp::MAX_NCHAN,
              "rtlws_dedisp.h, dedisp.h and search_plan.h disagree");

// ---- the rules, each worded once ----
const char* why_not_shape(int nchan, int ntrials)
{
    if (const char* why = sp::why_not_nchan(nchan)) return why;
    if (ntrials < 1 || ntrials > MAX_TRIALS) return WHY_NTRIALS;
    return nullptr;
}

// the shape, then the table's entries; *max_delay: the largest over the positions the mask keeps
const char* why_not_table(int nchan, int ntrials, const int32_t* delays, const uint8_t* mask, int* max_delay)
{
    if (const char* why = why_not_shape(nchan, ntrials)) return why;
    if (!delays) return WHY_NULL_DELAYS;
    int most = 0;
    for (long t = 0; t < ntrials; ++t)
        for (int i = 0; i < nchan; ++i) {
            const int32_t d = delays[t * nchan + i];
            if (d < 0 || d > MAX_DELAY) return WHY_DELAY;
            if ((!mask || mask[i]) && d > most) most = d;
        }
    *max_delay = most;
    return nullptr;
}

const char* why_not_nout(long nout) { return nout < 0 ? "nout must be >= 0" : nullptr; }

const char* why_not_grid(long nout, int ntrials, const Layout& l) { return sp::why_not_grid(sp::ceil_div(nout, TILE_OUT), groups_of(ntrials, l.trials)); }

}  // namespace

extern "C" {

const char* rtlws_dedisp_last_error(void) { return g_err.c_str(); }

int rtlws_dedisp_supported(int nchan, int ntrials) { return supported("rtlws_dedisp", why_not_shape(nchan, ntrials)); }

int rtlws_dedisp_delays(int nchan, int shifted, double f_centre_hz, double bandwidth_hz, double row_seconds, int ntrials,
                        double dm0, double dm_step, int32_t* delays)
{
    const char* fn = "rtlws_dedisp_delays";
    g_err.clear();
    if (const char* why = why_not_shape(nchan, ntrials)) return fail(fn, why, -1);
    if (shifted != 0 && shifted != 1) return fail(fn, WHY_SHIFTED, -1);
    if (!delays) return fail(fn, WHY_NULL_DELAYS, -1);
    if (const char* why = sp::why_not_band(nchan, f_centre_hz, bandwidth_hz, row_seconds)) return fail(fn, why, -1);
    const int M = nchan;
    const std::vector<double> excess = sp::excess(M, shifted, f_centre_hz, bandwidth_hz);
    for (int t = 0; t < ntrials; ++t) {
        const double dm = dm0 + (double)t * dm_step;
        char buf[96];
        if (!(std::isfinite(dm) && dm >= 0.0)) {
            snprintf(buf, sizeof buf, WHY_DM, t);
            return fail(fn, buf, -1);
        }
        for (int i = 0; i < M; ++i) {
            const double d = std::rint(sp::DISPERSION * dm * excess[i] / row_seconds);
            if (!(d <= (double)MAX_DELAY)) {
                snprintf(buf, sizeof buf, WHY_SWEEP, "trial", t);
                return fail(fn, buf, -1);
            }
            delays[(long)t * M + i] = (int32_t)d;
        }
    }
    return 0;
}

int rtlws_dedisp_geometry(int nchan, int ntrials, const int32_t* delays, const uint8_t* mask, long nout, int* blocks, int* threads,
                          int* lds_bytes, int* tile_out, int* trials_per_block, int* max_delay)
{
    const char* fn = "rtlws_dedisp_geometry";
    g_err.clear();
    int most = 0;
    if (const char* why = why_not_table(nchan, ntrials, delays, mask, &most)) return fail(fn, why, -1);
    if (const char* why = why_not_nout(nout)) return fail(fn, why, -1);
    const Layout l = choose_layout(nchan, ntrials, delays, mask);
    if (const char* why = why_not_grid(nout, ntrials, l)) return fail(fn, why, -1);
    if (blocks) *blocks = (int)(sp::ceil_div(nout, TILE_OUT) * groups_of(ntrials, l.trials));
    if (threads) *threads = THREADS;
    if (lds_bytes) *lds_bytes = rtlws::dedisp::lds_bytes(l);
    if (tile_out) *tile_out = TILE_OUT;
    if (trials_per_block) *trials_per_block = l.trials;
    if (max_delay) *max_delay = most;
    return 0;
}

rtlws_dedisp_plan* rtlws_dedisp_open(rtlws_engine* e, int nchan, int ntrials, const int32_t* delays, const uint8_t* mask)
{
    int most = 0;
    const char* why = why_not_table(nchan, ntrials, delays, mask, &most);
    const auto fill = [&](rtlws_dedisp_plan& p) {
        p.nchan = nchan, p.ntrials = ntrials, p.max_delay = most;
        p.layout = choose_layout(nchan, ntrials, delays, mask);
        std::vector<int2> units;
        std::vector<int> rel;
        build_tables(nchan, ntrials, delays, mask, p.layout, &units, &rel);
        hipError_t err = sp::upload(&p.d_units, units.data(), units.size());
        if (err == hipSuccess) err = sp::upload(&p.d_rel, rel.data(), rel.size());
        return err == hipSuccess ? prepare_dedisp(p.layout) : err;
    };
    return sp::open_plan<rtlws_dedisp_plan>("rtlws_dedisp_open", why, e, fill, "the tables or the kernel", rtlws_dedisp_close);
}

void rtlws_dedisp_close(rtlws_dedisp_plan* p) { sp::close_plan(p, &rtlws_dedisp_plan::d_units, &rtlws_dedisp_plan::d_rel); }

long rtlws_dedisp_rows_needed(const rtlws_dedisp_plan* p, long nout)
{
    const char* fn = "rtlws_dedisp_rows_needed";
    g_err.clear();
    if (const char* why = why_not_nout(nout)) return fail(fn, why, -1);
    if (!p) return fail(fn, NULL_PLAN, -1);
    return nout ? nout + p->max_delay : 0;
}

int rtlws_dedisp_run(rtlws_dedisp_plan* p, const float* d_rows, long in_stride, long nout, float* d_out, long out_stride, void* stream)
{
    const char* fn = "rtlws_dedisp_run";
    g_err.clear();
    // what needs no plan: a row holds at least 4 values
    if (const char* why = why_not_nout(nout)) return fail(fn, why, -1);
    if (const char* why = sp::why_not_row_stride(in_stride, MIN_NCHAN)) return fail(fn, why, -1);
    if (const char* why = sp::why_not_stride(in_stride)) return fail(fn, why, -1);
    if (out_stride < nout) return fail(fn, "out_stride must be >= nout", -1);
    if (nout > 0 && (!d_rows || !d_out)) return fail(fn, "null pointer", -1);
    if (sp::misaligned(d_rows, 16)) return fail(fn, "d_rows must be 16-byte aligned", -1);
    if (sp::misaligned(d_out, 4)) return fail(fn, "d_out must be 4-byte aligned", -1);
    if (!p) return fail(fn, NULL_PLAN, -1);
    // what the plan decides; still before anything is asked of the device
    if (const char* why = sp::why_not_row_stride(in_stride, p->nchan)) return fail(fn, why, -1);
    if (const char* why = why_not_grid(nout, p->ntrials, p->layout)) return fail(fn, why, -1);
    if (nout == 0) return 0;

    if (sp::use_device(fn, p)) return -3;
    Params kp;
    kp.rows = d_rows;
    kp.out = d_out;
    kp.units = p->d_units;
    kp.rel = p->d_rel;
    kp.in_stride = in_stride;
    kp.nout = nout;
    kp.out_stride = out_stride;
    kp.rows_needed = nout + p->max_delay;
    kp.nchan = p->nchan;
    kp.ntrials = p->ntrials;
    kp.ngroups = (int)groups_of(p->ntrials, p->layout.trials);
    kp.chunk = p->layout.chunk;
    kp.stride = p->layout.stride;
    const hipError_t err = launch_dedisp(p->layout, kp, stream_of(p->engine, stream));
    if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
    return 0;
}

}  // extern "C"
