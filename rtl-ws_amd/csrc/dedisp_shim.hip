// dedisp_shim.hip -- extern "C" glue of include/rtlws_dedisp.h (librtlws_dedisp.so): argument rules, the delay
// formula, the choice of a table's form (dedisp.h) and the tables of that form, the plan, the launch.  The engine
// (device, stream) is librtlws_hip.so's; nothing here reads the environment, and nothing of a run is computed on the
// host: without a device there is no plan.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "dedisp.h"
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
    if (ntrials < 1 || ntrials > MAX_TRIALS) return "ntrials must be 1 .. 4096";
    return nullptr;
}

// the shape, then the table's entries; *max_delay: the largest over the positions the mask keeps
const char* why_not_table(int nchan, int ntrials, const int32_t* delays, const uint8_t* mask, int* max_delay)
{
    if (const char* why = why_not_shape(nchan, ntrials)) return why;
    if (!delays) return "null delays";
    int most = 0;
    for (long t = 0; t < ntrials; ++t)
        for (int i = 0; i < nchan; ++i) {
            const int32_t d = delays[t * nchan + i];
            if (d < 0 || d > MAX_DELAY) return "every delay must be 0 .. 65535";
            if ((!mask || mask[i]) && d > most) most = d;
        }
    *max_delay = most;
    return nullptr;
}

const char* why_not_nout(long nout) { return nout < 0 ? "nout must be >= 0" : nullptr; }

long groups_of(int ntrials, int trials) { return sp::ceil_div(ntrials, trials); }

const char* why_not_grid(long nout, int ntrials, const Layout& l) { return sp::why_not_grid(sp::ceil_div(nout, TILE_OUT), groups_of(ntrials, l.trials)); }

// ---- the form of a table ----
// The least and the largest delay of positions i0 .. i0 + width - 1 under trials t0 .. t0 + trials - 1 (those of them
// there are), over the positions the mask keeps; false where it keeps none
bool unit_range(int nchan, int ntrials, const int32_t* delays, const uint8_t* mask, int t0, int trials, int i0, int width, int* lo, int* hi)
{
    int least = INT_MAX, most = -1;
    for (int i = i0; i < i0 + width; ++i) {
        if (mask && !mask[i]) continue;
        for (int t = t0; t < t0 + trials && t < ntrials; ++t) {
            const int d = delays[(long)t * nchan + i];
            least = d < least ? d : least;
            most = d > most ? d : most;
        }
    }
    *lo = least;
    *hi = most;
    return most >= 0;
}

// the widest spread of delays inside a unit of `width` positions and a group of `trials` trials
int widest_spread(int nchan, int ntrials, const int32_t* delays, const uint8_t* mask, int trials, int width)
{
    int widest = 0;
    for (int t0 = 0; t0 < ntrials; t0 += trials)
        for (int i0 = 0; i0 < nchan; i0 += width) {
            int lo, hi;
            if (unit_range(nchan, ntrials, delays, mask, t0, trials, i0, width, &lo, &hi) && hi - lo > widest) widest = hi - lo;
        }
    return widest;
}

// chunk positions of columns as long as `height`, in the smaller LDS where they fit, else the larger; false: in neither
bool fits(int trials, int chunk, int height, Layout* l)
{
    const int stride = fit_stride(height, chunk / 4);
    const long words = (long)chunk * stride + TILE_OUT;
    if (words > BIG_WORDS) return false;
    *l = Layout{trials, 0, words > SMALL_WORDS, chunk, stride};
    return true;
}

// The largest group of 8, 4, 2, 1 trials (no larger than ntrials fills half of) whose windows fit beside whole
// 128-byte pieces of the rows; one trial with narrower pieces; one trial, every position by itself (a column is then
// TILE_OUT rows whatever the table)
Layout choose_layout(int nchan, int ntrials, const int32_t* delays, const uint8_t* mask)
{
    Layout l;
    for (int trials = MAX_TRIALS_PER_BLOCK; trials >= 1; trials /= 2) {
        if (trials > 1 && trials >= 2 * ntrials) continue;
        const int height = TILE_OUT + widest_spread(nchan, ntrials, delays, mask, trials, 4);
        for (int chunk = MAX_CHUNK; chunk >= (trials > 1 ? MAX_CHUNK : 4); chunk /= 2)
            if (fits(trials, chunk, height, &l)) return l;
    }
    return Layout{1, 1, 0, MAX_CHUNK, fit_stride(TILE_OUT, MAX_CHUNK / 4)};
}

// the tables of dedisp.h's Params for a form
void build_tables(int nchan, int ntrials, const int32_t* delays, const uint8_t* mask, const Layout& l, std::vector<int2>* units,
                  std::vector<int>* rel)
{
    const int width = l.lone ? 1 : 4, per_group = nchan / width;
    const long groups = groups_of(ntrials, l.trials);
    units->assign(groups * per_group, make_int2(-1, 0));
    rel->assign(groups * nchan * l.trials, l.chunk * l.stride);
    for (long g = 0; g < groups; ++g)
        for (int u = 0; u < per_group; ++u) {
            int lo, hi;
            if (!unit_range(nchan, ntrials, delays, mask, (int)g * l.trials, l.trials, u * width, width, &lo, &hi)) continue;
            (*units)[g * per_group + u] = make_int2(lo, hi - lo);
            for (int i = u * width; i < (u + 1) * width; ++i) {
                if (mask && !mask[i]) continue;
                for (int k = 0; k < l.trials; ++k) {
                    const long t = g * l.trials + k < ntrials ? g * l.trials + k : ntrials - 1;      // past the table: the last trial again
                    (*rel)[(g * nchan + i) * l.trials + k] = i % l.chunk * l.stride + delays[t * nchan + i] - lo;
                }
            }
        }
}

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
    if (shifted != 0 && shifted != 1) return fail(fn, "shifted must be 0 or 1", -1);
    if (!delays) return fail(fn, "null delays", -1);
    if (const char* why = sp::why_not_band(nchan, f_centre_hz, bandwidth_hz, row_seconds)) return fail(fn, why, -1);
    const int M = nchan;
    const std::vector<double> excess = sp::excess(M, shifted, f_centre_hz, bandwidth_hz);
    for (int t = 0; t < ntrials; ++t) {
        const double dm = dm0 + (double)t * dm_step;
        char buf[96];
        if (!(std::isfinite(dm) && dm >= 0.0)) {
            snprintf(buf, sizeof buf, "trial %d: the dispersion measure must be finite and >= 0", t);
            return fail(fn, buf, -1);
        }
        for (int i = 0; i < M; ++i) {
            const double d = std::rint(sp::DISPERSION * dm * excess[i] / row_seconds);
            if (!(d <= (double)MAX_DELAY)) {
                snprintf(buf, sizeof buf, "trial %d: a delay above 65535 rows", t);
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
