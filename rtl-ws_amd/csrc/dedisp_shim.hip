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
#include "shim_common.h"

// The form the table took and its tables on the engine's device
struct rtlws_dedisp_plan {
    rtlws_engine* engine;
    int device;
    int nchan, ntrials, max_delay;
    rtlws::dedisp::Layout layout;
    int2* d_units;
    int* d_rel;
};

namespace {

using namespace rtlws::dedisp;

static_assert(MIN_NCHAN == RTLWS_DEDISP_MIN_NCHAN && MAX_NCHAN == RTLWS_DEDISP_MAX_NCHAN && MAX_TRIALS == RTLWS_DEDISP_MAX_TRIALS &&
                  MAX_DELAY == RTLWS_DEDISP_MAX_DELAY,
              "rtlws_dedisp.h and dedisp.h disagree");

// ---- the rules, each worded once ----
const char* why_not_shape(int nchan, int ntrials)
{
    if (nchan < MIN_NCHAN || nchan > MAX_NCHAN || nchan % 4) return "nchan must be 4 .. 4096 and a multiple of 4";
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

long groups_of(int ntrials, int trials) { return (ntrials + trials - 1) / trials; }

const char* why_not_grid(long nout, int ntrials, const Layout& l)
{
    return (nout + TILE_OUT - 1) / TILE_OUT > INT_MAX / groups_of(ntrials, l.trials) ? "more workgroups than one grid holds" : nullptr;
}

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

void free_tables(int2* d_units, int* d_rel)
{
    if (d_units) (void)hipFree(d_units);
    if (d_rel) (void)hipFree(d_rel);
}

}  // namespace

extern "C" {

const char* rtlws_dedisp_last_error(void) { return g_err.c_str(); }

int rtlws_dedisp_supported(int nchan, int ntrials)
{
    g_err.clear();
    const char* why = why_not_shape(nchan, ntrials);
    if (why) fail("rtlws_dedisp", why, 0);
    return why ? 0 : 1;
}

int rtlws_dedisp_delays(int nchan, int shifted, double f_centre_hz, double bandwidth_hz, double row_seconds, int ntrials,
                        double dm0, double dm_step, int32_t* delays)
{
    const char* fn = "rtlws_dedisp_delays";
    g_err.clear();
    if (const char* why = why_not_shape(nchan, ntrials)) return fail(fn, why, -1);
    if (shifted != 0 && shifted != 1) return fail(fn, "shifted must be 0 or 1", -1);
    if (!delays) return fail(fn, "null delays", -1);
    if (!(std::isfinite(bandwidth_hz) && bandwidth_hz > 0.0)) return fail(fn, "bandwidth_hz must be finite and > 0", -1);
    if (!(std::isfinite(row_seconds) && row_seconds > 0.0)) return fail(fn, "row_seconds must be finite and > 0", -1);
    const int M = nchan;
    // the lowest channel is c = M / 2, half the band below the centre
    if (!(std::isfinite(f_centre_hz) && f_centre_hz + (double)(M / 2 - M) * bandwidth_hz / (double)M > 0.0))
        return fail(fn, "every channel's frequency must be finite and > 0", -1);
    std::vector<double> excess(M);                            // nu_i^-2 - nu_max^-2, nu in MHz
    const double top = (f_centre_hz + (double)(M / 2 - 1) * bandwidth_hz / (double)M) / 1e6;
    for (int i = 0; i < M; ++i) {
        const int c = shifted ? (i + M / 2) % M : i;
        const double nu = (f_centre_hz + (double)(c < M / 2 ? c : c - M) * bandwidth_hz / (double)M) / 1e6;
        excess[i] = 1.0 / (nu * nu) - 1.0 / (top * top);
    }
    for (int t = 0; t < ntrials; ++t) {
        const double dm = dm0 + (double)t * dm_step;
        char buf[96];
        if (!(std::isfinite(dm) && dm >= 0.0)) {
            snprintf(buf, sizeof buf, "trial %d: the dispersion measure must be finite and >= 0", t);
            return fail(fn, buf, -1);
        }
        for (int i = 0; i < M; ++i) {
            const double d = std::rint(4.148808e3 * dm * excess[i] / row_seconds);
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
    if (blocks) *blocks = (int)((nout + TILE_OUT - 1) / TILE_OUT * groups_of(ntrials, l.trials));
    if (threads) *threads = THREADS;
    if (lds_bytes) *lds_bytes = rtlws::dedisp::lds_bytes(l);
    if (tile_out) *tile_out = TILE_OUT;
    if (trials_per_block) *trials_per_block = l.trials;
    if (max_delay) *max_delay = most;
    return 0;
}

rtlws_dedisp_plan* rtlws_dedisp_open(rtlws_engine* e, int nchan, int ntrials, const int32_t* delays, const uint8_t* mask)
{
    const char* fn = "rtlws_dedisp_open";
    g_err.clear();
    int most = 0;
    const int device = open_device(fn, why_not_table(nchan, ntrials, delays, mask, &most), e);
    if (device < 0) return nullptr;
    const Layout l = choose_layout(nchan, ntrials, delays, mask);
    std::vector<int2> units;
    std::vector<int> rel;
    build_tables(nchan, ntrials, delays, mask, l, &units, &rel);
    int2* d_units = nullptr;
    int* d_rel = nullptr;
    hipError_t err = hipMalloc(reinterpret_cast<void**>(&d_units), units.size() * sizeof(int2));
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&d_rel), rel.size() * sizeof(int));
    if (err == hipSuccess) err = hipMemcpy(d_units, units.data(), units.size() * sizeof(int2), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(d_rel, rel.data(), rel.size() * sizeof(int), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = prepare_dedisp(l);
    if (err != hipSuccess) {
        free_tables(d_units, d_rel);
        fail_hip(fn, "the tables or the kernel", err);
        return nullptr;
    }
    return new rtlws_dedisp_plan{e, device, nchan, ntrials, most, l, d_units, d_rel};
}

void rtlws_dedisp_close(rtlws_dedisp_plan* p)
{
    if (!p) return;
    if (hipSetDevice(p->device) == hipSuccess) free_tables(p->d_units, p->d_rel);
    delete p;
}

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
    if (in_stride < MIN_NCHAN) return fail(fn, "in_stride must be >= nchan", -1);
    if (in_stride % 4) return fail(fn, "in_stride must be a multiple of 4", -1);
    if (out_stride < nout) return fail(fn, "out_stride must be >= nout", -1);
    if (nout > 0 && (!d_rows || !d_out)) return fail(fn, "null pointer", -1);
    if (reinterpret_cast<uintptr_t>(d_rows) & 15u) return fail(fn, "d_rows must be 16-byte aligned", -1);
    if (reinterpret_cast<uintptr_t>(d_out) & 3u) return fail(fn, "d_out must be 4-byte aligned", -1);
    if (!p) return fail(fn, NULL_PLAN, -1);
    // what the plan decides; still before anything is asked of the device
    if (in_stride < p->nchan) return fail(fn, "in_stride must be >= nchan", -1);
    if (const char* why = why_not_grid(nout, p->ntrials, p->layout)) return fail(fn, why, -1);
    if (nout == 0) return 0;

    hipError_t err = hipSetDevice(p->device);
    if (err != hipSuccess) return fail_hip(fn, "hipSetDevice", err);
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
    err = launch_dedisp(p->layout, kp, stream_of(p->engine, stream));
    if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
    return 0;
}

}  // extern "C"
