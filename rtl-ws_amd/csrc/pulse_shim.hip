// pulse_shim.hip -- extern "C" glue of include/rtlws_pulse.h (librtlws_pulse.so): argument rules, the rows of LDS a
// table takes (pulse.h) and the table of its pieces, the plan, the launch, the signal-to-noise ratio.  The engine
// (device, stream) is librtlws_hip.so's; nothing here reads the environment, and nothing of a run is computed on the
// host: without a device there is no plan.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "pulse.h"
#include "rtlws_pulse.h"
#include "search_plan.h"

// The rows the table took and its pieces on the engine's device
struct rtlws_pulse_plan : rtlws::search::Plan {
    int nwidths;
    long seg;
    rtlws::pulse::Layout layout;
    int* d_table;
};

namespace {

using namespace rtlws::pulse;
namespace sp = rtlws::search;

static_assert(MAX_WIDTHS == RTLWS_PULSE_MAX_WIDTHS && MAX_WIDTH == RTLWS_PULSE_MAX_WIDTH && MIN_SEG == RTLWS_PULSE_MIN_SEG &&
                  MAX_SEG == RTLWS_PULSE_MAX_SEG && MAX_TRIALS == RTLWS_PULSE_MAX_TRIALS && MAX_NOUT == RTLWS_PULSE_MAX_NOUT &&
                  MAX_WIDTHS == sp::MAX_WIDTHS && MAX_TRIALS == sp::MAX_TRIALS,
              "rtlws_pulse.h, pulse.h and search_plan.h disagree");

// ---- the rules, each worded once ----
const char* why_not_table(int nwidths, const int32_t* widths, long seg)
{
    if (const char* why = sp::why_not_widths(nwidths, widths, MAX_WIDTH, "every width must be 1 .. 1024")) return why;
    if (seg < MIN_SEG || seg > MAX_SEG || seg % 4) return "seg must be 64 .. 1048576 and a multiple of 4";
    return nullptr;
}

const char* why_not_nout(long nout) { return nout < 0 || nout > MAX_NOUT ? "nout must be 0 .. 2^30" : nullptr; }

const char* why_not_grid(int ntrials, long nout, long seg) { return sp::why_not_grid(sp::ceil_div(nout, seg), ntrials); }

// ---- the rows of a table ----
Layout layout_of(int nwidths, const int32_t* widths)
{
    Layout l{};
    int bits = 0;
    for (int k = 0; k < nwidths; ++k) bits |= widths[k];
    l.w_max = widths[nwidths - 1];
    while ((2 << l.top) <= l.w_max) ++l.top;
    l.levels_kept = __builtin_popcount(bits);
    const int unused = l.top + 1 - l.levels_kept;
    l.rows = l.levels_kept + (unused < 2 ? unused : 2);
    const auto row_of = [&](int tile) { return (tile + l.w_max - 1 + 3) & ~3; };
    l.tile_out = MAX_TILE;
    while (l.tile_out > MIN_TILE && l.rows * row_of(l.tile_out) > LDS_WORDS[2]) l.tile_out /= 2;      // at 256 every table fits: 11 rows of 1280
    l.row = row_of(l.tile_out);
    const int words = l.rows * l.row > SCRATCH_WORDS ? l.rows * l.row : SCRATCH_WORDS;
    while (LDS_WORDS[l.lds] < words) ++l.lds;
    return l;
}

// pulse.h's table: a kept level's row is its rank among the kept ones, the others take the rows behind those in turn
std::vector<int> build_table(int nwidths, const int32_t* widths, const Layout& l)
{
    std::vector<int> table(TABLE_WORDS, 0);
    int bits = 0, kept = 0, others = 0;
    for (int k = 0; k < nwidths; ++k) bits |= widths[k];
    for (int a = 0; a <= l.top; ++a)
        table[LEVEL_ROW + a] = ((bits >> a & 1) ? kept++ : l.levels_kept + others++ % 2) * l.row;
    int next = PIECES;
    for (int k = 0; k < nwidths; ++k) {
        table[FIRST + k] = next;
        int offset = 0;
        for (int a = l.top; a >= 0; --a)
            if (widths[k] >> a & 1) {
                table[next++] = table[LEVEL_ROW + a] + offset;
                offset += 1 << a;
            }
    }
    table[FIRST + nwidths] = next;
    return table;
}

}  // namespace

extern "C" {

const char* rtlws_pulse_last_error(void) { return g_err.c_str(); }

int rtlws_pulse_supported(int nwidths, const int32_t* widths, long seg) { return supported("rtlws_pulse", why_not_table(nwidths, widths, seg)); }

int rtlws_pulse_geometry(int nwidths, const int32_t* widths, long seg, int ntrials, long nout, int* blocks, int* threads,
                         int* lds_bytes, int* tile_out, int* levels_kept, long* nseg)
{
    const char* fn = "rtlws_pulse_geometry";
    g_err.clear();
    if (const char* why = why_not_table(nwidths, widths, seg)) return fail(fn, why, -1);
    if (const char* why = sp::why_not_ntrials(ntrials)) return fail(fn, why, -1);
    if (const char* why = why_not_nout(nout)) return fail(fn, why, -1);
    if (const char* why = why_not_grid(ntrials, nout, seg)) return fail(fn, why, -1);
    const Layout l = layout_of(nwidths, widths);
    if (blocks) *blocks = (int)(sp::ceil_div(nout, seg) * ntrials);
    if (threads) *threads = THREADS;
    if (lds_bytes) *lds_bytes = LDS_WORDS[l.lds] * 4;
    if (tile_out) *tile_out = l.tile_out;
    if (levels_kept) *levels_kept = l.levels_kept;
    if (nseg) *nseg = sp::ceil_div(nout, seg);
    return 0;
}

rtlws_pulse_plan* rtlws_pulse_open(rtlws_engine* e, int nwidths, const int32_t* widths, long seg)
{
    const auto fill = [&](rtlws_pulse_plan& p) {
        p.nwidths = nwidths, p.seg = seg, p.layout = layout_of(nwidths, widths);
        const std::vector<int> table = build_table(nwidths, widths, p.layout);
        const hipError_t err = sp::upload(&p.d_table, table.data(), table.size());
        return err == hipSuccess ? prepare_pulse(p.layout) : err;
    };
    return sp::open_plan<rtlws_pulse_plan>("rtlws_pulse_open", why_not_table(nwidths, widths, seg), e, fill, "the table or the kernel", rtlws_pulse_close);
}

void rtlws_pulse_close(rtlws_pulse_plan* p) { sp::close_plan(p, &rtlws_pulse_plan::d_table); }

long rtlws_pulse_samples_needed(const rtlws_pulse_plan* p, long nout)
{
    const char* fn = "rtlws_pulse_samples_needed";
    g_err.clear();
    if (const char* why = why_not_nout(nout)) return fail(fn, why, -1);
    if (!p) return fail(fn, NULL_PLAN, -1);
    return nout ? nout + p->layout.w_max - 1 : 0;
}

long rtlws_pulse_segments(const rtlws_pulse_plan* p, long nout)
{
    const char* fn = "rtlws_pulse_segments";
    g_err.clear();
    if (const char* why = why_not_nout(nout)) return fail(fn, why, -1);
    if (!p) return fail(fn, NULL_PLAN, -1);
    return sp::ceil_div(nout, p->seg);
}

int rtlws_pulse_run(rtlws_pulse_plan* p, const float* d_in, long in_stride, int ntrials, long nout, float* d_peak, int32_t* d_at,
                    double* d_mom, void* stream)
{
    const char* fn = "rtlws_pulse_run";
    g_err.clear();
    // what needs no plan: a trial holds at least its nout samples
    if (const char* why = sp::why_not_ntrials(ntrials)) return fail(fn, why, -1);
    if (const char* why = why_not_nout(nout)) return fail(fn, why, -1);
    if (in_stride < nout) return fail(fn, "in_stride must be >= samples_needed", -1);
    if (const char* why = sp::why_not_stride(in_stride)) return fail(fn, why, -1);
    if (nout > 0 && (!d_in || !d_peak || !d_at)) return fail(fn, "null pointer", -1);
    if (sp::misaligned(d_in, 16)) return fail(fn, "d_in must be 16-byte aligned", -1);
    if (sp::misaligned(d_peak, 4)) return fail(fn, "d_peak must be 4-byte aligned", -1);
    if (sp::misaligned(d_at, 4)) return fail(fn, "d_at must be 4-byte aligned", -1);
    if (sp::misaligned(d_mom, 8)) return fail(fn, "d_mom must be 8-byte aligned", -1);
    if (!p) return fail(fn, NULL_PLAN, -1);
    // what the plan decides; still before anything is asked of the device
    const long need = nout ? nout + p->layout.w_max - 1 : 0;
    if (in_stride < need) return fail(fn, "in_stride must be >= samples_needed", -1);
    if (const char* why = why_not_grid(ntrials, nout, p->seg)) return fail(fn, why, -1);
    if (nout == 0) return 0;

    if (sp::use_device(fn, p)) return -3;
    Params kp;
    kp.in = d_in;
    kp.peak = d_peak;
    kp.at = d_at;
    kp.mom = d_mom;
    kp.table = p->d_table;
    kp.in_stride = in_stride;
    kp.nout = nout;
    kp.seg = p->seg;
    kp.nseg = sp::ceil_div(nout, p->seg);
    kp.need = need;
    kp.nwidths = p->nwidths;
    kp.top = p->layout.top;
    kp.w_max = p->layout.w_max;
    const hipError_t err = launch_pulse(p->layout, kp, ntrials, stream_of(p->engine, stream));
    if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
    return 0;
}

double rtlws_pulse_snr(double peak, int width, double sum1, double sum2, long count)
{
    double mean, var;
    if (width < 1 || !sp::moments(sum1, sum2, count, &mean, &var)) return std::numeric_limits<double>::quiet_NaN();
    return (peak - (double)width * mean) / std::sqrt((double)width * var);
}

}  // extern "C"
