// ffa_shim.hip -- extern "C" glue of include/rtlws_ffa.h (librtlws_ffa.so): argument rules, the split of the stages into
// passes and their LDS (ffa.h), the plan with its table and workspace, the groups of a run and their launches, and the
// host's helpers (the period of a row, the signal-to-noise ratio of a peak).  The engine (device, stream) is
// librtlws_hip.so's; nothing here reads the environment, and nothing of a run is computed on the host: without a
// device there is no plan.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <limits>

#include "ffa.h"
#include "rtlws_ffa.h"
#include "search_plan.h"

// The table and the workspace on the engine's device
struct rtlws_ffa_plan : rtlws::search::Plan {
    int p0, nper, L, nwidths, seg_log2, top;
    rtlws::ffa::Split split;
    int eval_log2;             // of the last pass
    bool merge;
    int pairs;                 // (trial, base period) pairs in flight
    size_t pair_bytes, ws_bytes;
    int* d_table;
    char* d_ws;                // rows [2 or fewer][pairs][m * pitch] f32, then the partial pairs: best, then at
};

namespace {

using namespace rtlws::ffa;
namespace sp = rtlws::search;
using sp::log2_of;

static_assert(MIN_P == RTLWS_FFA_MIN_P && MAX_P == RTLWS_FFA_MAX_P && MAX_L == RTLWS_FFA_MAX_L && MAX_CELLS == RTLWS_FFA_MAX_CELLS &&
                  MAX_WIDTHS == RTLWS_FFA_MAX_WIDTHS && MAX_WIDTH == RTLWS_FFA_MAX_WIDTH && MAX_TRIALS == RTLWS_FFA_MAX_TRIALS &&
                  MAX_PASSES == RTLWS_FFA_MAX_PASSES && WORKSPACE_CAP == RTLWS_FFA_WORKSPACE_CAP && MAX_WIDTHS == sp::MAX_WIDTHS &&
                  MAX_TRIALS == sp::MAX_TRIALS,
              "rtlws_ffa.h, ffa.h and search_plan.h disagree");

// ---- the rules, each worded once ----
const char* why_not_plan(int p0, int nper, int L, int nwidths, const int32_t* widths, int seg)
{
    if (p0 < MIN_P) return "p0 must be >= 16";
    if (nper < 1) return "nper must be >= 1";
    if (nper > MAX_P || p0 + nper - 1 > MAX_P) return "p0 + nper - 1 must be <= 1024";
    if (L < 1 || L > MAX_L) return "L must be 1 .. 12";
    if (((long)(p0 + nper - 1) << L) > MAX_CELLS) return "m * (p0 + nper - 1) must be <= 2^22";
    if (const char* why = sp::why_not_widths(nwidths, widths, p0 < MAX_WIDTH ? p0 : MAX_WIDTH, "a width must be 1 .. min(256, p0)")) return why;
    if (seg < 1 || seg > (1 << L) || (seg & (seg - 1))) return "seg must be a power of two 1 .. m";
    return nullptr;
}

const char* why_not_max_trials(int max_trials) { return max_trials < 1 ? "max_trials must be >= 1" : nullptr; }

// what a plan of these (served) arguments is, but for the device's side
rtlws_ffa_plan shape_of(int p0, int nper, int L, int nwidths, const int32_t* widths, int seg, int max_trials)
{
    rtlws_ffa_plan p{};
    const int pitch = p0 + nper - 1;
    p.p0 = p0, p.nper = nper, p.L = L, p.nwidths = nwidths, p.seg_log2 = log2_of(seg);
    p.top = log2_of(widths[nwidths - 1] + 1) - 1;             // floor(log2 w_max)
    p.split = split_of(L, pitch);
    const int last = p.split.stages[p.split.passes - 1];
    p.eval_log2 = eval_waves_log2(last, pitch, p.top);
    p.merge = p.seg_log2 > last;
    p.pair_bytes = (size_t)(p.split.passes - 1) * ((size_t)pitch << L) * sizeof(float) +
                   (p.merge ? ((size_t)nwidths << (L - last)) * 8 : 0);
    long pairs = (long)max_trials * nper;
    if (pairs > MAX_PAIRS) pairs = MAX_PAIRS;
    if (p.pair_bytes && pairs > (long)(WORKSPACE_CAP / p.pair_bytes)) pairs = (long)(WORKSPACE_CAP / p.pair_bytes);
    p.pairs = pairs < 1 ? 1 : (int)pairs;
    p.ws_bytes = p.pairs * p.pair_bytes;
    return p;
}

size_t lds_of(const rtlws_ffa_plan& p, int pass)
{
    const int pitch = p.p0 + p.nper - 1, n = p.split.stages[pass];
    return pass == p.split.passes - 1 ? last_lds_bytes(n, pitch, 1 << p.eval_log2, p.top) : stage_lds_bytes(n, pitch);
}

// the table of ffa.h: every width's pieces, highest bit first
void fill_table(int nwidths, const int32_t* widths, int* t)
{
    int at = PIECES;
    for (int k = 0; k < nwidths; ++k) {
        t[FIRST + k] = at;
        int offset = 0;
        for (int level = 8; level >= 0; --level)
            if (widths[k] >> level & 1) {
                t[at++] = (level << 16) | offset;
                offset += 1 << level;
            }
    }
    t[FIRST + nwidths] = at;
}

}  // namespace

extern "C" {

const char* rtlws_ffa_last_error(void) { return g_err.c_str(); }

int rtlws_ffa_supported(int p0, int nper, int L, int nwidths, const int32_t* widths, int seg)
{
    return supported("rtlws_ffa", why_not_plan(p0, nper, L, nwidths, widths, seg));
}

int rtlws_ffa_geometry(int p0, int nper, int L, int nwidths, const int32_t* widths, int seg, int max_trials, int* passes,
                       int* stages, int* blocks, int* threads, int* lds_bytes, int* merge, size_t* workspace_bytes, int* pairs)
{
    const char* fn = "rtlws_ffa_geometry";
    g_err.clear();
    if (const char* why = why_not_plan(p0, nper, L, nwidths, widths, seg)) return fail(fn, why, -1);
    if (const char* why = why_not_max_trials(max_trials)) return fail(fn, why, -1);
    const rtlws_ffa_plan p = shape_of(p0, nper, L, nwidths, widths, seg, max_trials);
    if (passes) *passes = p.split.passes;
    for (int k = 0; k < MAX_PASSES; ++k) {
        const bool has = k < p.split.passes;
        if (stages) stages[k] = p.split.stages[k];
        if (blocks) blocks[k] = has ? 1 << (L - p.split.stages[k]) : 0;
        if (lds_bytes) lds_bytes[k] = has ? (int)lds_of(p, k) : 0;
    }
    if (threads) *threads = THREADS;
    if (merge) *merge = p.merge ? 1 : 0;
    if (workspace_bytes) *workspace_bytes = p.ws_bytes;
    if (pairs) *pairs = p.pairs;
    return 0;
}

rtlws_ffa_plan* rtlws_ffa_open(rtlws_engine* e, int p0, int nper, int L, int nwidths, const int32_t* widths, int seg, int max_trials)
{
    const char* why = why_not_plan(p0, nper, L, nwidths, widths, seg);
    if (!why) why = why_not_max_trials(max_trials);
    const auto fill = [&](rtlws_ffa_plan& p) {
        const sp::Plan head = p;                              // shape_of gives a whole plan but for the device's side
        p = shape_of(p0, nper, L, nwidths, widths, seg, max_trials);
        static_cast<sp::Plan&>(p) = head;
        int table[TABLE_WORDS] = {};
        fill_table(nwidths, widths, table);
        hipError_t err = sp::upload(&p.d_table, table, TABLE_WORDS);
        if (err == hipSuccess && p.ws_bytes) err = hipMalloc(reinterpret_cast<void**>(&p.d_ws), p.ws_bytes);
        return err == hipSuccess ? prepare(p.device) : err;
    };
    return sp::open_plan<rtlws_ffa_plan>("rtlws_ffa_open", why, e, fill, "the table, the workspace or the kernels", rtlws_ffa_close);
}

void rtlws_ffa_close(rtlws_ffa_plan* p) { sp::close_plan(p, &rtlws_ffa_plan::d_table, &rtlws_ffa_plan::d_ws); }

long rtlws_ffa_samples_needed(const rtlws_ffa_plan* p)
{
    g_err.clear();
    if (!p) return fail("rtlws_ffa_samples_needed", NULL_PLAN, -1);
    return (long)(p->p0 + p->nper - 1) << p->L;
}

size_t rtlws_ffa_workspace_bytes(const rtlws_ffa_plan* p) { return p ? p->ws_bytes : 0; }

int rtlws_ffa_run(rtlws_ffa_plan* p, const float* d_in, long in_stride, int ntrials, float* d_peak, int32_t* d_at, float* d_prof,
                  long prof_stride, void* stream)
{
    const char* fn = "rtlws_ffa_run";
    g_err.clear();
    // what needs no plan
    if (const char* why = sp::why_not_ntrials(ntrials)) return fail(fn, why, -1);
    if (const char* why = sp::why_not_stride(in_stride)) return fail(fn, why, -1);
    if (!d_in || !d_peak || !d_at) return fail(fn, "null pointer", -1);
    if (sp::misaligned(d_in, 16)) return fail(fn, "d_in must be 16-byte aligned", -1);
    if (sp::misaligned(d_peak, 4)) return fail(fn, "d_peak must be 4-byte aligned", -1);
    if (sp::misaligned(d_at, 4)) return fail(fn, "d_at must be 4-byte aligned", -1);
    if (sp::misaligned(d_prof, 4)) return fail(fn, "d_prof must be 4-byte aligned", -1);
    if (!p) return fail(fn, NULL_PLAN, -1);
    // what the plan decides; still before anything is asked of the device
    const int pitch = p->p0 + p->nper - 1;
    if (in_stride < ((long)pitch << p->L)) return fail(fn, "in_stride must be >= samples_needed", -1);
    if (d_prof && prof_stride < pitch) return fail(fn, "prof_stride must be >= p0 + nper - 1", -1);

    if (sp::use_device(fn, p)) return -3;
    const hipStream_t st = stream_of(p->engine, stream);
    const int passes = p->split.passes, last = p->split.stages[passes - 1];
    const size_t rows_bytes = (size_t)p->pairs * ((size_t)pitch << p->L) * sizeof(float);
    char* const parts = p->d_ws + (size_t)(passes - 1) * rows_bytes;
    Params kp{};
    kp.in = d_in;
    kp.prof = d_prof;
    kp.peak = d_peak;
    kp.at = d_at;
    kp.part_best = reinterpret_cast<float*>(parts);
    kp.part_at = reinterpret_cast<int32_t*>(parts + ((size_t)p->pairs * p->nwidths << (p->L - last)) * sizeof(float));
    kp.table = p->d_table;
    kp.in_stride = in_stride;
    kp.prof_stride = prof_stride;
    kp.pair_words = (long)pitch << p->L;
    kp.p0 = p->p0, kp.nper = p->nper, kp.L = p->L;
    kp.pitch = pitch, kp.nwidths = p->nwidths, kp.top = p->top, kp.seg_log2 = p->seg_log2, kp.eval_log2 = p->eval_log2;
    // the groups of pairs that fit the workspace, one after the other
    const long total = (long)ntrials * p->nper;
    for (long pair0 = 0; pair0 < total; pair0 += p->pairs) {
        kp.pair0 = pair0;
        kp.pairs = (int)(total - pair0 < p->pairs ? total - pair0 : p->pairs);
        kp.a = 0;
        for (int pass = 0; pass < passes; ++pass) {
            kp.n = p->split.stages[pass];
            kp.from_series = pass == 0;
            kp.ws_src = reinterpret_cast<const float*>(p->d_ws + (size_t)(pass ? pass - 1 : 0) * rows_bytes);
            kp.ws_dst = reinterpret_cast<float*>(p->d_ws + (size_t)pass * rows_bytes);        // not the last pass's
            const hipError_t err = launch_pass(kp, pass == passes - 1, lds_of(*p, pass), st);
            if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
            kp.a += kp.n;
        }
        if (p->merge) {
            kp.n = last;
            const hipError_t err = launch_merge(kp, st);
            if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
        }
    }
    return 0;
}

double rtlws_ffa_period(int p, int s, int L)
{
    if (p < 1 || L < 1 || L > MAX_L || s < 0 || s >= (1 << L)) return std::numeric_limits<double>::quiet_NaN();
    return (double)p + (double)s / (double)((1 << L) - 1);
}

double rtlws_ffa_snr(double peak, int width, int rows, double sum1, double sum2, long count)
{
    double mean, var;
    if (width < 1 || rows < 1 || !sp::moments(sum1, sum2, count, &mean, &var)) return std::numeric_limits<double>::quiet_NaN();
    const double n = (double)width * (double)rows;
    return (peak - n * mean) / std::sqrt(n * var);
}

}  // extern "C"
