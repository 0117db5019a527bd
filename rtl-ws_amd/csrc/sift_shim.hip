// sift_shim.hip -- extern "C" glue of include/rtlws_sift.h (librtlws_sift.so): argument rules, the plane's tiles and the
// workspace's parts (sift.h), the plan, the three launches.  The engine (device, stream) is librtlws_hip.so's; nothing
// here reads the environment, and nothing of a run is computed on the host: without a device there is no plan.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <vector>

#include "rtlws_sift.h"
#include "search_plan.h"
#include "sift.h"

// The widths as the scoring reads them, on the engine's device
struct rtlws_sift_plan : rtlws::search::Plan {
    int nwidths, rt, rs;
    long seg;
    double* d_widths;
};

namespace {

using namespace rtlws::sift;
namespace sp = rtlws::search;

static_assert(MAX_WIDTHS == RTLWS_SIFT_MAX_WIDTHS && MAX_WIDTH == RTLWS_SIFT_MAX_WIDTH && MIN_SEG == RTLWS_SIFT_MIN_SEG && MAX_SEG == RTLWS_SIFT_MAX_SEG &&
                  MAX_TRIALS == RTLWS_SIFT_MAX_TRIALS && MAX_NOUT == RTLWS_SIFT_MAX_NOUT && MAX_RT == RTLWS_SIFT_MAX_RT && MAX_RS == RTLWS_SIFT_MAX_RS &&
                  MAX_CAND == RTLWS_SIFT_MAX_CAND && CAND_WORDS == RTLWS_SIFT_CAND_WORDS && MAX_WIDTHS == sp::MAX_WIDTHS && MAX_TRIALS == sp::MAX_TRIALS,
              "rtlws_sift.h, sift.h, pulse.h and search_plan.h disagree");

// ---- the rules, each worded once ----
const char* why_not_plan(int nwidths, const int32_t* widths, long seg, int rt, int rs)
{
    if (const char* why = sp::why_not_widths(nwidths, widths, MAX_WIDTH, "every width must be 1 .. 1024")) return why;
    if (seg < MIN_SEG || seg > MAX_SEG || seg % 4) return "seg must be 64 .. 1048576 and a multiple of 4";
    if (rt < 0 || rt > MAX_RT) return "rt must be 0 .. 32";
    if (rs < 0 || rs > MAX_RS) return "rs must be 0 .. 8";
    return nullptr;
}

const char* why_not_nout(long nout) { return nout < 1 || nout > MAX_NOUT ? "nout must be 1 .. 2^30 (0: there is no event to sift)" : nullptr; }

// the plane of ntrials x ceil(nout / seg) events: one run counts them in an int32, and its tiles are one grid
const char* why_not_plane(int ntrials, long nout, long seg)
{
    const long nseg = sp::ceil_div(nout, seg);
    if (nseg > INT_MAX / ntrials) return "more than 2^31 - 1 events";
    return sp::why_not_grid(sp::ceil_div(nseg, TILE_S), sp::ceil_div(ntrials, TILE_T));
}

long tiles_of(int ntrials, long nseg) { return sp::ceil_div(nseg, TILE_S) * sp::ceil_div(ntrials, TILE_T); }

}  // namespace

extern "C" {

const char* rtlws_sift_last_error(void) { return g_err.c_str(); }

int rtlws_sift_supported(int nwidths, const int32_t* widths, long seg, int rt, int rs)
{
    return supported("rtlws_sift", why_not_plan(nwidths, widths, seg, rt, rs));
}

int rtlws_sift_geometry(int nwidths, const int32_t* widths, long seg, int rt, int rs, int ntrials, long nout, int* blocks, int* threads,
                        int* lds_bytes, int* tile_t, int* tile_s, long* nseg)
{
    const char* fn = "rtlws_sift_geometry";
    g_err.clear();
    if (const char* why = why_not_plan(nwidths, widths, seg, rt, rs)) return fail(fn, why, -1);
    if (const char* why = sp::why_not_ntrials(ntrials)) return fail(fn, why, -1);
    if (const char* why = why_not_nout(nout)) return fail(fn, why, -1);
    if (const char* why = why_not_plane(ntrials, nout, seg)) return fail(fn, why, -1);
    const long S = sp::ceil_div(nout, seg);
    if (blocks) blocks[0] = (int)sp::ceil_div(ntrials * S, THREADS), blocks[1] = blocks[2] = (int)tiles_of(ntrials, S);
    if (threads) threads[0] = threads[1] = threads[2] = THREADS;
    if (lds_bytes) lds_bytes[0] = 0, lds_bytes[1] = (int)sizeof(BoxLds), lds_bytes[2] = (int)sizeof(ListLds);
    if (tile_t) *tile_t = TILE_T;
    if (tile_s) *tile_s = TILE_S;
    if (nseg) *nseg = S;
    return 0;
}

rtlws_sift_plan* rtlws_sift_open(rtlws_engine* e, int nwidths, const int32_t* widths, long seg, int rt, int rs)
{
    const auto fill = [&](rtlws_sift_plan& p) {
        p.nwidths = nwidths, p.seg = seg, p.rt = rt, p.rs = rs;
        const std::vector<double> table(widths, widths + nwidths);
        const hipError_t err = sp::upload(&p.d_widths, table.data(), table.size());
        return err == hipSuccess ? prepare_sift() : err;
    };
    return sp::open_plan<rtlws_sift_plan>("rtlws_sift_open", why_not_plan(nwidths, widths, seg, rt, rs), e, fill, "the table or the kernels", rtlws_sift_close);
}

void rtlws_sift_close(rtlws_sift_plan* p) { sp::close_plan(p, &rtlws_sift_plan::d_widths); }

long rtlws_sift_work_bytes(const rtlws_sift_plan* p, int ntrials, long nout)
{
    const char* fn = "rtlws_sift_work_bytes";
    g_err.clear();
    if (const char* why = sp::why_not_ntrials(ntrials)) return fail(fn, why, -1);
    if (const char* why = why_not_nout(nout)) return fail(fn, why, -1);
    if (!p) return fail(fn, NULL_PLAN, -1);
    if (const char* why = why_not_plane(ntrials, nout, p->seg)) return fail(fn, why, -1);
    const long S = sp::ceil_div(nout, p->seg);
    return work_bytes(ntrials * S, tiles_of(ntrials, S));
}

int rtlws_sift_run(rtlws_sift_plan* p, const float* d_peak, const int32_t* d_at, const double* d_mom, int ntrials, long nout, float threshold,
                   int max_cand, void* d_work, uint32_t* d_cand, int32_t* d_count, float* d_score, int32_t* d_k, void* stream)
{
    const char* fn = "rtlws_sift_run";
    g_err.clear();
    // what needs no plan
    if (const char* why = sp::why_not_ntrials(ntrials)) return fail(fn, why, -1);
    if (const char* why = why_not_nout(nout)) return fail(fn, why, -1);
    if (threshold != threshold) return fail(fn, "threshold must not be NaN", -1);
    if (max_cand < 1 || max_cand > MAX_CAND) return fail(fn, "max_cand must be 1 .. 16777216", -1);
    if (!d_peak || !d_at || !d_mom || !d_work || !d_cand || !d_count) return fail(fn, "null pointer", -1);
    if (sp::misaligned(d_peak, 4)) return fail(fn, "d_peak must be 4-byte aligned", -1);
    if (sp::misaligned(d_at, 4)) return fail(fn, "d_at must be 4-byte aligned", -1);
    if (sp::misaligned(d_mom, 8)) return fail(fn, "d_mom must be 8-byte aligned", -1);
    if (sp::misaligned(d_work, 16)) return fail(fn, "d_work must be 16-byte aligned", -1);
    if (sp::misaligned(d_cand, 16)) return fail(fn, "d_cand must be 16-byte aligned", -1);
    if (sp::misaligned(d_count, 4)) return fail(fn, "d_count must be 4-byte aligned", -1);
    if (sp::misaligned(d_score, 4)) return fail(fn, "d_score must be 4-byte aligned", -1);
    if (sp::misaligned(d_k, 4)) return fail(fn, "d_k must be 4-byte aligned", -1);
    if (!p) return fail(fn, NULL_PLAN, -1);
    // what the plan decides; still before anything is asked of the device
    if (const char* why = why_not_plane(ntrials, nout, p->seg)) return fail(fn, why, -1);

    if (sp::use_device(fn, p)) return -3;
    const long S = sp::ceil_div(nout, p->seg), events = ntrials * S, ntiles = tiles_of(ntrials, S);
    char* const work = static_cast<char*>(d_work);
    Params k;
    k.peak = d_peak;
    k.at = d_at;
    k.mom = d_mom;
    k.widths = p->d_widths;
    k.score = reinterpret_cast<float*>(work);
    k.kword = reinterpret_cast<int32_t*>(work + plane_bytes(events));
    k.cc = reinterpret_cast<int32_t*>(work + 2 * plane_bytes(events));
    k.tot = reinterpret_cast<int2*>(work + 2 * plane_bytes(events) + round16(ntiles * TILE_S * 4));
    k.cand = d_cand;
    k.count = d_count;
    k.d_score = d_score;
    k.d_k = d_k;
    k.nout = nout;
    k.seg = p->seg;
    k.T = ntrials;
    k.K = p->nwidths;
    k.S = (int)S;
    k.rt = p->rt;
    k.rs = p->rs;
    k.ntb = (int)sp::ceil_div(ntrials, TILE_T);
    k.nsb = (int)sp::ceil_div(S, TILE_S);
    k.max_cand = max_cand;
    k.threshold = threshold;
    const hipError_t err = launch_sift(k, stream_of(p->engine, stream));
    if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
    return 0;
}

}  // extern "C"
