// subdedisp_shim.hip -- extern "C" glue of include/rtlws_subdedisp.h (librtlws_subdedisp.so): argument rules, the
// sweep's tables, the plan (stage 1's form by dedisp_form.h's rule over d1, stage 2's by the rule below over d2), the two
// launches.  The engine (device, stream) is librtlws_hip.so's; nothing here reads the environment, and nothing of a run
// is computed on the host: without a device there is no plan.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "dedisp_form.h"
#include "rtlws_subdedisp.h"
#include "search_plan.h"
#include "subdedisp.h"

// The forms the tables took and their tables on the engine's device
struct rtlws_subdedisp_plan : rtlws::search::Plan {
    int nchan, nsub, nnominal, ntrials, max_d1, max_d2, ngroups2;
    rtlws::dedisp::Layout stage1, stage2;
    int2* d_units1;
    int* d_rel1;
    int4* d_groups;
    int2* d_units2;
    int* d_rel2;
};

namespace {

using namespace rtlws::subdedisp;
namespace dd = rtlws::dedisp;
namespace sp = rtlws::search;

static_assert(MIN_NCHAN == RTLWS_SUBDEDISP_MIN_NCHAN && MAX_NCHAN == RTLWS_SUBDEDISP_MAX_NCHAN && MIN_PER_SUB == RTLWS_SUBDEDISP_MIN_PER_SUB &&
                  MAX_NOMINALS == RTLWS_SUBDEDISP_MAX_NOMINALS && MAX_TRIALS == RTLWS_SUBDEDISP_MAX_TRIALS &&
                  MAX_DELAY == RTLWS_SUBDEDISP_MAX_DELAY && MIN_NCHAN == sp::MIN_NCHAN && MAX_NCHAN == sp::MAX_NCHAN && MAX_TRIALS <= sp::MAX_TRIALS,
              "rtlws_subdedisp.h, subdedisp.h, dedisp.h and search_plan.h disagree");

// ---- the rules, each worded once ----
const char* why_not_nsub(int nchan, int nsub)
{
    return nsub < 1 || nsub > nchan / MIN_PER_SUB || nchan % nsub || nchan / nsub % 4
               ? "nsub must be 1 .. nchan / 4 and divide nchan into subbands of a multiple of 4 positions"
               : nullptr;
}

const char* why_not_ntrials(int ntrials) { return ntrials < 1 || ntrials > MAX_TRIALS ? dd::WHY_NTRIALS : nullptr; }

const char* why_not_shape(int nchan, int nsub, int nnominal, int ntrials)
{
    if (const char* why = sp::why_not_nchan(nchan)) return why;
    if (const char* why = why_not_nsub(nchan, nsub)) return why;
    if (nnominal < 1 || nnominal > MAX_NOMINALS) return "nnominal must be 1 .. 4096";
    if (const char* why = why_not_ntrials(ntrials)) return why;
    if (nnominal > ntrials) return "nnominal must be <= ntrials";
    return nullptr;
}

// subband s keeps a position
bool kept(int per, const uint8_t* mask, int s)
{
    if (!mask) return true;
    for (int i = s * per; i < (s + 1) * per; ++i)
        if (mask[i]) return true;
    return false;
}

// the shape, then first, then the tables' entries; *max_d1: the largest over the positions the mask keeps, *max_d2: over
// the subbands that keep one
const char* why_not_tables(int nchan, int nsub, int nnominal, int ntrials, const int32_t* first, const int32_t* d1, const int32_t* d2,
                           const uint8_t* mask, int* max_d1, int* max_d2)
{
    if (const char* why = why_not_shape(nchan, nsub, nnominal, ntrials)) return why;
    if (!first) return "null first";
    for (int a = 0; a < nnominal; ++a)
        if (first[a] >= first[a + 1]) return "first must ascend strictly from 0 to ntrials";
    if (first[0] != 0 || first[nnominal] != ntrials) return "first must ascend strictly from 0 to ntrials";
    if (!d1 || !d2) return dd::WHY_NULL_DELAYS;
    int most1 = 0, most2 = 0;
    for (long a = 0; a < nnominal; ++a)
        for (int i = 0; i < nchan; ++i) {
            const int32_t d = d1[a * nchan + i];
            if (d < 0 || d > MAX_DELAY) return dd::WHY_DELAY;
            if ((!mask || mask[i]) && d > most1) most1 = d;
        }
    for (int s = 0; s < nsub; ++s) {
        const bool keeps = kept(nchan / nsub, mask, s);
        for (long t = 0; t < ntrials; ++t) {
            const int32_t d = d2[t * nsub + s];
            if (d < 0 || d > MAX_DELAY) return dd::WHY_DELAY;
            if (keeps && d > most2) most2 = d;
        }
    }
    *max_d1 = most1;
    *max_d2 = most2;
    return nullptr;
}

const char* why_not_nout(long nout) { return nout < 0 ? "nout must be >= 0" : nullptr; }

long mid_stride_of(long nmid) { return sp::ceil_div(nmid, 4) * 4; }

// ---- the form of stage 2 ----
// the groups of `trials` consecutive trials, none across a border of first: {first trial, trials, nominal, 0}
std::vector<int4> groups_of_trials(int nnominal, const int32_t* first, int trials)
{
    std::vector<int4> groups;
    for (int a = 0; a < nnominal; ++a)
        for (int t0 = first[a]; t0 < first[a + 1]; t0 += trials) groups.push_back(make_int4(t0, first[a + 1] - t0 < trials ? first[a + 1] - t0 : trials, a, 0));
    return groups;
}

// the least and the largest d2 of subband s under a group's trials
void group_range(int nsub, const int32_t* d2, const int4& g, int s, int* lo, int* hi)
{
    int least = INT_MAX, most = -1;
    for (int t = g.x; t < g.x + g.y; ++t) {
        const int d = d2[(long)t * nsub + s];
        least = d < least ? d : least;
        most = d > most ? d : most;
    }
    *lo = least;
    *hi = most;
}

// The largest group of 8, 4, 2, 1 trials (no larger than the largest nominal fills half of) whose windows of
// MAX_CHUNK subbands fit, in the smaller LDS where they do, else the larger; one trial spreads nothing and fits the smaller
dd::Layout choose_stage2(int nchan, int nsub, int nnominal, const int32_t* first, const int32_t* d2, const uint8_t* mask)
{
    int most = 0;
    for (int a = 0; a < nnominal; ++a) most = first[a + 1] - first[a] > most ? first[a + 1] - first[a] : most;
    std::vector<uint8_t> keeps(nsub);
    for (int s = 0; s < nsub; ++s) keeps[s] = kept(nchan / nsub, mask, s);
    for (int trials = MAX_TRIALS_PER_BLOCK; trials > 1; trials /= 2) {
        if (trials >= 2 * most) continue;
        int widest = 0;
        for (const int4& g : groups_of_trials(nnominal, first, trials))
            for (int s = 0; s < nsub; ++s) {
                int lo, hi;
                group_range(nsub, d2, g, s, &lo, &hi);
                if (keeps[s] && hi - lo > widest) widest = hi - lo;
            }
        const long words = (long)MAX_CHUNK * (TILE_OUT + widest) + TILE_OUT;
        if (words <= BIG_WORDS) return dd::Layout{trials, 1, words > SMALL_WORDS, MAX_CHUNK, TILE_OUT + widest};
    }
    return dd::Layout{1, 1, 0, MAX_CHUNK, TILE_OUT};
}
static_assert((long)MAX_CHUNK * TILE_OUT + TILE_OUT <= SMALL_WORDS, "one trial a workgroup must fit the smaller LDS");

// the tables of subdedisp.h's Params2 for a form
void build_stage2(int nchan, int nsub, const int32_t* d2, const uint8_t* mask, const dd::Layout& l, const std::vector<int4>& groups,
                  std::vector<int2>* units, std::vector<int>* rel)
{
    units->assign(groups.size() * nsub, make_int2(-1, 0));
    rel->assign(groups.size() * nsub * l.trials, l.chunk * l.stride);
    for (size_t g = 0; g < groups.size(); ++g)
        for (int s = 0; s < nsub; ++s) {
            if (!kept(nchan / nsub, mask, s)) continue;
            int lo, hi;
            group_range(nsub, d2, groups[g], s, &lo, &hi);
            (*units)[g * nsub + s] = make_int2(lo, hi - lo);
            for (int k = 0; k < l.trials; ++k) {
                const long t = groups[g].x + (k < groups[g].y ? k : groups[g].y - 1);                  // past the group: its last trial again
                (*rel)[(g * nsub + s) * l.trials + k] = s % l.chunk * l.stride + d2[t * nsub + s] - lo;
            }
        }
}

// both grids of a run, stage 1's first
const char* why_not_grids(long nout, int max_d2, int nnominal, const dd::Layout& stage1, long ngroups2)
{
    if (const char* why = sp::why_not_grid(sp::ceil_div(nout + max_d2, TILE_OUT), dd::groups_of(nnominal, stage1.trials))) return why;
    return sp::why_not_grid(sp::ceil_div(nout, TILE_OUT), ngroups2);
}

}  // namespace

extern "C" {

const char* rtlws_subdedisp_last_error(void) { return g_err.c_str(); }

int rtlws_subdedisp_supported(int nchan, int nsub, int nnominal, int ntrials)
{
    return supported("rtlws_subdedisp", why_not_shape(nchan, nsub, nnominal, ntrials));
}

int rtlws_subdedisp_delays(int nchan, int nsub, int shifted, double f_centre_hz, double bandwidth_hz, double row_seconds, int ntrials,
                           double dm0, double dm_step, int per_nominal, int32_t* first, int32_t* d1, int32_t* d2, double* smear_rows)
{
    const char* fn = "rtlws_subdedisp_delays";
    g_err.clear();
    if (const char* why = sp::why_not_nchan(nchan)) return fail(fn, why, -1);
    if (const char* why = why_not_nsub(nchan, nsub)) return fail(fn, why, -1);
    if (const char* why = why_not_ntrials(ntrials)) return fail(fn, why, -1);
    if (shifted != 0 && shifted != 1) return fail(fn, dd::WHY_SHIFTED, -1);
    if (per_nominal < 1) return fail(fn, "per_nominal must be >= 1", -1);
    if (!first || !d1 || !d2) return fail(fn, "null table", -1);
    if (const char* why = sp::why_not_band(nchan, f_centre_hz, bandwidth_hz, row_seconds)) return fail(fn, why, -1);
    const int M = nchan, B = nsub, C = M / B;
    const int A = (int)sp::ceil_div(ntrials, per_nominal);
    const std::vector<double> x = sp::excess(M, shifted, f_centre_hz, bandwidth_hz);
    std::vector<int> ref(B);
    for (int s = 0; s < B; ++s) {
        ref[s] = s * C;
        for (int i = s * C; i < (s + 1) * C; ++i)
            if (x[i] < x[ref[s]]) ref[s] = i;
    }
    char buf[96];
    for (int t = 0; t < ntrials; ++t) {
        const double dm = dm0 + (double)t * dm_step;
        if (!(std::isfinite(dm) && dm >= 0.0)) {
            snprintf(buf, sizeof buf, dd::WHY_DM, t);
            return fail(fn, buf, -1);
        }
    }
    double smear = 0.0;
    for (int a = 0; a < A; ++a) {
        const int t0 = (int)((long)a * per_nominal), t1 = (long)t0 + per_nominal < ntrials ? t0 + per_nominal : ntrials;
        first[a] = t0;
        const double dm_a = ((dm0 + (double)t0 * dm_step) + (dm0 + (double)(t1 - 1) * dm_step)) / 2.0;
        for (int i = 0; i < M; ++i) {
            const double dx = x[i] - x[ref[i / C]];
            const double d = std::rint(sp::DISPERSION * dm_a * dx / row_seconds);
            if (!(d <= (double)MAX_DELAY)) {
                snprintf(buf, sizeof buf, dd::WHY_SWEEP, "nominal", a);
                return fail(fn, buf, -1);
            }
            d1[(long)a * M + i] = (int32_t)d;
            for (int t = t0; t < t1; ++t) {
                const double off = std::fabs((dm0 + (double)t * dm_step) - dm_a) * sp::DISPERSION * dx / row_seconds;
                smear = off > smear ? off : smear;
            }
        }
        for (int t = t0; t < t1; ++t) {
            const double dm = dm0 + (double)t * dm_step;
            for (int s = 0; s < B; ++s) {
                const double d = std::rint(sp::DISPERSION * dm * x[ref[s]] / row_seconds);
                if (!(d <= (double)MAX_DELAY)) {
                    snprintf(buf, sizeof buf, dd::WHY_SWEEP, "trial", t);
                    return fail(fn, buf, -1);
                }
                d2[(long)t * B + s] = (int32_t)d;
            }
        }
    }
    first[A] = ntrials;
    if (smear_rows) *smear_rows = smear;
    return 0;
}

int rtlws_subdedisp_geometry(int nchan, int nsub, int nnominal, int ntrials, const int32_t* first, const int32_t* d1, const int32_t* d2,
                             const uint8_t* mask, long nout, int* blocks, int* threads, int* lds_bytes, int* tile_out, int* nominals_per_block,
                             int* trials_per_block, int* max_d1, int* max_d2)
{
    const char* fn = "rtlws_subdedisp_geometry";
    g_err.clear();
    int most1 = 0, most2 = 0;
    if (const char* why = why_not_tables(nchan, nsub, nnominal, ntrials, first, d1, d2, mask, &most1, &most2)) return fail(fn, why, -1);
    if (const char* why = why_not_nout(nout)) return fail(fn, why, -1);
    const dd::Layout l1 = dd::choose_layout(nchan, nnominal, d1, mask), l2 = choose_stage2(nchan, nsub, nnominal, first, d2, mask);
    const long ngroups2 = (long)groups_of_trials(nnominal, first, l2.trials).size();
    if (const char* why = why_not_grids(nout, most2, nnominal, l1, ngroups2)) return fail(fn, why, -1);
    if (blocks) {
        blocks[0] = nout ? (int)(sp::ceil_div(nout + most2, TILE_OUT) * dd::groups_of(nnominal, l1.trials)) : 0;
        blocks[1] = (int)(sp::ceil_div(nout, TILE_OUT) * ngroups2);
    }
    if (threads) threads[0] = threads[1] = THREADS;
    if (lds_bytes) lds_bytes[0] = dd::lds_bytes(l1), lds_bytes[1] = dd::lds_bytes(l2);
    if (tile_out) *tile_out = TILE_OUT;
    if (nominals_per_block) *nominals_per_block = l1.trials;
    if (trials_per_block) *trials_per_block = l2.trials;
    if (max_d1) *max_d1 = most1;
    if (max_d2) *max_d2 = most2;
    return 0;
}

rtlws_subdedisp_plan* rtlws_subdedisp_open(rtlws_engine* e, int nchan, int nsub, int nnominal, int ntrials, const int32_t* first,
                                           const int32_t* d1, const int32_t* d2, const uint8_t* mask)
{
    int most1 = 0, most2 = 0;
    const char* why = why_not_tables(nchan, nsub, nnominal, ntrials, first, d1, d2, mask, &most1, &most2);
    const auto fill = [&](rtlws_subdedisp_plan& p) {
        p.nchan = nchan, p.nsub = nsub, p.nnominal = nnominal, p.ntrials = ntrials, p.max_d1 = most1, p.max_d2 = most2;
        p.stage1 = dd::choose_layout(nchan, nnominal, d1, mask);
        p.stage2 = choose_stage2(nchan, nsub, nnominal, first, d2, mask);
        std::vector<int2> units1, units2;
        std::vector<int> rel1, rel2;
        dd::build_tables(nchan, nnominal, d1, mask, p.stage1, &units1, &rel1);
        const std::vector<int4> groups = groups_of_trials(nnominal, first, p.stage2.trials);
        build_stage2(nchan, nsub, d2, mask, p.stage2, groups, &units2, &rel2);
        p.ngroups2 = (int)groups.size();
        hipError_t err = sp::upload(&p.d_units1, units1.data(), units1.size());
        if (err == hipSuccess) err = sp::upload(&p.d_rel1, rel1.data(), rel1.size());
        if (err == hipSuccess) err = sp::upload(&p.d_groups, groups.data(), groups.size());
        if (err == hipSuccess) err = sp::upload(&p.d_units2, units2.data(), units2.size());
        if (err == hipSuccess) err = sp::upload(&p.d_rel2, rel2.data(), rel2.size());
        if (err == hipSuccess) err = prepare_stage1(p.stage1);
        return err == hipSuccess ? prepare_stage2(p.stage2) : err;
    };
    return sp::open_plan<rtlws_subdedisp_plan>("rtlws_subdedisp_open", why, e, fill, "the tables or the kernels", rtlws_subdedisp_close);
}

void rtlws_subdedisp_close(rtlws_subdedisp_plan* p)
{
    sp::close_plan(p, &rtlws_subdedisp_plan::d_units1, &rtlws_subdedisp_plan::d_rel1, &rtlws_subdedisp_plan::d_groups, &rtlws_subdedisp_plan::d_units2,
                   &rtlws_subdedisp_plan::d_rel2);
}

long rtlws_subdedisp_rows_needed(const rtlws_subdedisp_plan* p, long nout)
{
    const char* fn = "rtlws_subdedisp_rows_needed";
    g_err.clear();
    if (const char* why = why_not_nout(nout)) return fail(fn, why, -1);
    if (!p) return fail(fn, NULL_PLAN, -1);
    return nout ? nout + p->max_d2 + p->max_d1 : 0;
}

long rtlws_subdedisp_mid_stride(const rtlws_subdedisp_plan* p, long nout)
{
    const char* fn = "rtlws_subdedisp_mid_stride";
    g_err.clear();
    if (const char* why = why_not_nout(nout)) return fail(fn, why, -1);
    if (!p) return fail(fn, NULL_PLAN, -1);
    return nout ? mid_stride_of(nout + p->max_d2) : 0;
}

long rtlws_subdedisp_work_floats(const rtlws_subdedisp_plan* p, long nout)
{
    const char* fn = "rtlws_subdedisp_work_floats";
    g_err.clear();
    if (const char* why = why_not_nout(nout)) return fail(fn, why, -1);
    if (!p) return fail(fn, NULL_PLAN, -1);
    return nout ? (long)p->nnominal * p->nsub * mid_stride_of(nout + p->max_d2) : 0;
}

int rtlws_subdedisp_run(rtlws_subdedisp_plan* p, const float* d_rows, long in_stride, long nout, float* d_work, float* d_out, long out_stride,
                        void* stream)
{
    const char* fn = "rtlws_subdedisp_run";
    g_err.clear();
    // what needs no plan: a row holds at least 4 values
    if (const char* why = why_not_nout(nout)) return fail(fn, why, -1);
    if (const char* why = sp::why_not_row_stride(in_stride, MIN_NCHAN)) return fail(fn, why, -1);
    if (const char* why = sp::why_not_stride(in_stride)) return fail(fn, why, -1);
    if (out_stride < nout) return fail(fn, "out_stride must be >= nout", -1);
    if (nout > 0 && (!d_rows || !d_work || !d_out)) return fail(fn, "null pointer", -1);
    if (sp::misaligned(d_rows, 16)) return fail(fn, "d_rows must be 16-byte aligned", -1);
    if (sp::misaligned(d_work, 4)) return fail(fn, "d_work must be 4-byte aligned", -1);
    if (sp::misaligned(d_out, 4)) return fail(fn, "d_out must be 4-byte aligned", -1);
    if (!p) return fail(fn, NULL_PLAN, -1);
    // what the plan decides; still before anything is asked of the device
    if (const char* why = sp::why_not_row_stride(in_stride, p->nchan)) return fail(fn, why, -1);
    if (const char* why = why_not_grids(nout, p->max_d2, p->nnominal, p->stage1, p->ngroups2)) return fail(fn, why, -1);
    if (nout == 0) return 0;

    if (sp::use_device(fn, p)) return -3;
    const long nmid = nout + p->max_d2, mid_stride = mid_stride_of(nmid);
    const hipStream_t st = stream_of(p->engine, stream);
    dd::Params k1;
    k1.rows = d_rows;
    k1.out = d_work;
    k1.units = p->d_units1;
    k1.rel = p->d_rel1;
    k1.in_stride = in_stride;
    k1.nout = nmid;
    k1.out_stride = mid_stride;
    k1.rows_needed = nmid + p->max_d1;
    k1.nchan = p->nchan;
    k1.ntrials = p->nnominal;
    k1.ngroups = (int)dd::groups_of(p->nnominal, p->stage1.trials);
    k1.chunk = p->stage1.chunk;
    k1.stride = p->stage1.stride;
    hipError_t err = launch_stage1(p->stage1, k1, p->nchan / p->nsub, p->nsub, st);
    if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
    Params2 k2;
    k2.mid = d_work;
    k2.out = d_out;
    k2.groups = p->d_groups;
    k2.units = p->d_units2;
    k2.rel = p->d_rel2;
    k2.mid_stride = mid_stride;
    k2.nmid = nmid;
    k2.nout = nout;
    k2.out_stride = out_stride;
    k2.nsub = p->nsub;
    k2.ngroups = p->ngroups2;
    k2.stride = p->stage2.stride;
    err = launch_stage2(p->stage2, k2, st);
    if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
    return 0;
}

}  // extern "C"
