// dedisp_form.h -- the host rule that turns a table of per-position delays and a mask into the form of dedisp.h's tile
// (Layout) and the tables of that form (units, rel): shared by dedisp_shim.hip, whose table is [trial][position], and
// subdedisp_shim.hip, whose first stage hands it [nominal][position].  Internal linkage, like
// search_plan.h: a library has one shim.
#ifndef RTLWS_CSRC_DEDISP_FORM_H
#define RTLWS_CSRC_DEDISP_FORM_H

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <vector>

#include "dedisp.h"
#include "search_plan.h"

namespace rtlws {
namespace dedisp {
namespace {

namespace sp = rtlws::search;

// ---- what both libraries say of a table and of a sweep, each worded once ----
constexpr const char* WHY_NTRIALS = "ntrials must be 1 .. 4096";
constexpr const char* WHY_SHIFTED = "shifted must be 0 or 1";
constexpr const char* WHY_NULL_DELAYS = "null delays";
constexpr const char* WHY_DELAY = "every delay must be 0 .. 65535";
constexpr const char* WHY_DM = "trial %d: the dispersion measure must be finite and >= 0";      // printf forms: the trial,
constexpr const char* WHY_SWEEP = "%s %d: a delay above 65535 rows";                            // "trial" or "nominal" and which

[[maybe_unused]] long groups_of(int ntrials, int trials) { return sp::ceil_div(ntrials, trials); }

// ---- the form of a table ----
// The least and the largest delay of positions i0 .. i0 + width - 1 under trials t0 .. t0 + trials - 1 (those of them
// there are), over the positions the mask keeps; false where it keeps none
[[maybe_unused]] bool unit_range(int nchan, int ntrials, const int32_t* delays, const uint8_t* mask, int t0, int trials, int i0, int width, int* lo, int* hi)
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
[[maybe_unused]] int widest_spread(int nchan, int ntrials, const int32_t* delays, const uint8_t* mask, int trials, int width)
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
[[maybe_unused]] bool fits(int trials, int chunk, int height, Layout* l)
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
[[maybe_unused]] Layout choose_layout(int nchan, int ntrials, const int32_t* delays, const uint8_t* mask)
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
[[maybe_unused]] void build_tables(int nchan, int ntrials, const int32_t* delays, const uint8_t* mask, const Layout& l, std::vector<int2>* units,
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
}  // namespace dedisp
}  // namespace rtlws
#endif
