// ffa.h -- shared between ffa.hip (the kernels) and ffa_shim.hip (rtlws_ffa.h's host glue): the limits, how the stages
// split into passes, the LDS of a pass, the table the plan uploads and the kernels' arguments.
#ifndef RTLWS_CSRC_FFA_H
#define RTLWS_CSRC_FFA_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rtlws {
namespace ffa {

constexpr int MIN_P = 16, MAX_P = 1024, MAX_L = 12, MAX_WIDTHS = 16, MAX_WIDTH = 256, MAX_TRIALS = 65536, MAX_PASSES = 3;
constexpr long MAX_CELLS = 1L << 22;
constexpr size_t WORKSPACE_CAP = (size_t)1 << 30;
constexpr int MAX_PAIRS = 65535;                               // a launch's second grid axis

// A workgroup is WAVES wavefronts; a wavefront owns a row of the tile at a time and its lanes run along c.  LDS holds
// rows of `pitch` = p0 + nper - 1 f32: consecutive lanes read consecutive words at every shift, so no pitch conflicts.
constexpr int LANES = 64, WAVES = 8, THREADS = LANES * WAVES;
constexpr int MAX_STAGES = 7;                                  // of one pass: 128 rows
constexpr int LDS_CAP = 160 * 1024;
constexpr int SLOT_BYTES = MAX_WIDTHS * 8;                     // a (best, at) pair per width

// A pass that is not the last: two copies of the tile of 2^n rows.  The last pass: the tile (where its stages end),
// a second region of max(2^n, eval_waves * top) rows (the other copy of the tile, then `top` level rows P_1 .. P_top of
// each evaluating wavefront), and behind them 2^n slots of a pair per width
constexpr int stage_lds_bytes(int n, int pitch) { return (2 << n) * pitch * 4; }
constexpr int second_rows(int n, int waves, int top) { return (1 << n) > waves * top ? (1 << n) : waves * top; }
constexpr int last_lds_bytes(int n, int pitch, int waves, int top) { return ((1 << n) + second_rows(n, waves, top)) * pitch * 4 + (SLOT_BYTES << n); }

// the most stages of a pass at this pitch: what the last pass needs with one evaluating wavefront never exceeds it
constexpr int max_stages(int pitch)
{
    int n = 0;
    while (n < MAX_STAGES && stage_lds_bytes(n + 1, pitch) + (SLOT_BYTES << (n + 1)) <= LDS_CAP) ++n;
    return n;
}
static_assert(max_stages(MAX_P) == 4 && max_stages(MIN_P) == MAX_STAGES, "the tiles at the two ends of the pitch");
static_assert(MAX_PASSES * max_stages(MAX_P) >= MAX_L, "three passes serve every L at every pitch");
static_assert(last_lds_bytes(2, MAX_P, 1, 8) <= LDS_CAP && last_lds_bytes(4, MAX_P, 1, 8) <= LDS_CAP, "the last pass with one evaluating wavefront");

// as few passes as max_stages allows, the stages dealt as evenly as they go, the larger shares first
struct Split {
    int passes;
    int stages[MAX_PASSES];
};
constexpr Split split_of(int L, int pitch)
{
    Split s{(L + max_stages(pitch) - 1) / max_stages(pitch), {0, 0, 0}};
    int left = L;
    for (int k = 0; k < s.passes; ++k) {
        s.stages[k] = (left + s.passes - k - 1) / (s.passes - k);
        left -= s.stages[k];
    }
    return s;
}

// the wavefronts of the last pass that evaluate a row each at a time: the largest power of two up to WAVES and 2^n whose
// level rows fit
constexpr int eval_waves_log2(int n, int pitch, int top)
{
    int e = n < 3 ? n : 3;
    while (e > 0 && last_lds_bytes(n, pitch, 1 << e, top) > LDS_CAP) --e;
    return e;
}
static_assert((1 << 3) == WAVES, "eval_waves_log2's ceiling");

// The plan's table on the device, int32 words:
//   [FIRST + k]       where width k's pieces begin in the table, k = 0 .. nwidths (the last one: where they end)
//   [from PIECES on]  a piece: (its level << 16) | (its offset, the sum of the width's higher bits); highest bit first
constexpr int FIRST = 0, PIECES = 32, MAX_PIECES = 8, TABLE_WORDS = PIECES + MAX_WIDTHS * MAX_PIECES;

struct Params {
    const float* in;           // the series (the first pass)
    const float* ws_src;       // the rows of the pass before (the other passes), pair_words apart
    float* ws_dst;             // the rows of this pass (not the last)
    float* prof;               // the last pass; NULL: no profiles
    float* peak;
    int32_t* at;
    float* part_best;          // the last pass with a merge behind it: a pair per (pair in flight, workgroup, width)
    int32_t* part_at;
    const int* table;
    long in_stride, prof_stride, pair_words;                    // pair_words = m * pitch
    long pair0;                // the first (trial, base period) pair of this group: pair = t * nper + i
    int p0, nper, L, a, n;     // this pass: stages a + 1 .. a + n
    int pitch, nwidths, top, seg_log2, eval_log2;
    int from_series;
    int pairs;                 // of this group: the grid's second axis
};

// pass: m >> n by p.pairs workgroups.  merge: the partial pairs of p.pairs pairs into d_peak and d_at
hipError_t launch_pass(const Params& p, bool last, size_t lds_bytes, hipStream_t st);
hipError_t launch_merge(const Params& p, hipStream_t st);
// the kernels loaded on the current device, and the limit of their dynamic LDS raised to LDS_CAP
hipError_t prepare(int device);

}  // namespace ffa
}  // namespace rtlws
#endif
