// sift.h -- shared between sift.hip (the kernels) and sift_shim.hip (rtlws_sift.h's host glue): the tile of the plane,
// the workspace's layout, the word a candidate is marked with and the launches' parameters.  The limits
// of the width table and of seg are pulse.h's: the sift reads what that library wrote.
#ifndef RTLWS_CSRC_SIFT_H
#define RTLWS_CSRC_SIFT_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pulse.h"

namespace rtlws {
namespace sift {

constexpr int MAX_WIDTHS = pulse::MAX_WIDTHS, MAX_WIDTH = pulse::MAX_WIDTH, MAX_TRIALS = pulse::MAX_TRIALS;
constexpr long MIN_SEG = pulse::MIN_SEG, MAX_SEG = pulse::MAX_SEG, MAX_NOUT = pulse::MAX_NOUT;
constexpr int MAX_RT = 32, MAX_RS = 8, MAX_CAND = 1 << 24, CAND_WORDS = 8;

// The plane of events is [t][s], s consecutive.  The scoring launch takes one event a thread in that order.  The box and
// the list launches cut it into tiles of TILE_T x TILE_S events, tile (sb, tb) being workgroup sb * ntb + tb: the tiles
// of one block of segments are consecutive, so the tiles that precede a block of segments in the list's order are a
// prefix.  Thread i of a tile owns segment i % 64 and the ROWS_PER_THREAD trials from (i / 64) * ROWS_PER_THREAD on.
constexpr int THREADS = 256, TILE_T = 64, TILE_S = 64, ROW_GROUPS = THREADS / TILE_S, ROWS_PER_THREAD = TILE_T / ROW_GROUPS;
constexpr int LDS_ROWS = TILE_T + 2 * MAX_RT, LDS_STRIDE = TILE_S + 2 * MAX_RS;          // the tile with the widest halo
constexpr int SCAN_BLOCK = THREADS;                           // tile totals the list launch adds up in one step

// The workspace, in this order, every part from a multiple of 16 bytes:
//   score  f32 [T * S]      stage 1's scores
//   kword  int32 [T * S]    stage 1's k; the box launch ORs a candidate's mark and figures in (below)
//   cc     int32 [ntiles][TILE_S]   candidates of a tile in each of its segments
//   tot    int2 [ntiles]    {candidates, events at or above threshold} of a tile
constexpr int K_MASK = 15, CAND_BIT = 16, MEMBERS_SHIFT = 5, MEMBERS_MASK = 0x7FF, LO_SHIFT = 16, HI_SHIFT = 22, SPAN_MASK = 63;
static_assert((2 * MAX_RT + 1) * (2 * MAX_RS + 1) <= MEMBERS_MASK && MAX_RT <= SPAN_MASK && MAX_WIDTHS <= K_MASK + 1, "a candidate's figures must fit its word");

inline long round16(long bytes) { return (bytes + 15) & ~15L; }
inline long plane_bytes(long events) { return round16(events * 4); }
inline long work_bytes(long events, long ntiles) { return 2 * plane_bytes(events) + round16(ntiles * TILE_S * 4) + round16(ntiles * 8); }

struct Params {
    const float* peak;
    const int32_t* at;
    const double* mom;
    const double* widths;  // the plan's: (double) w_k, k = 0 .. K - 1
    float* score;          // the workspace's four parts
    int32_t* kword;
    int32_t* cc;
    int2* tot;
    uint32_t* cand;
    int32_t* count;
    float* d_score;        // NULL: not written
    int32_t* d_k;          // NULL: not written
    long nout, seg;
    int T, K, S, rt, rs, ntb, nsb, max_cand;
    float threshold;
};

// the static LDS of the box launch and of the list launch; the scoring launch has none
struct BoxLds {
    float tile[LDS_ROWS * LDS_STRIDE];     // row r, column c: event (t0 - rt + r, s0 - rs + c); NaN outside the plane
    int cnt[ROW_GROUPS][TILE_S];
    int part[2][THREADS / 64];
};
struct ListLds {
    int n[3][ROW_GROUPS][TILE_S];          // a thread's counts before, in all and in its own tile, by row group and segment
    int off[TILE_S];
    int part[3][THREADS / 64];
};

// ceil(T * S / THREADS) workgroups, then nsb * ntb twice
hipError_t launch_sift(const Params& p, hipStream_t st);
hipError_t prepare_sift();

}  // namespace sift
}  // namespace rtlws
#endif
