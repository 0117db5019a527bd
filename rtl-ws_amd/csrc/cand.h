// cand.h -- shared between cand.hip (the kernels) and cand_shim.hip (rtlws_cand.h's host glue): the limits, what the cube's
// fold and the two stages of the refinement launch, and the kernels' arguments.  The block shape a bin
// count takes is the epoch folding's (fold.h): its rule, its LDS figure, its lanes.
#ifndef RTLWS_CSRC_CAND_H
#define RTLWS_CSRC_CAND_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fold.h"

namespace rtlws {
namespace cand {

using fold::LANES;
using fold::lds_bytes;                                          // of a fold workgroup: waves_per_block * nbins * 256
using fold::waves_per_block;                                    // 4 up to 64 bins, 2 up to 128, 1 up to 256

constexpr int MAX_CANDS = 64, MIN_NCHAN = 4, MAX_NCHAN = 4096, MAX_DELAY = 65535;
constexpr int MIN_BINS = fold::MIN_BINS, MAX_BINS = fold::MAX_BINS;
constexpr long MIN_SUB = 16, MAX_SUB = fold::MAX_SUB, MAX_NSAMP = fold::MAX_NSAMP;
constexpr int MAX_NSUB = 1024, MAX_NDM = 256, MAX_NTR = 4096;
constexpr long MAX_WORKSPACE = 1L << 30;                        // bytes of T a search plan may own

// ---- the cube ----
// One workgroup per (candidate, sub-integration, group of 64 waves_per_block channels): a lane a channel, the histogram
// [bin][lane] f32 of fold.h.  UNROLL samples' loads are issued together, a batch ahead of their additions
constexpr int UNROLL = 16;
static_assert(UNROLL % fold::GROUP == 0, "the unrolled samples are whole groups of fold_kernel.h's add_group");
constexpr int chan_groups(int nchan, int nbins) { return (nchan + LANES * waves_per_block(nbins) - 1) / (LANES * waves_per_block(nbins)); }

struct FoldParams {
    const float* rows;         // the waterfall
    float* cube;
    uint32_t* hits;            // NULL: no hits
    const uint64_t* steps;     // [ncand]
    const uint64_t* phases;    // [ncand]
    const int32_t* delays;     // [ncand][nchan]; -1: the mask drops the channel
    long in_stride, nsamp, sub, nsub;
    int nchan, nbins, groups;  // groups = chan_groups(nchan, nbins)
};

// ncand * nsub * groups workgroups; nsamp > 0
hipError_t launch_fold(const FoldParams& p, int ncand, hipStream_t st);
hipError_t prepare_fold(int nbins);

// ---- the refinement: one kernel text for both stages ----
// out[c][..][b] = sum over k ascending of in[c][o][k][(b + shift[c][t][k]) mod nbins].  A wavefront a trial t, WAVES trials a
// workgroup, one workgroup per (c, o, group of WAVES trials); CHUNK rows of nbins values are staged into LDS at a time
// and read by every wavefront at its own rotation.  Stage 1: o = s, k = i, t = q, out = T[c][q][s]; stage 2: o = q,
// k = s, t = r, out = P[c][q][r] and its two f64 sums
constexpr int WAVES = 8, CHUNK = 32;
constexpr int trial_groups(int ntrials) { return (ntrials + WAVES - 1) / WAVES; }
constexpr int stage_lds_bytes(int nbins, bool sums) { return (CHUNK + (sums ? WAVES : 0)) * nbins * 4; }
static_assert(stage_lds_bytes(MAX_BINS, true) == 40960, "a stage's LDS at 256 bins");

struct StageParams {
    const float* in;           // [ncand][no][nk][nbins]
    const int32_t* shifts;     // [ncand][nt][nk], 0 .. nbins - 1
    float* out;                // stage 1: [ncand][nt][no][nbins], never NULL; stage 2: [ncand][no][nt][nbins] or NULL
    float* copy;               // stage 1: a second place for the same rows, or NULL
    double* stat;              // stage 2: [ncand][no][nt]
    double* total;
    int no, nk, nt, nbins;
};

// ncand * no * trial_groups(nt) workgroups of WAVES wavefronts
hipError_t launch_stage(bool sums, const StageParams& p, int ncand, hipStream_t st);
hipError_t prepare_stages(int nbins);

}  // namespace cand
}  // namespace rtlws
#endif
