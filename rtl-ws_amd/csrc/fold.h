// fold.h -- shared between fold.hip (the kernel) and fold_shim.hip (rtlws_fold.h's host glue): the limits, the block
// shape a bin count takes and the kernel's arguments.
#ifndef RTLWS_CSRC_FOLD_H
#define RTLWS_CSRC_FOLD_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtlws {
namespace fold {

constexpr int MAX_PERIODS = 4096, MIN_BINS = 2, MAX_BINS = 256, MAX_TRIALS = 65536;
constexpr long MIN_SUB = 64, MAX_SUB = 1L << 24, MAX_NSAMP = 1L << 30;

// A wavefront owns 64 consecutive periods (a lane a period), one trial and one sub-integration; it stages TILE samples
// per step, a lane a sample.  Its histogram is [bin][lane] f32 in LDS: a pitch of exactly LANES dwords, so that a
// lane's column is its own bank whatever its bins are.  A workgroup is the wavefronts of waves_per_block consecutive
// groups of 64 periods of one trial and sub-integration.
constexpr int LANES = 64, TILE = 64;
constexpr int GROUP = 4;                                        // samples whose LDS reads are issued together (fold_kernel.h)
static_assert(TILE % GROUP == 0, "a tile is whole groups");
constexpr int WAVE_LDS_BYTES_PER_BIN = LANES * 4;

// 4 wavefronts up to 64 bins, 2 up to 128, 1 up to 256: never more than 64 KiB of LDS
constexpr int waves_per_block(int nbins) { return nbins <= 64 ? 4 : nbins <= 128 ? 2 : 1; }
constexpr int lds_bytes(int nbins) { return waves_per_block(nbins) * nbins * WAVE_LDS_BYTES_PER_BIN; }
static_assert(lds_bytes(64) == 65536 && lds_bytes(128) == 65536 && lds_bytes(256) == 65536 && lds_bytes(65) < 65536, "a workgroup's LDS");

struct Params {
    const float* in;
    float* prof;
    uint32_t* hits;        // NULL: no hits
    const uint64_t* steps;
    const uint64_t* phases;
    long in_stride, nsamp, sub, nsub;
    int nperiods, nbins, groups;                                // groups = ceil(nperiods / (64 waves_per_block))
};

// ntrials * groups * nsub workgroups; nsamp > 0
hipError_t launch_fold(const Params& p, int ntrials, hipStream_t st);
hipError_t prepare_fold(int nbins);

}  // namespace fold
}  // namespace rtlws
#endif
