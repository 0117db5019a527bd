// cutout.h -- shared between cutout.hip (the kernels) and cutout_shim.hip (rtlws_cutout.h's host glue): the limits,
// the tile of the band-time launch, the plan's tables as the kernels read them and the launches' parameters (DESIGN.md
// 4.31).  The limits of the waterfall and of its table are the dedispersion's (dedisp.h), those of the widths the pulse
// search's (pulse.h), the candidate's words the sift's (sift.h): the cutouts read what those libraries wrote.
#ifndef RTLWS_CSRC_CUTOUT_H
#define RTLWS_CSRC_CUTOUT_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dedisp.h"
#include "pulse.h"
#include "sift.h"

namespace rtlws {
namespace cutout {

constexpr int MIN_NCHAN = dedisp::MIN_NCHAN, MAX_NCHAN = dedisp::MAX_NCHAN, MAX_TRIALS = dedisp::MAX_TRIALS, MAX_DELAY = dedisp::MAX_DELAY;
constexpr int MAX_WIDTHS = pulse::MAX_WIDTHS, MAX_WIDTH = pulse::MAX_WIDTH, CAND_WORDS = sift::CAND_WORDS;
constexpr int MAX_BIN = 1024, MIN_NX = 4, MAX_NX = 256, MAX_NF = MAX_NCHAN, MAX_RQ = 64, MAX_DQ = 64, MAX_CAND = 4096, INFO_WORDS = 4;
constexpr long MAX_NSAMP = 1L << 30;
static_assert(MAX_DELAY <= 0xFFFF, "the plan keeps a delay in 16 bits");

// The band-time launch: workgroup ((i * xgroups + xg) * fgroups + fg) owns candidate i, the time bins xg * TILE_X .. of
// it and the subbands fg * per .., per = subbands_per_group(cpb); thread c of it owns channel fg * per * cpb + c of the
// chunk.  R lies in LDS as tile[x * TILE_STRIDE + c]: a row's stores fall on consecutive banks, and the 32 bins that
// the lanes of a half-wavefront read at one channel on 32 different ones (TILE_STRIDE is odd).
constexpr int THREADS = 256, TILE_X = 32, TILE_C = THREADS, TILE_STRIDE = TILE_C + 1;
constexpr int DEPTH = 8;                                       // rows of a lane in flight
constexpr int subbands_per_group(int cpb) { return cpb <= TILE_C ? TILE_C / cpb : 1; }

struct BandLds {
    float tile[TILE_X * TILE_STRIDE];
};

// the DM-time launch: workgroup i * ndm + r, thread x; nx threads rounded up to whole wavefronts
constexpr int dmt_threads(int nx) { return (nx + 63) / 64 * 64; }

struct Params {
    const float* rows;             // NULL with a NULL ft
    const float* series;           // NULL with a NULL dmt
    const uint32_t* cand;
    const int32_t* count;
    const uint16_t* delays;        // the plan's: [ntrials][nchan]
    const uint8_t* keep;           // the plan's: [nchan], 1 or 0
    const int2* shape;             // the plan's: {w_k, bin_k}, k = 0 .. K - 1
    float* ft;
    float* dmt;
    int32_t* info;
    long in_stride, series_stride;
    int nsamp, nchan, ntrials, K, nx, nf, cpb, per, xgroups, fgroups, rq, dq, ndm, max_cand;
    int info_from_dmt;             // 1: there is no band-time launch, the DM-time launch writes d_info
};

// max_cand * xgroups * fgroups workgroups where p.ft, max_cand * ndm where p.dmt
hipError_t launch_cutout(const Params& p, hipStream_t st);
hipError_t prepare_cutout();

}  // namespace cutout
}  // namespace rtlws
#endif
