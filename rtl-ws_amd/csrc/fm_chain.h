// fm_chain.h -- shared between fm_chain.hip (the kernels) and fm_shim.hip (rtlws_fm.h's host glue).
#ifndef RTLWS_FM_CHAIN_H
#define RTLWS_FM_CHAIN_H

#include <hip/hip_runtime.h>

namespace rtlws {
namespace fm {

// A workgroup owns TILE consecutive audio samples.  The capacities are those of the worst block
// shape, block_len = 23 (half = 11, quarter = 5: 23 decimated samples for 5 audio samples instead of 20):
//   stage-2 stream   n2 <= 2 TILE + 9                                  = 1033
//   work span        <= (n2 - 1) + one skipped output per 10 of them   <= 1032 + 104 = 1136
//   stage-1 stream   n1 <= 2 * 1136 + 11                               = 2283
//   phases           <= n1 + one skipped sample per 20 of them + 1     <= 2283 + 115 + 1 = 2399
// The two halves (even and odd stream index) of a stream lie H floats apart with H = 16 mod 32: lanes 2k and 2k+1
// of a wavefront store to banks 16 apart.
constexpr int TILE = 512;
constexpr int THREADS = 256;
constexpr int PHASE_CAP = 2400;
constexpr int S1_HALF = 1168;             // >= ceil(2283 / 2) = 1142
constexpr int S1_CAP = S1_HALF + 1152;
constexpr int S2_HALF = 528;              // >= ceil(1033 / 2) = 517; the stage-2 stream lies over the phases
constexpr int LDS_FLOATS = PHASE_CAP + S1_CAP;

// source of the decimated samples: cmplx_s32, or cmplx_u8 through a CIC block sum of 8 / 10 / 12 / any factor
enum { SRC_CS32 = 0, SRC_CU8_ANY = 1, SRC_CU8_8 = 8, SRC_CU8_10 = 10, SRC_CU8_12 = 12 };

struct ChainParams {
    const void* src;          // cmplx_s32 or cmplx_u8
    void* dec;                // decimated cmplx_s32 out, or nullptr
    const float* state_in;
    float* state_out;
    float* audio;
    long nblocks, ntiles;
    int block_len, cic_r;
};

// ntiles + 1 workgroups: tiles, then the one that writes state_out.  run_stage2 == false: the tiles only store
// p.dec (one workgroup when p.dec is null).
hipError_t launch_chain(const ChainParams& p, bool run_stage2, hipStream_t st);
hipError_t launch_state_copy(const float* state_in, float* state_out, hipStream_t st);
hipError_t prepare_chain();

}  // namespace fm
}  // namespace rtlws
#endif
