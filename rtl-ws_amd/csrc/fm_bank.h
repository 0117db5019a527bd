// fm_bank.h -- shared between fm_bank.hip (the kernels) and fmbank_shim.hip (rtlws_fmbank.h's host glue).
#ifndef RTLWS_FM_BANK_H
#define RTLWS_FM_BANK_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddc_bank.h"

namespace rtlws {
namespace fmbank {

constexpr int MAX_CH = ddc::MAX_CH;       // RTLWS_FMBANK_MAX_CHANNELS
constexpr int STATE = 21;                 // RTLWS_FM_STATE_FLOATS
constexpr int COL_CH = 8;                 // channels of a column tile: the M dimension of the DDC's contraction

// A workgroup owns TILE consecutive audio samples of one column tile of eight channels.  TILE is
// half of fm_chain.h's: eight channels of its capacities would be 151 KiB of the CU's 160 KiB and one workgroup per
// CU; at 256 a CU holds two, for a halo of about 35 decimated samples per 1024.  The
// capacities per channel are derived as fm_chain.h's, for the worst block shape block_len = 23 (half = 11,
// quarter = 5: 23 decimated samples for 5 audio samples instead of 20):
//   stage-2 stream   n2 <= 2 TILE + 9                                  = 521
//   work span        <= (n2 - 1) + one skipped output per 10 of them   <= 520 + 52 = 572
//   stage-1 stream   n1 <= 2 * 572 + 11                                = 1155
//   phases           <= n1 + one skipped sample per 20 of them + 1     <= 1155 + 58 + 1 = 1214
// The two halves (even and odd stream index) of a stream lie H floats apart with H = 16 mod 32, as in fm_chain.h.
// PHASE_CAP = 8 mod 32: the four row groups of an accumulator (channel pairs 2 PHASE_CAP floats apart) store their
// phases to banks 16 apart.
constexpr int TILE = 256;
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int PHASE_CAP = 1224;
constexpr int S1_HALF = 592;              // >= ceil(1155 / 2) = 578
constexpr int S1_CAP = 2 * S1_HALF;
constexpr int S2_HALF = 272;              // >= ceil(521 / 2) = 261; the stage-2 stream lies over the phases
constexpr int CH_FLOATS = PHASE_CAP + S1_CAP;
constexpr int LDS_FLOATS = COL_CH * CH_FLOATS;
constexpr int LDS_BYTES = LDS_FLOATS * 4;
// the generic kernel's phasor operands (one column tile, 16 bytes per lane and K step) lie over the stage-1 streams
constexpr int K_STEPS = ddc::K_STEPS;
static_assert(K_STEPS * 64 * 4 <= COL_CH * S1_CAP, "the operands fit under the stage-1 streams");
static_assert(S2_HALF + 261 <= PHASE_CAP && PHASE_CAP % 32 == 8 && S1_HALF % 32 == 16 && S2_HALF % 32 == 16, "layout");

struct BankParams {
    const void* src;          // cmplx_u8, nblocks * block_len * cic_r samples
    const uint32_t* table;    // T on the device, as ddc::BankParams's
    const float* state_in;    // [nch][STATE]
    float* state_out;
    float* audio;             // channel c at audio + c * audio_stride
    long audio_stride, first, nblocks, ntiles;
    int block_len, cic_r, nch;
    int16_t words[MAX_CH];    // the tuning words travel by value
};

// (ntiles + 1) * ceil(nch / 8) workgroups: per column tile the audio tiles, then the one that writes state_out
hipError_t launch_bank(const BankParams& p, hipStream_t st);
// nfloats = nch * STATE
hipError_t launch_state_copy(const float* state_in, float* state_out, int nfloats, hipStream_t st);
hipError_t prepare_bank();

}  // namespace fmbank
}  // namespace rtlws
#endif
