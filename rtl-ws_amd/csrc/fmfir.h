// fmfir.h -- shared between fmfir_bank.hip (the kernels) and fmfir_shim.hip (rtlws_fmfir.h's host glue): the
// geometry of the filtered FM bank and its kernel parameters.  The work split, the tile and the LDS
// layout are fm_bank.h's, the filter's limits and K steps ddcfir.h's.
#ifndef RTLWS_FMFIR_BANK_H
#define RTLWS_FMFIR_BANK_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddcfir.h"
#include "fm_bank.h"

namespace rtlws {
namespace fmfir {

using ddcfir::MAX_SHIFT;
using ddcfir::MAX_TAP;
using ddcfir::MAX_TAPS;
using fmbank::COL_CH;
using fmbank::LDS_BYTES;
using fmbank::LDS_FLOATS;
using fmbank::MAX_CH;                     // RTLWS_FMFIR_MAX_CHANNELS
using fmbank::STATE;
using fmbank::THREADS;
using fmbank::TILE;
using fmbank::WAVES;
constexpr int PAIR = ddcfir::PAIR;        // row tiles a wavefront takes against one read of an operand

// The filter's operands of one column tile, ddcfir.h's 1 KiB per K step, lie over the stage-1 streams until stage A's
// barrier, where fm_bank_kernel<0> keeps its phasor operands: the kernel's LDS is fm_bank.h's, two workgroups a CU
constexpr int operand_bytes(int ntaps) { return ddcfir::k_steps(ntaps) * ddcfir::OPERAND_BYTES; }
static_assert(operand_bytes(MAX_TAPS) == 16 * 1024 && operand_bytes(MAX_TAPS) <= COL_CH * fmbank::S1_CAP * 4,
              "the operands fit under the stage-1 streams");
static_assert(2 * LDS_BYTES <= 160 * 1024, "two workgroups per CU");

struct BankParams {
    const void* src;          // cmplx_u8, (nblocks * block_len - 1) * decim + ntaps samples
    const uint32_t* table;    // T on the device, as ddc::BankParams's
    const int16_t* taps;      // h on the device, ntaps int16
    const float* state_in;    // [nch][STATE]
    float* state_out;
    float* audio;             // channel c at audio + c * audio_stride
    long audio_stride, first, nblocks, ntiles;
    int block_len, decim, ntaps, nch, shift;
    int16_t words[MAX_CH];    // the tuning words travel by value
};

// the shift s of the rotation in front of the discriminator (fm_bank_stages.h's emit_phase): the caller's
__device__ __forceinline__ int shift_of(const BankParams& p) { return p.shift; }

// (ntiles + 1) * ceil(nch / 8) workgroups of the instantiation of (decim, ntaps); nblocks > 0
hipError_t launch_bank(const BankParams& p, hipStream_t st);
// nfloats = nch * STATE
hipError_t launch_state_copy(const float* state_in, float* state_out, int nfloats, hipStream_t st);
// loads that instantiation and the state copy on the current device
hipError_t prepare_bank(int decim, int ntaps);

}  // namespace fmfir
}  // namespace rtlws
#endif
