// ddcfir.h -- shared between ddcfir_bank.hip (the kernels) and ddcfir_shim.hip (rtlws_ddcfir.h's host glue): the
// geometry of the filtered down-converter bank and its kernel parameters; its integer pieces are
// ddc_ops.h's.
#ifndef RTLWS_DDCFIR_BANK_H
#define RTLWS_DDCFIR_BANK_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddc_bank.h"

namespace rtlws {
namespace ddcfir {

using ddc::MAX_CH;
using ddc::MAX_R;
using ddc::P;
using ddc::ROWS;
using ddc::THREADS;
using ddc::TILE_DEC;
constexpr int MAX_TAPS = 256;             // RTLWS_DDCFIR_MAX_TAPS
constexpr int MAX_TAP = 32639;            // RTLWS_DDCFIR_MAX_TAP: 256 * 127 + 127, the largest |G| whose high byte is an int8
constexpr int MAX_SHIFT = 30;             // RTLWS_DDCFIR_MAX_SHIFT

// A workgroup owns TILE_DEC consecutive decimated samples of every channel, as the unfiltered bank's does: four
// wavefronts, each ROW_TILES / 4 row tiles of 16 decimated samples, taken PAIR at a time against one read of the
// filter's operands.  A column tile is 8 channels, a K step 16 taps (32 bytes of a window).
constexpr int ROW_TILES = TILE_DEC / ROWS;
constexpr int PAIR = 2;
constexpr int OPERAND_BYTES = 64 * 16;    // of one (column tile, K step): 16 bytes per lane
constexpr int col_tiles(int nch) { return (nch + 7) >> 3; }
constexpr int k_steps(int ntaps) { return (ntaps + 15) >> 4; }
constexpr int lds_bytes(int ntaps, int nch) { return col_tiles(nch) * k_steps(ntaps) * OPERAND_BYTES; }   // <= 64 KiB
// 8-byte operand loads: every window starts 8-byte aligned and ends on a whole load
constexpr bool aligned_loads(int decim, int ntaps) { return decim % 4 == 0 && ntaps % 4 == 0; }

struct FirParams {
    const void* src;          // cmplx_u8, (dec_len - 1) * decim + ntaps samples
    void* out;                // cmplx_s32, channel c at out + c * out_stride
    const uint32_t* table;    // T on the device: cos in the low half of a word, sin in the high half
    const int16_t* taps;      // h on the device, ntaps int16
    long dec_len, first, out_stride;
    int decim, ntaps, nch, shift;
    int16_t words[MAX_CH];    // the tuning words travel by value
};

// the shift s of ddc_ops.h's rotation and store: the caller's
__device__ __forceinline__ int shift_of(const FirParams& p) { return p.shift; }

// ceil(dec_len / TILE_DEC) workgroups of the instantiation of (decim, ntaps); dec_len > 0
hipError_t launch_bank(const FirParams& p, hipStream_t st);
// loads that instantiation on the current device (`device`)
hipError_t prepare_bank(int decim, int ntaps, int device);

}  // namespace ddcfir
}  // namespace rtlws
#endif
