// ddc_bank.h -- shared between ddc_bank.hip (the kernels) and ddc_shim.hip (rtlws_ddc.h's host glue).
#ifndef RTLWS_DDC_BANK_H
#define RTLWS_DDC_BANK_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtlws {
namespace ddc {

constexpr int LOG2_P = 16;                // phase period P = 2^16 (RTLWS_DDC_LOG2_PERIOD)
constexpr int P = 1 << LOG2_P;
constexpr int MAX_CH = 32;                // RTLWS_DDC_MAX_CHANNELS
constexpr int MAX_R = 128;

// A workgroup owns TILE_DEC consecutive decimated samples of every channel: four wavefronts,
// each ROW_TILES / 4 row tiles of 16 decimated samples (the N dimension of v_mfma_i32_16x16x32_i8), taken
// GROUP at a time.  A column tile is 8 channels (16 rows of the M dimension: re and im of each), a K step 16
// input samples (32 bytes).
constexpr int THREADS = 256;
constexpr int ROWS = 16;
constexpr int GROUP = 8;
constexpr int TILE_DEC = 1024;
constexpr int ROW_TILES = TILE_DEC / ROWS;
constexpr int COL_TILES = MAX_CH / 8;     // 4
constexpr int K_STEPS = MAX_R / 16;       // 8: the generic kernel's phasor operands, 16 bytes per lane and (tile, step)
constexpr int LDS_BYTES_ANY = COL_TILES * K_STEPS * 64 * 16;
// the kernels' template argument: the factors with an instantiation of their own (one K step, the phasor operands in
// registers), 0 for the kernel of any factor (the operands in LDS).  Also fm_bank.hip's
constexpr int rt_of(int cic_r) { return cic_r == 8 || cic_r == 10 || cic_r == 12 ? cic_r : 0; }

struct BankParams {
    const void* src;          // cmplx_u8, dec_len * cic_r samples
    void* out;                // cmplx_s32, channel c at out + c * out_stride
    const uint32_t* table;    // T on the device: cos in the low half of a word, sin in the high half
    long dec_len, first, out_stride;
    int cic_r, nch;
    int16_t words[MAX_CH];    // the tuning words travel by value
};

// ceil(dec_len / TILE_DEC) workgroups; dec_len > 0
hipError_t launch_bank(const BankParams& p, hipStream_t st);
hipError_t prepare_bank();

}  // namespace ddc
}  // namespace rtlws
#endif
