// pfbsk.h -- shared between pfbsk.hip (the kernels) and pfbsk_shim.hip (rtlws_pfbsk.h's host glue).
#ifndef RTLWS_CSRC_PFBSK_H
#define RTLWS_CSRC_PFBSK_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pfb_bank.h"

namespace rtlws {
namespace pfbsk {

constexpr int OUT_SUM = 0, OUT_DB = 1, OUT_PAYLOAD = 2;   // RTLWS_OUT_POWER_SUM, RTLWS_OUT_MEAN_DB, RTLWS_OUT_PAYLOAD_U8
constexpr int MAX_NSUB = 65535;

// A sub-integration is laid on the tile as the spectrometer lays a spectrum (pfb_bank.h: slice_frames,
// spectra_per_block), a function of (log2 M, K) alone; a workgroup owns one output row of nsub sub-integrations and
// walks them in order.  The tile (pfb::lds_bytes) is reused for both sets of partial sums and, after the last
// sub-integration, for the finished row: no LDS beyond it
constexpr int lds_bytes(int k) { return pfb::lds_bytes(k); }
constexpr int ROWS_PER_BLOCK = 1;

struct SkParams {
    pfb::PfbParams bank;      // src, taps, tw, nframes = nspectra * nsub * k_avg, taps_per_branch, half_hop; first = 0, out unused
    void* clean;              // f32 or u8 rows
    uint32_t* kept;           // or null
    float *s1, *s2;           // both or neither
    long nspectra, clean_stride, kept_stride, sub_stride;
    int k_avg, nsub;
    int output;               // OUT_*
    int shift;                // 0, or M / 2: value i of a row is channel (i + shift) mod M
    float scale;              // OUT_DB, OUT_PAYLOAD: lin = scale / (K N) per channel
    float power_scale, ratio_lo, ratio_hi;
};

// nspectra workgroups; nspectra > 0, k = pfb::MIN_LOG2_M .. pfb::MAX_LOG2_M
hipError_t launch_pfbsk(int k, const SkParams& p, hipStream_t st);
hipError_t prepare_pfbsk(int k);

}  // namespace pfbsk
}  // namespace rtlws
#endif
