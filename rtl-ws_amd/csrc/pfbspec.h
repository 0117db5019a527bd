// pfbspec.h -- shared between pfbspec.hip (the kernels) and pfbspec_shim.hip (rtlws_pfbspec.h's host glue).
#ifndef RTLWS_CSRC_PFBSPEC_H
#define RTLWS_CSRC_PFBSPEC_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pfb_bank.h"

namespace rtlws {
namespace pfbspec {

constexpr int OUT_SUM = 0, OUT_DB = 1, OUT_PAYLOAD = 2;   // RTLWS_OUT_POWER_SUM, RTLWS_OUT_MEAN_DB, RTLWS_OUT_PAYLOAD_U8

// The geometry of a launch is pfb_bank.h's (slice_frames, spectra_per_block), a function of (log2 M, K) alone.
// the tile (pfb::lds_bytes) is reused for the partial sums and the finished rows: no LDS beyond it
constexpr int lds_bytes(int k) { return pfb::lds_bytes(k); }

struct SpecParams {
    pfb::PfbParams bank;      // src, taps, tw, nframes = nspectra * k_avg, taps_per_branch, half_hop; first = 0, out unused
    void* out;                // f32 or u8 rows
    long nspectra, out_stride;
    int k_avg;
    int output;               // OUT_*
    int shift;                // 0, or M / 2: value i of a row is channel (i + shift) mod M
    float lin;                // scale / K, formed on the host (OUT_DB, OUT_PAYLOAD)
};

// ceil(nspectra / spectra_per_block) workgroups; nspectra > 0, k = pfb::MIN_LOG2_M .. pfb::MAX_LOG2_M
hipError_t launch_pfbspec(int k, const SpecParams& p, hipStream_t st);
hipError_t prepare_pfbspec(int k);

}  // namespace pfbspec
}  // namespace rtlws
#endif
