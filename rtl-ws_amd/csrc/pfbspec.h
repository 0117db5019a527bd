// pfbspec.h -- shared between pfbspec.hip (the kernels) and pfbspec_shim.hip (rtlws_pfbspec.h's host glue).
#ifndef RTLWS_CSRC_PFBSPEC_H
#define RTLWS_CSRC_PFBSPEC_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pfb_bank.h"

namespace rtlws {
namespace pfbspec {

constexpr int MAX_K_AVG = 65536;
constexpr int OUT_SUM = 0, OUT_DB = 1, OUT_PAYLOAD = 2;   // RTLWS_OUT_POWER_SUM, RTLWS_OUT_MEAN_DB, RTLWS_OUT_PAYLOAD_U8

// The geometry of a launch, a function of (log2 M, K) alone.  With F = pfb::tile_frames(k) frames
// in the filter bank's tile, a workgroup owns
//   K >= F: one spectrum, ceil(K / F) tile iterations (the last one ragged);
//   K <  F: floor(F / K) spectra in one tile.
// A spectrum's K frames r = 0 .. K - 1 are summed in slices of SLICE = min(16, F) consecutive frames; slice s of a
// tile iteration holds the frames it * F + s * SLICE + (0 .. SLICE - 1).
constexpr int slice_frames(int k) { return pfb::tile_frames(k) < 16 ? pfb::tile_frames(k) : 16; }
constexpr int spectra_per_block(int k, int k_avg) { return k_avg >= pfb::tile_frames(k) ? 1 : pfb::tile_frames(k) / k_avg; }
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
