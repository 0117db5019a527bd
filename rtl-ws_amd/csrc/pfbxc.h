// pfbxc.h -- shared between pfbxc.hip (the kernels) and pfbxc_shim.hip (rtlws_pfbxc.h's host glue).
#ifndef RTLWS_CSRC_PFBXC_H
#define RTLWS_CSRC_PFBXC_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pfb_bank.h"

namespace rtlws {
namespace pfbxc {

constexpr int MIN_INPUTS = 2, MAX_INPUTS = 4;

// The geometry of a launch is pfb_bank.h's (slice_frames, spectra_per_block), a function of (log2 M, K) alone.  Every
// input has a tile of its own.
constexpr int pairs(int ninputs) { return ninputs * (ninputs - 1) / 2; }
// ninputs tiles (the slices' partial sums reuse them): 69 632, 104 448 or 139 264 bytes of the 160 KiB of a CU
constexpr int lds_bytes(int k, int ninputs) { return ninputs * pfb::lds_bytes(k); }

struct XcParams {
    pfb::PfbParams bank;          // taps, tw, nframes = nspectra * k_avg, taps_per_branch, half_hop; first = 0; src, out unused
    const void* src[MAX_INPUTS];  // the captures, cmplx_u8; those at or behind ninputs are null
    float* autos;                 // row j * A + a: S_a[j]
    float2* cross;                // row j * NX + x: V_ab[j], x the pair's number
    long nspectra, auto_stride, cross_stride;   // strides in elements: floats, complex values
    int k_avg;
    int shift;                    // 0, or M / 2: value i of a row is channel (i + shift) mod M
};

// ceil(nspectra / spectra_per_block) workgroups; nspectra > 0, k = pfb::MIN_LOG2_M .. pfb::MAX_LOG2_M,
// ninputs = MIN_INPUTS .. MAX_INPUTS
hipError_t launch_pfbxc(int k, int ninputs, const XcParams& p, hipStream_t st);
hipError_t prepare_pfbxc(int k, int ninputs);

}  // namespace pfbxc
}  // namespace rtlws
#endif
