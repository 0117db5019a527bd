// pfbbf.h -- shared between pfbbf.hip (the kernels) and pfbbf_shim.hip (rtlws_pfbbf.h's host glue).
#ifndef RTLWS_CSRC_PFBBF_H
#define RTLWS_CSRC_PFBBF_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pfb_bank.h"

namespace rtlws {
namespace pfbbf {

constexpr int MIN_INPUTS = 1, MAX_INPUTS = 8;
constexpr int MIN_BEAMS = 1, MAX_BEAMS = 4;

// Voltage mode has the channelizer's geometry (pfb::tile_frames frames per workgroup), power mode the one of the
// K-frame sums (pfb::slice_frames, pfb::spectra_per_block): both pfb_bank.h's.  One tile serves every number of inputs
// and beams: the beams' running values stay in registers.
constexpr int lds_bytes(int k) { return pfb::lds_bytes(k); }

struct BfParams {
    // taps, tw, taps_per_branch, half_hop; src unused.  Voltage mode: out, nframes, first, out_stride, layout are the
    // channelizer's.  Power mode: nframes = nspectra * k_avg, first = 0
    pfb::PfbParams bank;
    const void* src[MAX_INPUTS];  // the captures, cmplx_u8; those at or behind ninputs are null
    const float2* w;              // W[b][a][c], [nbeams][ninputs][M]
    float* rows;                  // power mode: row j * B + b is S_b[j]
    long beam_stride;             // voltage mode: beam b at out + b * beam_stride complex values
    long nspectra, row_stride;    // power mode; the stride in floats
    int ninputs;
    int k_avg;
    int shift;                    // power mode: 0, or M / 2: value i of a row is channel (i + shift) mod M
};

// voltage mode: ceil(nframes / tile_frames) workgroups, nframes > 0; power mode: ceil(nspectra / spectra_per_block)
// workgroups, nspectra > 0.  k = pfb::MIN_LOG2_M .. pfb::MAX_LOG2_M, nbeams = MIN_BEAMS .. MAX_BEAMS
hipError_t launch_pfbbf(int k, int nbeams, const BfParams& p, hipStream_t st);
hipError_t launch_pfbbf_power(int k, int nbeams, const BfParams& p, hipStream_t st);
hipError_t prepare_pfbbf(int k, int nbeams);

}  // namespace pfbbf
}  // namespace rtlws
#endif
