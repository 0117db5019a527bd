// pfb_bank.h -- shared between pfb_bank.hip (the kernels) and pfb_shim.hip (rtlws_pfb.h's host glue), and the geometry
// of the whole polyphase family (pfbspec, pfbxc, pfbbf): the tile, and how K-frame sums are laid over it.
#ifndef RTLWS_PFB_BANK_H
#define RTLWS_PFB_BANK_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtlws {
namespace pfb {

constexpr int MIN_LOG2_M = 4, MAX_LOG2_M = 10;   // M = 16 .. 1024 channels
constexpr int MAX_TAPS = 32;                     // taps per branch
constexpr int LAYOUT_CHANNEL = 0, LAYOUT_TIME = 1;   // RTLWS_PFB_CHANNEL_MAJOR, RTLWS_PFB_TIME_MAJOR

// A workgroup owns a tile of TILE_POINTS / M consecutive frames: 256 threads, 16 points each in
// every phase.  The tile lives in LDS as complex f32, one row per frame; a row has one place of padding after every
// 16 points (point i at place i + i / 16), so that lanes which take points 16, 64 or M / 16 apart, or read at those
// strides, fall on different banks.
constexpr int THREADS = 256;
constexpr int TILE_POINTS = 4096;
constexpr int tile_frames(int k) { return TILE_POINTS >> k; }
constexpr int row_pad(int k) { return (1 << k) / 16; }
constexpr int row_stride(int k) { return (1 << k) + row_pad(k); }
constexpr int lds_bytes(int k) { return tile_frames(k) * row_stride(k) * 8; }

// The geometry of a launch that sums K = k_avg frames per spectrum (the spectrometer, the correlator, the beamformer's
// power mode), a function of (log2 M, K) alone.  With F = tile_frames(k), a workgroup owns
//   K >= F: one spectrum, ceil(K / F) tile iterations (the last one ragged);
//   K <  F: floor(F / K) spectra in one tile.
// A spectrum's K frames r = 0 .. K - 1 are summed in slices of SLICE = min(16, F) consecutive frames; slice s of a
// tile iteration holds the frames it * F + s * SLICE + (0 .. SLICE - 1).  The order of the sums is pfbspec.hip's.
constexpr int MAX_K_AVG = 65536;
constexpr int slice_frames(int k) { return tile_frames(k) < 16 ? tile_frames(k) : 16; }
constexpr int spectra_per_block(int k, int k_avg) { return k_avg >= tile_frames(k) ? 1 : tile_frames(k) / k_avg; }

struct PfbParams {
    const void* src;          // cmplx_u8, (nframes - 1) * hop + taps * M samples
    float2* out;              // complex f32
    const int16_t* taps;      // the prototype on the device, taps * M int16
    const float2* tw;         // exp(-2 pi i j / M), j = 0 .. M - 1, on the device
    long nframes, first, out_stride;
    int taps_per_branch;
    int half_hop;             // 1: hop M / 2, 0: hop M
    int layout;
};

// ceil(nframes / tile_frames(k)) workgroups; nframes > 0, k = MIN_LOG2_M .. MAX_LOG2_M
hipError_t launch_pfb(int k, const PfbParams& p, hipStream_t st);
hipError_t prepare_pfb(int k);

}  // namespace pfb
}  // namespace rtlws
#endif
