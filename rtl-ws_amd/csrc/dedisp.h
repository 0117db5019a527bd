// dedisp.h -- shared between dedisp.hip (the kernels) and dedisp_shim.hip (rtlws_dedisp.h's host glue): the tile, the
// forms a plan can take and the tables it uploads.  The subband dedisperser's first stage is this tile
// too (subdedisp.h); the rule that chooses a form is dedisp_form.h's.
#ifndef RTLWS_CSRC_DEDISP_H
#define RTLWS_CSRC_DEDISP_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtlws {
namespace dedisp {

constexpr int MIN_NCHAN = 4, MAX_NCHAN = 4096, MAX_TRIALS = 4096, MAX_DELAY = 65535;

// A workgroup owns TILE_OUT consecutive outputs n (one per thread) of `trials` consecutive trials (a trial group) and
// walks the row in chunks of `chunk` positions.  For a chunk it stages a window of the rows in LDS position-major:
// position il of the chunk is the column tile[il * stride + r], r counting rows from the base of the position's unit,
// and behind the chunk's columns lie TILE_OUT zeros, which a position that the mask leaves out reads instead.
// A unit is what shares a base: four neighbouring positions (one 16-byte load of a row), or in the `lone` form one
// position.  The column is as long as TILE_OUT plus the largest spread of delays inside a unit and a trial group.
constexpr int THREADS = 256;
constexpr int TILE_OUT = 256;
constexpr int MAX_TRIALS_PER_BLOCK = 8;
constexpr int MAX_CHUNK = 32;                                  // positions: 128 bytes of a row
constexpr int SMALL_WORDS = 9 * 1024, BIG_WORDS = 16 * 1024;   // f32 of LDS: 36 KiB (four workgroups a CU), 64 KiB (two)

struct Layout {
    int trials;        // per workgroup: 8, 4, 2, 1
    int lone;          // 1: a unit is one position (trials == 1, chunk == MAX_CHUNK), every row is read four times
    int big;           // 1: BIG_WORDS of LDS, 0: SMALL_WORDS
    int chunk;         // positions per chunk: 32, 16, 8, 4
    int stride;        // f32 between the columns of a chunk: > TILE_OUT - 1 + the largest spread, chunk * stride + TILE_OUT <= the LDS
};
constexpr int lds_bytes(const Layout& l) { return (l.big ? BIG_WORDS : SMALL_WORDS) * 4; }

// The smallest stride >= height whose transposing stores fall on 32 different banks: a half-wavefront stores `quads`
// neighbouring quads of 32 / quads consecutive rows, quad q's four values at columns 4 q .. 4 q + 3, so the columns'
// distance 4 stride must step through the banks in strides of 32 / quads: stride = (8 / quads) * odd.  One quad (and
// the lone form, 32 positions of one row: stride odd) takes consecutive rows of one column
constexpr int fit_stride(int height, int quads)
{
    const int unit = quads > 1 ? 8 / quads : 1;
    int s = (height + unit - 1) / unit;
    if (quads > 1 && s % 2 == 0) ++s;
    return s * unit;
}

struct Params {
    const float* rows;
    float* out;
    const int2* units;     // [group][unit] {base, span}: the unit's window is rows n0 + base .. n0 + base + TILE_OUT - 1 + span; base < 0: nothing kept
    const int* rel;        // [group][position][trial of the group]: the word of the tile that output n0 of the trial reads, (position in
                           // its chunk) * stride + delay - base of the position's unit; chunk * stride (the zeros) where the mask leaves it out
    long in_stride, nout, out_stride, rows_needed;
    int nchan, ntrials, ngroups;
    int chunk, stride;
};

// ceil(nout / TILE_OUT) * ngroups workgroups; nout > 0
hipError_t launch_dedisp(const Layout& l, const Params& p, hipStream_t st);
hipError_t prepare_dedisp(const Layout& l);

}  // namespace dedisp
}  // namespace rtlws
#endif
