// pulse.h -- shared between pulse.hip (the kernel) and pulse_shim.hip (rtlws_pulse.h's host glue): the tile, the rows
// of LDS a table takes and the table the plan uploads.
#ifndef RTLWS_CSRC_PULSE_H
#define RTLWS_CSRC_PULSE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtlws {
namespace pulse {

constexpr int MAX_WIDTHS = 16, MAX_WIDTH = 1024, MAX_TRIALS = 65536;
constexpr long MIN_SEG = 64, MAX_SEG = 1048576, MAX_NOUT = 1L << 30;
constexpr int MAX_LEVELS = 11;                                 // P_0 .. P_10: 2^10 = MAX_WIDTH
constexpr int MAX_PIECES = 10;                                 // the most bits a width has (1023)

// A workgroup owns one segment of one trial and walks it in tiles of tile_out outputs, thread i the outputs i, i + 256,
// .. of the tile.  For a tile of cnt outputs (tile_out but for the segment's last) LDS holds rows of `row` f32: level l
// of the tile, P_l[n0 .. n0 + cnt + w_max - 2^l - 1], in the row level_row[l] names.  A level that some width's binary
// form uses keeps a row of its own for the tile; the levels in between take the (at most two) rows behind those in
// turn.  Behind the last tile the rows' words are the scratch of the reductions.
constexpr int THREADS = 256;
constexpr int MAX_TILE = 1024, MIN_TILE = 256;
constexpr int LDS_WORDS[3] = {4 * 1024, 8 * 1024, 16 * 1024};  // f32 of LDS: 16, 32, 64 KiB
constexpr int SCRATCH_WORDS = 4 * THREADS + 2 * MAX_WIDTHS * (THREADS / 64);      // two f64 per thread, a pair per width and wavefront

struct Layout {
    int tile_out;      // 1024, 512, 256: the largest whose rows fit in 64 KiB
    int row;           // f32 per row: roundup4(tile_out + w_max - 1)
    int rows;          // levels_kept + min(2, levels below the top that no width uses)
    int levels_kept;   // distinct bits set over the table
    int top;           // floor(log2 w_max): the levels are 0 .. top
    int w_max;
    int lds;           // index into LDS_WORDS: the smallest that holds rows * row words
};

// The plan's table on the device, int32 words:
//   [LEVEL_ROW + l]   the word of LDS where level l's row begins, l = 0 .. top
//   [FIRST + k]       where width k's pieces begin in the table, k = 0 .. nwidths (the last one: where they end)
//   [from PIECES on]  a piece: (its level's row) + (its offset, the sum of the width's higher bits); highest bit first
constexpr int LEVEL_ROW = 0, FIRST = 16, PIECES = 48, TABLE_WORDS = PIECES + MAX_WIDTHS * MAX_PIECES;

struct Params {
    const float* in;
    float* peak;
    int32_t* at;
    double* mom;       // NULL: no moments
    const int* table;
    long in_stride, nout, seg, nseg, need;                      // need = nout + w_max - 1: no sample at or beyond it is read
    int nwidths, top, w_max;
};

// ntrials * nseg workgroups; nout > 0
hipError_t launch_pulse(const Layout& l, const Params& p, int ntrials, hipStream_t st);
hipError_t prepare_pulse(const Layout& l);

}  // namespace pulse
}  // namespace rtlws
#endif
