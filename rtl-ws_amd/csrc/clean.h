// clean.h -- shared between clean.hip (the kernels) and clean_shim.hip (rtlws_clean.h's host glue): the limits, what the
// three launches of a run look like, the workspace between them and the kernels' arguments.
#ifndef RTLWS_CSRC_CLEAN_H
#define RTLWS_CSRC_CLEAN_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtlws {
namespace clean {

constexpr int LANES = 64;
constexpr int MIN_NCHAN = 4, MAX_NCHAN = 4096, MIN_BLOCK = 32, MAX_BLOCK = 16384;
constexpr long MAX_NROWS = 1L << 24;
constexpr long MAX_CELLS = 1L << 22;                            // (block, channel) pairs a plan's workspace holds
constexpr int FLAG_ZERODM = 1;

constexpr int pow2_at_least(int n) { int p = 1; while (p < n) p <<= 1; return p; }

// ---- the workspace: 16 bytes a (block, channel) cell, then one int32 a block ----
// Stage 1 leaves (mu, sd) as two f64 in a cell, sd = -1.0 where the channel is not valid; stage 2, which owns the cells of
// its block, reads them all and then writes (m, r) as two f32 over mu and keep as an int32 over the low half of sd
struct Cell {
    double mu, sd;
};
struct Flagged {
    float m, r;
    int32_t keep, unused;
};
static_assert(sizeof(Cell) == 16 && sizeof(Flagged) == 16, "a cell is 16 bytes in both of its forms");
constexpr long max_blocks(int nchan, int block_rows)           // the blocks a plan serves in one run
{
    const long by_rows = (MAX_NROWS + block_rows - 1) / block_rows, by_cells = MAX_CELLS / nchan;
    return by_rows < by_cells ? by_rows : by_cells;
}
constexpr long workspace_bytes(int nchan, long nblocks) { return nblocks * ((long)nchan * (long)sizeof(Cell) + 4); }
static_assert(workspace_bytes(MAX_NCHAN, max_blocks(MAX_NCHAN, MIN_BLOCK)) == (64L << 20) + 4096, "the largest workspace");

// ---- stage 1: the statistics ----
// A workgroup of RES wavefronts owns GROUP consecutive channels of one block: a lane four neighbouring channels, a
// wavefront the rows k == its number (mod RES) of the window; the RES partial pairs meet in LDS [RES][2][GROUP] f64
constexpr int RES = 8, GROUP = 4 * LANES, UNROLL = 8;       // UNROLL rows' loads of a wavefront are in flight together
constexpr int chan_groups(int nchan) { return (nchan + GROUP - 1) / GROUP; }
constexpr int STATS_THREADS = RES * LANES, STATS_LDS = RES * 2 * GROUP * 8;
static_assert(STATS_LDS == 32768, "256 channels x 8 residues x 2 f64");

struct StatsParams {
    const float* rows;
    Cell* cells;               // [nblocks][nchan]
    long in_stride, nrows;
    int nchan, block_rows, groups;
};

// ---- stage 2: the flags ----
// One workgroup a block: a bitonic sort of two lists of sort_len(nchan) f64 keys in LDS side by side, twice
constexpr int sort_len(int nchan) { return pow2_at_least(nchan); }
constexpr int flag_threads(int nchan) { return sort_len(nchan) / 2 < LANES ? LANES : sort_len(nchan) / 2 > 1024 ? 1024 : sort_len(nchan) / 2; }
constexpr int FLAG_SCRATCH = 128;                               // bytes behind the keys: the medians, the counts of 16 wavefronts
constexpr int flag_lds(int nchan) { return 2 * sort_len(nchan) * 8 + FLAG_SCRATCH; }
static_assert(flag_lds(MAX_NCHAN) == 65664, "128 bytes above 64 KiB at 4096 channels: the kernel's limit is raised at open");
constexpr int FLAG_PER_THREAD = 4;                              // channels a thread holds at most: 4096 / 1024
static_assert(sort_len(MAX_NCHAN) == FLAG_PER_THREAD * flag_threads(MAX_NCHAN), "every channel has a register");

struct FlagParams {
    Cell* cells;               // in: stage 1's; out: Flagged
    int32_t* ws_nkept;         // [nblocks]
    const uint8_t* mask;       // [nchan] on the device
    uint8_t* keep;             // the caller's, or NULL
    float* stats;
    int32_t* nkept;
    double t_mean, t_sigma;
    int nchan;
};

// ---- stage 3: the rows ----
// A row takes row_threads(nchan) = the power of two >= nchan / 4 lanes, a lane four neighbouring channels.  Up to 64
// lanes several rows lie side by side in a wavefront; from 128 lanes on a row takes row_waves wavefronts, whose 64 partial
// sums each meet in LDS.  A workgroup has at least 4 wavefronts, stays inside one block and walks APPLY_ITERS times the
// rows it holds at once
constexpr int row_threads(int nchan) { return pow2_at_least(nchan / 4); }
constexpr int row_waves(int nchan) { return row_threads(nchan) <= LANES ? 1 : row_threads(nchan) / LANES; }
constexpr int apply_waves(int nchan) { return row_waves(nchan) < 4 ? 4 : row_waves(nchan); }
constexpr int apply_threads(int nchan) { return apply_waves(nchan) * LANES; }
constexpr int rows_at_once(int nchan) { return apply_threads(nchan) / row_threads(nchan); }
constexpr int APPLY_ITERS = 16;
constexpr int rows_per_group(int nchan) { return rows_at_once(nchan) * APPLY_ITERS; }
constexpr int apply_groups(int nchan, int block_rows) { return (block_rows + rows_per_group(nchan) - 1) / rows_per_group(nchan); }
// two buffers of one f32 a thread where a row takes more than one wavefront
constexpr int apply_lds(int nchan) { return row_waves(nchan) > 1 ? 2 * apply_threads(nchan) * 4 : 0; }
static_assert(apply_threads(MAX_NCHAN) == 1024 && rows_at_once(MAX_NCHAN) == 1 && rows_at_once(4) == 256, "the ends of the row shapes");

struct ApplyParams {
    const float* rows;
    float* out;
    const Flagged* cells;
    const int32_t* ws_nkept;
    long in_stride, out_stride, nrows;
    int nchan, block_rows, groups;      // groups = apply_groups(nchan, block_rows)
    int row_log2;                       // row_threads(nchan) = 1 << row_log2
    int zerodm;
};

// the three launches of a run over nblocks blocks; nblocks > 0
hipError_t launch_stats(const StatsParams& p, long nblocks, hipStream_t st);
hipError_t launch_flags(const FlagParams& p, long nblocks, hipStream_t st);
hipError_t launch_apply(const ApplyParams& p, long nblocks, hipStream_t st);
// loads the kernels a plan of nchan channels launches on `device`, the current one, and raises stage 2's LDS limit where it
// needs more than 64 KiB, so that a run makes no call but its launches
hipError_t prepare(int nchan, int device);

}  // namespace clean
}  // namespace rtlws
#endif
