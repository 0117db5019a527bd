// ffa.hip -- the kernels of include/rtlws_ffa.h (librtlws_ffa.so): the pass kernel of the fast folding
// transform, which in the last pass also evaluates the rows, and the merge of partial peaks.
//
// A pass does the stages a + 1 .. a + n.  A workgroup takes one (trial, base period) pair (blockIdx.y), one superblock
// of 2^(a+n) rows from row B0 and one q = 0 .. 2^a - 1: it loads the 2^n rows B0 + i 2^a + q into LDS, a wavefront a row
// at a time, lanes along c, runs the n stages between two copies of the tile with a barrier behind each, and stores the
// rows B0 + q 2^n + u.  A row's two sources and its shift are the same for the whole wavefront, so they are scalar; the
// mod of a column is one compare and subtract; consecutive lanes read consecutive words at every shift, so no access
// has a bank conflict.  The last pass evaluates the rows where they lie: an evaluating wavefront builds the levels
// P_1 .. P_top of its row by circular doubling in rows of its own, reads every width's pieces, highest bit first, at
// places read from the plan's table, which lies in three registers, and takes every lane's best of its columns; the
// lanes' pairs meet (period_stages.h) and then meet the slot of LDS of the row's run, the slots of a segment meet into the output,
// or into the workspace for the merge where a segment is more than the workgroup's rows.  Plain loads and stores only.
#include <hip/hip_runtime.h>

#include "ffa.h"
#include "period_stages.h"
#include "rtlws_internal.h"

namespace rtlws {
namespace ffa {

using period::stages::meet;
using period::stages::meet_lanes;
static_assert(period::LANES == LANES, "meet_lanes meets a wavefront");

// The plan's table, a word a lane in three registers, loaded once: a word at a wavefront-uniform index is one v_readlane,
// where a scalar load from memory inside the loops over rows and widths would be a round trip each
static_assert(TABLE_WORDS > 2 * LANES && TABLE_WORDS <= 3 * LANES, "the table fills three registers");
struct Words {
    int t0, t1, t2;
    __device__ __forceinline__ Words(const int* t, int lane)
        : t0(t[lane]), t1(t[LANES + lane]), t2(2 * LANES + lane < TABLE_WORDS ? t[2 * LANES + lane] : 0) {}
    __device__ __forceinline__ int operator[](int j) const
    {
        return j < LANES       ? __builtin_amdgcn_readlane(t0, j)
               : j < 2 * LANES ? __builtin_amdgcn_readlane(t1, j - LANES)
                               : __builtin_amdgcn_readlane(t2, j - 2 * LANES);
    }
};

// (c + shift) mod p for c < p, shift < p
__device__ __forceinline__ int wrapped(int c, int shift, int p)
{
    const int i = c + shift;
    return i >= p ? i - p : i;
}

template <bool LAST>
__global__ __launch_bounds__(THREADS) void ffa_pass(const Params k)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const int tid = threadIdx.x, lane = tid & (LANES - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pairl = blockIdx.y;
    const long pair = k.pair0 + pairl;
    const int t = (int)(pair / k.nper), i = (int)(pair - (long)t * k.nper), p = k.p0 + i;
    const int n = k.n, a = k.a, rows = 1 << n, pitch = k.pitch;
    const int q = (int)(blockIdx.x & ((1u << a) - 1u)), b0 = (int)(blockIdx.x >> a) << (a + n);

    float* const tile = lds;                                   // where the stages end
    float* const second = lds + rows * pitch;
    float* cur = (n & 1) ? second : tile;
    float* nxt = (n & 1) ? tile : second;

    // 1: the rows B0 + i 2^a + q, row i to row i of the tile
    {
        const float* src = k.from_series ? k.in + (long)t * k.in_stride : k.ws_src + (long)pairl * k.pair_words;
        src += (long)(b0 + q) * p;
        const long apart = (long)p << a;
        for (int r = wave; r < rows; r += WAVES) {
            const float* const s = src + r * apart;
            float* const d = cur + r * pitch;
            for (int c = lane; c < p; c += LANES) d[c] = s[c];
        }
    }
    __syncthreads();

    // 2: the stages.  Local stage jl is global stage a + jl; row r = g + u of a local block of 2^jl rows from g is row
    // s_j = (q << jl) | u of its global block
    for (int jl = 1; jl <= n; ++jl) {
        const int half = 1 << (jl - 1), mask = (1 << jl) - 1;
        for (int r = wave; r < rows; r += WAVES) {
            const int u = r & mask, g = r - u;
            const int sj = (q << jl) | u;
            const int shift = ((sj + 1) >> 1) % p;
            const float* const x = cur + (g + (u >> 1)) * pitch;
            const float* const y = cur + (g + half + (u >> 1)) * pitch;
            float* const d = nxt + r * pitch;
            for (int c = lane; c < p; c += LANES) d[c] = x[c] + y[wrapped(c, shift, p)];
        }
        __syncthreads();
        float* const was = cur;
        cur = nxt;
        nxt = was;
    }
    // cur == tile

    // 3: the rows B0 + q 2^n + u, contiguous: to the workspace at the pair's own pitch p, or the profiles
    {
        const int m = 1 << k.L;
        float* dst;
        long dpitch;
        if (LAST) {
            dst = k.prof ? k.prof + (pair * m + (q << n)) * k.prof_stride : nullptr;
            dpitch = k.prof_stride;
        } else {
            dst = k.ws_dst + (long)pairl * k.pair_words + (long)(b0 + (q << n)) * p;
            dpitch = p;
        }
        if (dst)
            for (int r = wave; r < rows; r += WAVES) {
                const float* const s = tile + r * pitch;
                float* const d = dst + r * dpitch;
                for (int c = lane; c < p; c += LANES) d[c] = s[c];
            }
    }

    if (LAST) {
        // 4: the peaks.  The first 2^eval_log2 wavefronts evaluate, each its own run of rows_per consecutive rows, a row
        // at a time; every wavefront takes every barrier.  A slot holds the pairs of `unit` consecutive rows: a whole
        // segment where a wavefront's rows hold one, else all the rows of the wavefront
        const Words table(k.table, lane);
        const int nw = k.nwidths, top = k.top;
        const int rows_per = rows >> k.eval_log2;
        const int unit_log2 = k.seg_log2 < n - k.eval_log2 ? k.seg_log2 : n - k.eval_log2;
        const bool evaluating = wave < (1 << k.eval_log2);
        float* const lv = second + wave * top * pitch;         // P_1 .. P_top of this wavefront's row
        float* const slot_best = second + second_rows(n, 1 << k.eval_log2, top) * pitch;
        int* const slot_at = reinterpret_cast<int*>(slot_best + (MAX_WIDTHS << n));

        for (int it = 0; it < rows_per; ++it) {
            const int u = wave * rows_per + it;
            const float* const row0 = tile + u * pitch;
            for (int l = 0; l < top; ++l) {
                if (evaluating) {
                    const float* const s = l ? lv + (l - 1) * pitch : row0;
                    float* const d = lv + l * pitch;
                    for (int c = lane; c < p; c += LANES) d[c] = s[c] + s[wrapped(c, 1 << l, p)];
                }
                __syncthreads();
            }
            if (evaluating) {
                // a width at a time, its pieces' places read from the table's registers: every lane's best of its
                // columns, the lanes' best, and lane 0 meets it with what the slot's earlier rows left
                const int at0 = ((q << n) + u) * p;
                const int slot = (u >> unit_log2) * MAX_WIDTHS;
                const bool opens = (u & ((1 << unit_log2) - 1)) == 0;
                for (int w = 0; w < nw; ++w) {
                    const int first = table[FIRST + w], end = table[FIRST + w + 1];
                    const int top_level = table[first] >> 16;   // the highest bit's piece lies at the column itself
                    const float* const from = top_level ? lv + (top_level - 1) * pitch : row0;
                    float best = -__builtin_inff();
                    int at = -1;
                    for (int c = lane; c < p; c += LANES) {
                        float b = from[c];
                        for (int j = first + 1; j < end; ++j) {
                            const int piece = table[j], level = piece >> 16;
                            b = b + (level ? lv + (level - 1) * pitch : row0)[wrapped(c, piece & 0xffff, p)];
                        }
                        const bool take = b > best;           // strict: NaN never wins, the first of equal values stays
                        best = take ? b : best;
                        at = take ? at0 + c : at;
                    }
                    meet_lanes(best, at);
                    if (lane == 0) {
                        if (!opens) meet(best, at, slot_best[slot + w], slot_at[slot + w]);
                        slot_best[slot + w] = best;
                        slot_at[slot + w] = at;
                    }
                }
            }
            __syncthreads();                                  // the level rows are read: they may be written; the slots are written
        }

        // 5: the slots of an output meet: a segment of the workgroup's own, or the workgroup's partial of a longer one
        const int out_log2 = k.seg_log2 < n ? k.seg_log2 : n;
        const int nout = rows >> out_log2, per = 1 << (out_log2 - unit_log2);
        const int nseg = 1 << (k.L - k.seg_log2);
        for (int o = tid; o < nout * nw; o += THREADS) {
            const int oo = o / nw, w = o - oo * nw;
            float b = -__builtin_inff();
            int at_b = -1;
            for (int j = 0; j < per; ++j) meet(b, at_b, slot_best[(oo * per + j) * MAX_WIDTHS + w], slot_at[(oo * per + j) * MAX_WIDTHS + w]);
            if (k.seg_log2 <= n) {
                const long idx = (pair * nseg + (q << (n - k.seg_log2)) + oo) * nw + w;
                k.peak[idx] = b;
                k.at[idx] = at_b;
            } else {
                const long idx = ((long)pairl * (1 << a) + q) * nw + w;
                k.part_best[idx] = b;
                k.part_at[idx] = at_b;
            }
        }
    }
}

// The partial pairs of the last pass's workgroups, 2^(seg_log2 - n) of them a segment, into the outputs: a thread per
// (pair, segment, width)
__global__ __launch_bounds__(256) void ffa_merge(const Params k)
{
    const int nw = k.nwidths, nseg = 1 << (k.L - k.seg_log2), per = 1 << (k.seg_log2 - k.n), groups = 1 << (k.L - k.n);
    const long o = (long)blockIdx.x * 256 + threadIdx.x;
    if (o >= (long)k.pairs * nseg * nw) return;
    const int w = (int)(o % nw), g = (int)(o / nw % nseg), pairl = (int)(o / nw / nseg);
    float b = -__builtin_inff();
    int at_b = -1;
    for (int j = 0; j < per; ++j) {
        const long idx = ((long)pairl * groups + g * per + j) * nw + w;
        meet(b, at_b, k.part_best[idx], k.part_at[idx]);
    }
    const long idx = ((k.pair0 + pairl) * nseg + g) * nw + w;
    k.peak[idx] = b;
    k.at[idx] = at_b;
}

hipError_t launch_pass(const Params& p, bool last, size_t lds_bytes, hipStream_t st)
{
    const dim3 grid(1u << (p.L - p.n), (unsigned)p.pairs);
    return launch(last ? &ffa_pass<true> : &ffa_pass<false>, grid, dim3(THREADS), lds_bytes, st, p);
}

hipError_t launch_merge(const Params& p, hipStream_t st)
{
    const long outputs = ((long)p.pairs << (p.L - p.seg_log2)) * p.nwidths;
    return launch(&ffa_merge, dim3((unsigned)((outputs + 255) / 256)), dim3(256), 0, st, p);
}

// load_kernel (rtlws_internal.h) for the three kernels; the limit of the pass kernels' dynamic LDS is raised once, to the
// most any plan takes
hipError_t prepare(int device)
{
    hipError_t err = load_kernel(&ffa_pass<false>);
    if (err == hipSuccess) err = load_kernel(&ffa_pass<true>);
    if (err == hipSuccess) err = load_kernel(&ffa_merge);
    if (err == hipSuccess) err = lds_opt_in(&ffa_pass<false>, device, LDS_CAP);
    if (err == hipSuccess) err = lds_opt_in(&ffa_pass<true>, device, LDS_CAP);
    return err;
}

}  // namespace ffa
}  // namespace rtlws
