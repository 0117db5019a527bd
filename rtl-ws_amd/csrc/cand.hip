// cand.hip -- the kernels of include/rtlws_cand.h (librtlws_cand.so).
//
// The cube.  Lanes run along channels: a wavefront owns 64 consecutive channels, one candidate and one sub-integration
// and walks that sub-integration's samples in ascending n, reading row n + delay of its channel, a lane a channel, so a
// row is read in coalesced runs.  The candidate's phase is the same for all 64 lanes: it lives in scalar registers and
// the bin is one scalar multiply-high.  The histogram is fold_kernel.h's [bin][lane] f32 in LDS (a lane's column its own
// bank, no two lanes on one address, no barrier), and the addition is that file's add_group: the words of four
// consecutive samples are read together, a sample whose bin an earlier one of the group had takes that one's sum from a
// register, and the four sums are written in ascending n -- the additions of one LDS read-add-write per sample in the
// same order, so the same bits, with the LDS latency paid once per four samples.  UNROLL samples' loads are issued
// together, a batch ahead of their additions.  The epilogue is fold_kernel.h's row reads at a pitch of nbins words: channel i
// of cube[c][s] is the nbins words behind those of channel i - 1.  hits is counted once per (candidate,
// sub-integration), by the first wavefront of the first channel group: a lane every 64th sample, integer columns, a
// butterfly over the lanes.
//
// The refinement.  One kernel text, instantiated per number of bins a lane holds and per stage: lanes run along the
// bins, a wavefront a trial, WAVES trials a workgroup.  CHUNK rows of nbins values are staged into LDS by the whole
// workgroup and read by every wavefront at its own rotation, which is a scalar (v_readlane of the 32 shifts a lane each
// holds): consecutive lanes read consecutive words.  Stage 2 leaves a wavefront's profile in LDS and its first lane
// walks it in ascending b for the two f64 sums.
#include <hip/hip_runtime.h>

#include "cand.h"
#include "fold_kernel.h"
#include "rtlws_internal.h"

namespace rtlws {
namespace cand {

// bin_c(n) of rtlws_fold.h from the phase, as add_group forms it: the high half of (phase >> 32) * nbins (the hits)
__device__ __forceinline__ unsigned bin_of(uint64_t phase, unsigned nbins) { return __umulhi((unsigned)(phase >> 32), nbins); }

template <int WPB>
__global__ __launch_bounds__(WPB * LANES) void cand_fold_kernel(const FoldParams p)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const int lane = threadIdx.x & (LANES - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // workgroup (c, s, g): the channel groups of one candidate and sub-integration side by side
    const unsigned groups = (unsigned)p.groups, nsub = (unsigned)p.nsub;
    const unsigned g = blockIdx.x % groups, cs = blockIdx.x / groups;
    const long s = (long)(cs % nsub);
    const int c = (int)(cs / nsub);
    const int first = (int)(g * WPB + wave) * LANES;           // the wavefront's first channel
    if (first >= p.nchan) return;                             // a whole wavefront behind the row: nothing to do, no barrier to miss
    const int valid = p.nchan - first < LANES ? p.nchan - first : LANES;
    const int chan = first + lane;
    const int delay = lane < valid ? p.delays[(long)c * p.nchan + chan] : -1;
    const bool kept = delay >= 0;                             // lanes behind the row and masked channels add +0.0

    const long n0 = s * p.sub;
    const int len = (int)((n0 + p.sub < p.nsamp ? n0 + p.sub : p.nsamp) - n0);          // this sub-integration's samples: 1 .. sub
    const unsigned nbins = (unsigned)p.nbins;
    const uint64_t step = p.steps[c];
    const uint64_t phase0 = p.phases[c] + (uint64_t)n0 * step;                          // phase_c(n0), mod 2^64
    float* const hist = lds + wave * (p.nbins * LANES);
    float* const col = hist + lane;

    fold::clear_column(col, p.nbins);
    const unsigned long long keepers = __ballot(kept);
    if (keepers != 0) {                                       // a wavefront of masked channels reads no row at all
        // a lane with nothing to read loads what the wavefront's first kept lane loads and adds +0.0 in its place: the
        // loads stand in straight line, and no element is read that the definition does not read
        const int donor = __ffsll(keepers) - 1;
        const int donor_delay = __builtin_amdgcn_readlane(delay, donor);
        const long stride = p.in_stride;
        const float* src = p.rows + (n0 + (kept ? delay : donor_delay)) * stride + (kept ? chan : first + donor);
        uint64_t phase = phase0;
        // whole batches of UNROLL samples, the next batch's loads in flight under this batch's additions
        const int batches = len / UNROLL;
        float x[UNROLL];
        if (batches > 0) {
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) x[u] = src[u * stride];
        }
        for (int k = 0; k < batches; ++k) {
            src += UNROLL * stride;
            float next[UNROLL] = {};
            const bool more = k + 1 < batches;
            if (more) {
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) next[u] = src[u * stride];
            }
#pragma unroll
            for (int u = 0; u < UNROLL; u += fold::GROUP) {
                float y[fold::GROUP];
#pragma unroll
                for (int v = 0; v < fold::GROUP; ++v) y[v] = kept ? x[u + v] : 0.0f;
                fold::add_group<false, fold::GROUP>(col, phase, step, nbins, y);
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) x[u] = next[u];
        }
        int n = batches * UNROLL;
        for (; n < len; ++n) {
            const float v = *src;
            const float x[1] = {kept ? v : 0.0f};
            src += stride;
            fold::add_group<false, 1>(col, phase, step, nbins, x);
        }
    }
    const long cell = (long)c * p.nsub + s;
    fold::RowReads::store(hist, lane, valid, p.cube + (cell * p.nchan + first) * p.nbins, (long)p.nbins, p.nbins);

    if (g == 0 && wave == 0 && p.hits != nullptr) {
        fold::clear_column(col, p.nbins);
        unsigned* const mine = reinterpret_cast<unsigned*>(col);
        uint64_t phase = phase0 + (uint64_t)lane * step;
        const uint64_t stride64 = step * (uint64_t)LANES;
        for (int n = lane; n < len; n += LANES) {
            mine[bin_of(phase, nbins) * LANES] += 1u;
            phase += stride64;
        }
        uint32_t* const dst = p.hits + cell * p.nbins;
        for (int b = 0; b < p.nbins; ++b) {
            unsigned v = mine[b * LANES];
#pragma unroll
            for (int m = LANES / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, LANES);
            if (lane == 0) dst[b] = v;
        }
    }
}

// R: the bins a lane holds, ceil(nbins / 64).  SUMS: stage 2
template <int R, bool SUMS>
__global__ __launch_bounds__(WAVES * LANES) void cand_stage_kernel(const StageParams p)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    static_assert(CHUNK <= LANES, "a lane a shift of the chunk");

    const int tid = threadIdx.x, lane = tid & (LANES - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned tg = (unsigned)trial_groups(p.nt), no = (unsigned)p.no;
    const unsigned g = blockIdx.x % tg, co = blockIdx.x / tg;
    const long o = (long)(co % no), c = (long)(co / no);
    const int t = (int)g * WAVES + wave;                       // the wavefront's trial
    const bool live = t < p.nt;                                // a wavefront behind the trials stages rows and stores nothing
    const int nbins = p.nbins, nk = p.nk;
    const float* const src = p.in + (c * p.no + o) * nk * nbins;
    const int32_t* const tab = p.shifts + (c * p.nt + (live ? t : 0)) * nk;

    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0f;
    for (int k0 = 0; k0 < nk; k0 += CHUNK) {
        const int cnt = nk - k0 < CHUNK ? nk - k0 : CHUNK;
        const int words = cnt * nbins;
        __syncthreads();                                      // the last chunk has been read
        for (int j = tid; j < words; j += WAVES * LANES) lds[j] = src[(long)k0 * nbins + j];
        const int shift = live && lane < cnt ? tab[k0 + lane] : 0;
        __syncthreads();
        if (live) {
            for (int k = 0; k < cnt; ++k) {
                const int a = __builtin_amdgcn_readlane(shift, k);
                const float* const row = lds + k * nbins;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int b = lane + r * LANES;
                    if (b < nbins) {
                        const int j = b + a;
                        acc[r] = acc[r] + row[j >= nbins ? j - nbins : j];
                    }
                }
            }
        }
    }

    const long orow = SUMS ? (c * p.no + o) * p.nt + t : (c * p.nt + t) * p.no + o;
    if (live) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int b = lane + r * LANES;
            if (b < nbins) {
                if (p.out != nullptr) p.out[orow * nbins + b] = acc[r];
                if (p.copy != nullptr) p.copy[orow * nbins + b] = acc[r];
            }
        }
    }
    if constexpr (SUMS) {
        // the profile behind the chunk's rows, then one lane in ascending b: the product of two f32 is exact in f64, so a
        // fused multiply-add rounds what the separate addition rounds
        float* const mine = lds + (CHUNK + wave) * nbins;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int b = lane + r * LANES;
            if (live && b < nbins) mine[b] = acc[r];
        }
        __syncthreads();
        if (live && lane == 0) {
            double stat = 0.0, total = 0.0;
            for (int b = 0; b < nbins; ++b) {
                const double v = (double)mine[b];
                stat = stat + v * v;
                total = total + v;
            }
            p.stat[orow] = stat;
            p.total[orow] = total;
        }
    }
}

// The launch tables: f is handed the instantiation of the bin count's block shape
template <typename F>
static hipError_t with_fold_kernel(int nbins, F&& f)
{
    switch (waves_per_block(nbins)) {
    case 4: return f(&cand_fold_kernel<4>);
    case 2: return f(&cand_fold_kernel<2>);
    default: return f(&cand_fold_kernel<1>);
    }
}

using PerLane = Vals<1, 2, 3, 4>;
static int per_lane(int nbins) { return (nbins + LANES - 1) / LANES; }

hipError_t launch_fold(const FoldParams& p, int ncand, hipStream_t st)
{
    const long blocks = (long)ncand * p.nsub * p.groups;
    return with_fold_kernel(p.nbins, [&](auto kernel) {
        return launch(kernel, dim3((unsigned)blocks), dim3(waves_per_block(p.nbins) * LANES), (size_t)lds_bytes(p.nbins), st, p);
    });
}

hipError_t launch_stage(bool sums, const StageParams& p, int ncand, hipStream_t st)
{
    const long blocks = (long)ncand * p.no * trial_groups(p.nt);
    return pick(PerLane{}, per_lane(p.nbins), [&](auto r) {
        return pick(Bools{}, sums, [&](auto s) {
            return launch(&cand_stage_kernel<decltype(r)::value, decltype(s)::value>, dim3((unsigned)blocks), dim3(WAVES * LANES),
                          (size_t)stage_lds_bytes(p.nbins, sums), st, p);
        });
    });
}

// load_kernel (rtlws_internal.h) for the kernel of a bin count
hipError_t prepare_fold(int nbins)
{
    return with_fold_kernel(nbins, [](auto kernel) { return load_kernel(kernel); });
}

hipError_t prepare_stages(int nbins)
{
    return pick(PerLane{}, per_lane(nbins), [&](auto r) {
        return visit_all(Bools{}, false, [&](auto s) { return load_kernel(&cand_stage_kernel<decltype(r)::value, decltype(s)::value>); });
    });
}

}  // namespace cand
}  // namespace rtlws
