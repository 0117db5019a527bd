// spectrum_anylen.hip -- f64 power spectra of any frame length 2 .. 2^19: Bluestein's algorithm over the four-step
// transform of spectrum_long.hip (the tile's device text is long_tile.h, shared with it).
//
// With w[n] = exp(-i pi n^2 / N), a[n] = x[n] w[n] (n < N, zero up to M), b[n] = conj(w[|n|]) (|n| < N, wrapped around
// M = 2^m >= 2 N - 1): X[k] = w[k] (a (*) b)[k], a circular convolution of length M, and |w[k]| = 1, so the power is
// P[k] = |(a (*) b)[k]|^2: the last multiplication is never done.  Bhat = FFT_M(b) / M is made once per plan
// (anylen_shim.hip, with passes 3 and 2 below); 1/M is a power of two, so the unnormalised inverse comes out right.
//
// M = N1 * N2 as in spectrum_long.hip (n = N2 n1 + n2, k = k1 + N1 k2).  Four launches per group of frames, through
// two workspaces of 16 M bytes per frame:
//   1 anylen_pass_a_in    pass A of the forward transform; its load is convert(x[n]) * w[n] for n < N and ZERO, without
//                         touching memory, for n >= N (the last frame of a batch ends where the caller's buffer ends;
//                         rows n1 with N2 n1 >= N load nothing at all).  Stores ws1, element (k1, n2) at k1 N2 + n2.
//   2 anylen_pass_b_cplx  pass B of the forward transform: Y[k] * Bhat[k] as complex doubles to ws2 in NATURAL order
//                         k = k1 + N1 k2 (Bhat is held in the same order).
//   3 anylen_pass_a_ws    pass A of the inverse, computed as the forward transform of the conjugate: its load is
//                         conj(ws2[n]).  The result is the conjugate of a (*) b; a power does not see that.  Stores ws1.
//   4 anylen_pass_b_pow   pass B of the inverse, |.|^2 of the elements j = k1 + N1 k2 < N, K-frame sums in registers
//                         as in long_pass_b, store to slot (j - N/2) mod N.  The owner of bin 0 stores nothing; the
//                         owner of bin N-1 carries sum_k (K - k) P_k[N-1] (src/spectrum.c:25-33 in closed form) and
//                         stores slot N - N/2 beside its own.  Elements j >= N are discarded.
//
// Global accesses, per wavefront instruction (64 lanes, columns first), T = 8192 / L columns in a tile:
//   1 loads   as long_pass_a (T consecutive samples per n1), and the same T consecutive w[n]: T * 16 B, whole lines
//   1, 3 stores  T consecutive n2 of one k1: whole lines
//   2, 4 loads   8 consecutive n2 (one line) of each of 8 consecutive k1: whole lines
//   2 stores  T consecutive k1 of one k2, T * 16 B >= 128 B: whole lines; Bhat is read at the same addresses
//   3 loads   T consecutive n2 of one n1, T * 16 B: whole lines
//   4 stores  T consecutive k1 of one k2 are T consecutive slots (the shift by N/2 moves a run as a whole; at most
//             one run per row is cut by the wrap), T * 8 / 4 / 1 bytes as in long_pass_b; the rows start wherever
//             N values end, so for odd N the runs do not start on line boundaries
// Per frame that is about 16 M (1) + 48 M (2) + 32 M (3) + 16 M (4) = 112 M bytes plus the input and N / K of a row.
#include "long_tile.h"
#include "spectrum_anylen.h"

namespace rtlws {
namespace anylen {

using namespace lng;

// pass A's epilogue: X[k1] of column n2 times W_M^(n2 k1), to element (k1, n2) of the frame's first workspace
template <int LOG2L>
__device__ __forceinline__ void store_pass_a(const AnyParams& p, long frame, int n2_0, int t, const d2 (&v)[16])
{
    constexpr int T = TILE_POINTS >> LOG2L;
    const int N2 = 1 << p.log2n2;
    const int n2 = n2_0 + t % T, gi = t / T;
    d2* __restrict__ dst = p.ws1 + frame + n2;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const int k1 = out_k<LOG2L>(gi, s);
        const int j = n2 * k1;                                           // < M: no reduction
        const d2 w = f64::cmul(p.twh[j >> TW_SPLIT_LOG2], p.twl[j & ((1 << TW_SPLIT_LOG2) - 1)]);
        dst[(long)k1 * N2] = f64::cmul(v[s], w);
    }
}

// pass B's tile load: the T columns k1_0 .. k1_0 + T - 1 of a frame's first workspace (src points at column k1_0)
template <int LOG2L>
__device__ __forceinline__ void load_pass_b(d2* xs, const d2* __restrict__ src, int t)
{
    constexpr int L = 1 << LOG2L, T = TILE_POINTS / L;
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
        // 64 lanes: 8 columns x 8 consecutive n2 -- eight whole 128-byte lines -- with the columns first
        const int e = t + THREADS * i, rest = e >> 6;
        const int n2 = (rest % (L / 8)) * 8 + ((e >> 3) & 7), col = (rest / (L / 8)) * 8 + (e & 7);
        xs[swz<T>(n2) * T + col] = src[(long)col * L + n2];
    }
}

template <int LOG2L, int IN>
__global__ __launch_bounds__(THREADS) void anylen_pass_a_in(const AnyParams p)
{
    extern __shared__ __attribute__((aligned(16))) double2 xs[];
    constexpr int L = 1 << LOG2L, T = TILE_POINTS / L;                  // L = N1
    const int t = threadIdx.x;
    const int N2 = 1 << p.log2n2;
    const int tiles = N2 / T;
    const unsigned bid = xcd_chunked(blockIdx.x, gridDim.x);
    const long f = bid / tiles;
    const int n2_0 = (int)(bid % tiles) * T;
    const long M = (long)L << p.log2n2;
    const int N = p.n;
    const long in0 = f * N;                                              // frames follow each other without padding

#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int e = t + THREADS * i, col = e % T, n1 = e / T;
        const int n = n1 * N2 + n2_0 + col;                              // < M <= 2^20
        d2 a = make_double2(0.0, 0.0);
        if (n < N) a = f64::cmul(load_sample<IN>(p.in, in0 + n, p.in_scale), p.chirp[n]);
        xs[swz<T>(n1) * T + col] = a;
    }
    __syncthreads();

    d2 v[16];
    tile_fft<LOG2L>(xs, p.twc, t, v);
    store_pass_a<LOG2L>(p, f * M, n2_0, t, v);
}

template <int LOG2L>
__global__ __launch_bounds__(THREADS) void anylen_pass_b_cplx(const AnyParams p)
{
    extern __shared__ __attribute__((aligned(16))) double2 xs[];
    constexpr int L = 1 << LOG2L, T = TILE_POINTS / L;                  // L = N2
    const int t = threadIdx.x;
    const int N1 = 1 << p.log2n1;
    const int tiles = N1 / T;
    const long f = blockIdx.x / tiles;
    const int k1_0 = (int)(blockIdx.x % tiles) * T;
    const long M = (long)L << p.log2n1;

    load_pass_b<LOG2L>(xs, p.ws1 + f * M + (long)k1_0 * L, t);
    __syncthreads();

    d2 v[16];
    tile_fft<LOG2L>(xs, p.twc, t, v);

    const int k1 = k1_0 + t % T, gi = t / T;
    d2* __restrict__ dst = p.ws2 + f * M + k1;
    const d2* __restrict__ bh = p.bhat + k1;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const long k = (long)N1 * out_k<LOG2L>(gi, s);                   // + k1: natural order
        dst[k] = f64::cmul(v[s], bh[k]);
    }
}

template <int LOG2L>
__global__ __launch_bounds__(THREADS) void anylen_pass_a_ws(const AnyParams p)
{
    extern __shared__ __attribute__((aligned(16))) double2 xs[];
    constexpr int L = 1 << LOG2L, T = TILE_POINTS / L;                  // L = N1
    const int t = threadIdx.x;
    const int N2 = 1 << p.log2n2;
    const int tiles = N2 / T;
    const unsigned bid = xcd_chunked(blockIdx.x, gridDim.x);
    const long f = bid / tiles;
    const int n2_0 = (int)(bid % tiles) * T;
    const long M = (long)L << p.log2n2;
    const d2* __restrict__ src = p.ws2 + f * M + n2_0;

#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int e = t + THREADS * i, col = e % T, n1 = e / T;
        const d2 z = src[(long)n1 * N2 + col];
        xs[swz<T>(n1) * T + col] = make_double2(z.x, -z.y);
    }
    __syncthreads();

    d2 v[16];
    tile_fft<LOG2L>(xs, p.twc, t, v);
    store_pass_a<LOG2L>(p, f * M, n2_0, t, v);
}

template <int LOG2L, int ROWS>
__global__ __launch_bounds__(THREADS) void anylen_pass_b_pow(const AnyParams p)
{
    extern __shared__ __attribute__((aligned(16))) double2 xs[];
    constexpr int L = 1 << LOG2L, T = TILE_POINTS / L;                  // L = N2
    const int t = threadIdx.x;
    const int N1 = 1 << p.log2n1;
    const int tiles = N1 / T;
    const long row = blockIdx.x / tiles;
    const int k1_0 = (int)(blockIdx.x % tiles) * T;
    const long M = (long)L << p.log2n1;
    const int N = p.n, half = N / 2;
    if (k1_0 >= N) return;                                               // the whole workgroup: every j of the tile is >= N
    const int K = p.k_avg;
    const int k1 = k1_0 + t % T, gi = t / T;

    double acc[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) acc[s] = 0.0;
    double dc = 0.0;

    for (int kf = 0; kf < K; ++kf) {
        if (kf) __syncthreads();                                         // the previous frame's readers are done
        load_pass_b<LOG2L>(xs, p.ws1 + (row * K + kf) * M + (long)k1_0 * L, t);
        __syncthreads();

        d2 v[16];
        tile_fft<LOG2L>(xs, p.twc, t, v);
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const double pw = v[s].x * v[s].x + v[s].y * v[s].y;
            acc[s] += pw;
            if (k1 + N1 * out_k<LOG2L>(gi, s) == N - 1) dc += (double)(K - kf) * pw;    // bin N-1
        }
    }

    const long base = row * N;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const int j = k1 + N1 * out_k<LOG2L>(gi, s);                     // < M <= 2^20
        if (j == 0 || j >= N) continue;                                  // bin 0's slot is written by the owner of bin N-1
        store_value<ROWS>(p, base + (j >= half ? j - half : j - half + N), acc[s]);
        if (j == N - 1) store_value<ROWS>(p, base + (N - half), dc);
    }
}

using Lengths = Vals<7, 8, 9, 10>;
using Inputs = Vals<IN_CU8, IN_CS32, IN_RF32>;
using Rows = Vals<ROWS_F64, ROWS_F32, ROWS_U8>;

// M / 8192 tiles per frame in every pass
static unsigned grid_of(const AnyParams& p, long frames) { return (unsigned)(frames << (p.log2n1 + p.log2n2 - 13)); }

hipError_t launch_pass_a_in(const AnyParams& p, int in_kind, long frames, hipStream_t st)
{
    return pick(Lengths{}, p.log2n1, [&](auto l) {
        return pick(Inputs{}, in_kind, [&](auto in) {
            return launch(&anylen_pass_a_in<l, in>, dim3(grid_of(p, frames)), dim3(THREADS), LDS_BYTES, st, p);
        });
    });
}

hipError_t launch_pass_b_cplx(const AnyParams& p, long frames, hipStream_t st)
{
    return pick(Lengths{}, p.log2n2, [&](auto l) {
        return launch(&anylen_pass_b_cplx<l>, dim3(grid_of(p, frames)), dim3(THREADS), LDS_BYTES, st, p);
    });
}

hipError_t launch_pass_a_ws(const AnyParams& p, long frames, hipStream_t st)
{
    return pick(Lengths{}, p.log2n1, [&](auto l) {
        return launch(&anylen_pass_a_ws<l>, dim3(grid_of(p, frames)), dim3(THREADS), LDS_BYTES, st, p);
    });
}

hipError_t launch_pass_b_pow(const AnyParams& p, int rows_kind, long rows, hipStream_t st)
{
    return pick(Lengths{}, p.log2n2, [&](auto l) {
        return pick(Rows{}, rows_kind, [&](auto r) {
            return launch(&anylen_pass_b_pow<l, r>, dim3(grid_of(p, rows)), dim3(THREADS), LDS_BYTES, st, p);
        });
    });
}

hipError_t prepare_anylen(int log2m, int in_kind, int rows_kind, int device)
{
    hipError_t e = pick(Lengths{}, log2_n1(log2m), [&](auto l) {
        const hipError_t e1 = lds_opt_in(&anylen_pass_a_ws<l>, device, LDS_BYTES);
        if (e1 != hipSuccess) return e1;
        return pick(Inputs{}, in_kind, [&](auto in) { return lds_opt_in(&anylen_pass_a_in<l, in>, device, LDS_BYTES); });
    });
    if (e != hipSuccess) return e;
    return pick(Lengths{}, log2_n2(log2m), [&](auto l) {
        const hipError_t e2 = lds_opt_in(&anylen_pass_b_cplx<l>, device, LDS_BYTES);
        if (e2 != hipSuccess) return e2;
        return pick(Rows{}, rows_kind, [&](auto r) { return lds_opt_in(&anylen_pass_b_pow<l, r>, device, LDS_BYTES); });
    });
}

}  // namespace anylen
}  // namespace rtlws
