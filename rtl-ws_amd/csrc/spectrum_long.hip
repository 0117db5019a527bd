// spectrum_long.hip -- f64 power spectra of 2^14 .. 2^20-point frames: a four-step FFT through device memory.
//
// N = N1 * N2 with N1 = 2^ceil(m/2), N2 = 2^floor(m/2) (128 .. 1024 each); n = N2 n1 + n2, k = k1 + N1 k2:
//   X[k1 + N1 k2] = sum_n2 W_N2^(n2 k2) [ W_N^(n2 k1) sum_n1 W_N1^(n1 k1) x[N2 n1 + n2] ]
//
// Pass A (long_pass_a): a workgroup takes a tile of T = 8192 / N1 consecutive n2 and all n1, converts the input as
// the reference does (src/spectrum.c:54-58,72-76,90-94), runs the T N1-point transforms over n1, multiplies by
// W_N^(n2 k1) and writes complex doubles to the workspace, element (k1, n2) of a frame at k1 * N2 + n2.
// Pass B (long_pass_b): a workgroup takes a tile of T = 8192 / N2 consecutive k1 and all n2, runs the T N2-point
// transforms over n2, takes |X|^2, sums the K frames of a row in registers and stores the row: slot
// (k + N/2) mod N flips the top bit of k2, so the fft-shift costs nothing; the DC-slot rule (src/spectrum.c:25-33 in
// closed form, slot N/2 = sum_k (K - k) P_k[N-1]) is carried by the thread that owns bin N-1, which writes slot N/2
// beside its own, and the thread that owns bin 0 writes nothing.
//
// The sub-transform of both passes (tile_fft): the tile lives in LDS as 8192 complex doubles, element (pos, col) at
// swz(pos) * T + col, and each of the 512 threads owns sixteen points of one column per stage.  Decimation in
// frequency, in place, radix 16 in registers (fft_regs_impl.h through fft_regs_f64.h) with one LDS exchange between
// register stages: L = 128: 16 x 8, 256: 16 x 16, 512: 16 x 16 x 2, 1024: 16 x 16 x 4 (the last radix R < 16 as
// 16 / R butterflies per thread).  Lanes run over the columns first, so a lane group of a ds_read_b128 or
// ds_write_b128 covers T >= 8 consecutive 16-byte slots of one position: with T >= 16 every access is conflict-free
// whatever the positions are; with T = 8 (L = 1024) two positions share a 256-byte bank row and bit 0 of the
// position is swizzled with bit 2, which makes the four positions a read's lane group touches alternate in every
// stage (tools/lds_sim.py's bank model: tests/test_long_cpu.py).
//
// Global accesses, per wavefront instruction (64 lanes, columns first):
//   pass A loads   T consecutive samples per n1: whole 128-byte lines where T samples fill them -- cmplx_s32 for
//                  N1 <= 512, real f32 for N1 <= 256, cmplx_u8 at N1 = 128.  The rest CANNOT: the tile is bounded by
//                  the LDS (T * N1 = 8192), so at N1 = 1024 a run is 8 samples (16 B of cmplx_u8); the neighbouring
//                  tiles' workgroups read the rest of the line at about the same time on the same XCD (xcd_chunked).
//   pass A stores  T consecutive n2 of one k1: T * 16 B >= 128 B, whole lines.
//   pass B loads   8 consecutive n2 (128 B, one line) of each of 8 consecutive k1 per instruction: whole lines.
//   pass B stores  T consecutive k1 of one k2: T * 8 B of f64 rows (whole lines for N2 <= 512, 64 B at N2 = 1024),
//                  T * 4 B of f32 rows (N2 <= 256), T bytes of payload (N2 = 128): bounded by the tile like the loads
//                  of pass A, and a row is N / K of the 34 N bytes a frame moves.
//
// tile_fft, the tile's index maps, the sample conversion and the row store live in long_tile.h: spectrum_anylen.hip
// builds its kernels from the same text.
#include "long_tile.h"

namespace rtlws {
namespace lng {

template <int LOG2L, int IN>
__global__ __launch_bounds__(THREADS) void long_pass_a(const LongParams p)
{
    extern __shared__ __attribute__((aligned(16))) double2 xs[];
    constexpr int L = 1 << LOG2L, T = TILE_POINTS / L;                  // L = N1
    const int t = threadIdx.x;
    const int N2 = 1 << p.log2n2;
    const int tiles = N2 / T;
    const unsigned bid = xcd_chunked(blockIdx.x, gridDim.x);
    const long f = bid / tiles;
    const int n2_0 = (int)(bid % tiles) * T;
    const long N = (long)L << p.log2n2;
    const long frame = f * N;

#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int e = t + THREADS * i, col = e % T, n1 = e / T;
        xs[swz<T>(n1) * T + col] = load_sample<IN>(p.in, frame + (long)n1 * N2 + n2_0 + col, p.in_scale);
    }
    __syncthreads();

    d2 v[16];
    tile_fft<LOG2L>(xs, p.twc, t, v);

    const int n2 = n2_0 + t % T, gi = t / T;
    d2* __restrict__ dst = p.ws + frame + n2;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const int k1 = out_k<LOG2L>(gi, s);
        const int j = n2 * k1;                                           // < N: no reduction
        const d2 w = f64::cmul(p.twh[j >> TW_SPLIT_LOG2], p.twl[j & ((1 << TW_SPLIT_LOG2) - 1)]);
        dst[(long)k1 * N2] = f64::cmul(v[s], w);
    }
}

template <int LOG2L, int ROWS>
__global__ __launch_bounds__(THREADS) void long_pass_b(const LongParams p)
{
    extern __shared__ __attribute__((aligned(16))) double2 xs[];
    constexpr int L = 1 << LOG2L, T = TILE_POINTS / L;                  // L = N2
    const int t = threadIdx.x;
    const int N1 = 1 << p.log2n1;
    const int tiles = N1 / T;
    const long row = blockIdx.x / tiles;
    const int k1_0 = (int)(blockIdx.x % tiles) * T;
    const long N = (long)L << p.log2n1;
    const int K = p.k_avg;
    const int k1 = k1_0 + t % T, gi = t / T;
    const bool last_k1 = k1 == N1 - 1;

    double acc[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) acc[s] = 0.0;
    double dc = 0.0;

    for (int kf = 0; kf < K; ++kf) {
        const d2* __restrict__ src = p.ws + (row * K + kf) * N + (long)k1_0 * L;
        if (kf) __syncthreads();                                         // the previous frame's readers are done
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {
            // 64 lanes: 8 columns x 8 consecutive n2 -- eight whole 128-byte lines -- with the columns first, so that
            // 8 consecutive lanes write 8 consecutive LDS slots
            const int e = t + THREADS * i, rest = e >> 6;
            const int n2 = (rest % (L / 8)) * 8 + ((e >> 3) & 7), col = (rest / (L / 8)) * 8 + (e & 7);
            xs[swz<T>(n2) * T + col] = src[(long)col * L + n2];
        }
        __syncthreads();

        d2 v[16];
        tile_fft<LOG2L>(xs, p.twc, t, v);
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const double pw = v[s].x * v[s].x + v[s].y * v[s].y;
            acc[s] += pw;
            if (last_k1 && out_k<LOG2L>(gi, s) == L - 1) dc += (double)(K - kf) * pw;   // bin N-1
        }
    }

    const long base = row * N + k1;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const int k2 = out_k<LOG2L>(gi, s);
        if (k1 == 0 && k2 == 0) continue;                                // slot N/2 is written by the owner of bin N-1
        store_value<ROWS>(p, base + (long)N1 * (k2 ^ (L / 2)), acc[s]);
        if (last_k1 && k2 == L - 1) store_value<ROWS>(p, row * N + N / 2, dc);
    }
}

using Lengths = Vals<7, 8, 9, 10>;
using Inputs = Vals<IN_CU8, IN_CS32, IN_RF32>;
using Rows = Vals<ROWS_F64, ROWS_F32, ROWS_U8>;

hipError_t launch_long_pass_a(const LongParams& p, int in_kind, long frames, hipStream_t st)
{
    const long blocks = frames << (p.log2n2 - (13 - p.log2n1));          // N2 / T tiles per frame
    return pick(Lengths{}, p.log2n1, [&](auto l) {
        return pick(Inputs{}, in_kind, [&](auto in) {
            return launch(&long_pass_a<l, in>, dim3((unsigned)blocks), dim3(THREADS), LDS_BYTES, st, p);
        });
    });
}

hipError_t launch_long_pass_b(const LongParams& p, int rows_kind, long rows, hipStream_t st)
{
    const long blocks = rows << (p.log2n1 - (13 - p.log2n2));            // N1 / T tiles per row
    return pick(Lengths{}, p.log2n2, [&](auto l) {
        return pick(Rows{}, rows_kind, [&](auto r) {
            return launch(&long_pass_b<l, r>, dim3((unsigned)blocks), dim3(THREADS), LDS_BYTES, st, p);
        });
    });
}

hipError_t prepare_long(int log2n, int in_kind, int rows_kind, int device)
{
    const hipError_t e = pick(Lengths{}, log2_n1(log2n), [&](auto l) {
        return pick(Inputs{}, in_kind, [&](auto in) { return lds_opt_in(&long_pass_a<l, in>, device, LDS_BYTES); });
    });
    if (e != hipSuccess) return e;
    return pick(Lengths{}, log2_n2(log2n), [&](auto l) {
        return pick(Rows{}, rows_kind, [&](auto r) { return lds_opt_in(&long_pass_b<l, r>, device, LDS_BYTES); });
    });
}

}  // namespace lng
}  // namespace rtlws
