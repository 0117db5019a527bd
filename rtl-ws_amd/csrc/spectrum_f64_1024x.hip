// spectrum_f64_1024x.hip -- 1024-point rectangular cmplx_u8 frames -> power spectra in DOUBLE with
// ONE LDS transposition per frame instead of two (the reference's arithmetic: src/spectrum.c:54-60
// convert, :21 f64 forward DFT, :23-34 |X|^2 + fft-shift + accumulate + DC-slot rule; K loop of
// src/cbb_main.c:50-59; dB / payload epilogue of src/cbb_main.c:121-130 in double).
//
// Why: spectrum_f64_fused.hip (1024 = 16 x 16 x 4, two transpositions of 16-byte elements) moves
// 64 KiB per frame through LDS, and on gfx950 a ds_write_b128 costs 13 cycles per wave-instruction
// (~79 B/clk/CU, a third of the read rate): with f32 rows the kernel is bound by that and by the
// f64 issue rate together, not by HBM (ablations: 118 us per 65 536 frames, 90 us without the LDS
// traffic, stores free; profiles/r04_ab_f64_variants.txt).  This kernel decomposes
//      1024 = 4 x 256,   256 = 16 x 16
// and does the radix-4 FIRST, where the data are still the 8-bit samples:
//   pass 0  n = 256 a + m: lane t loads x[64 j + t], j < 16 (one 128-byte line per wave-instruction,
//           as everywhere), i.e. a = j / 4 and m = 64 b + t with b = j % 4.  y_p[m] = sum_a x[256a+m]
//           (-i)^(a p) is exact INTEGER arithmetic (|y| <= 1020), and
//   cross-row transpose  the 256-point transform p wants m = c + 16 r on lane (p, c): a 4 x 4
//           exchange (lane row t / 16  <->  index p).  Lane (row p, column c) then holds
//           y_p[c + 16 r], r = 4 b + g, r = 0 .. 15 in order.
//           K = 1 instantiations: both at once on the MATRIX pipe.  The coefficients (-i)^(a p) act on
//           (re, im) as 0 / +-1, so the radix-4 is a 16 x 32 int8 matrix A (two constants per lane: real
//           and imaginary parts) times the lane's own eight sample bytes of one b, and the operand /
//           result lane maps of v_mfma_i32_16x16x32_i8 ARE the exchange: 8 v_perm_b32 (2-byte loads ->
//           dwords) + 8 v_xor_b32 (offset-binary -> signed) + 8 MFMAs per frame, results int32 in pass
//           A's registers and lanes, the offset 512 (1 + i) of y_0 put back through the C operand so that
//           every integer is the vector form's (rows bit-identical: tests/test_f64_1024x_digest_gpu.py).
//           K > 1 instantiations (256 VGPRs, no room for the result quads): on the vector pipe -- packed
//           int16 (re, im) pairs, v_pk_add_u16 / v_pk_sub_i16, 11 instructions per b; two
//           v_permlane16_swap + two v_permlane32_swap of ONE dword per value per b; 32 sign extensions.
//   pass A  the twiddle owed, W_1024^(p m) = W_1024^(p c) (W_64^p)^r, is a lane constant times a
//           geometric sequence in the register index: the radix-16 over r absorbs the sequence in
//           fused-multiply-add form (fft_regs_impl.h "last pass": 8 (cos, tan) pairs per lane, 192
//           operations), the constant rides on ...
//   twB     ... the inner twiddles W_256^(c q) (one complex multiply per point, which also carries the
//           exact 1/128 input scale), then the ONE LDS transposition (16-byte elements, 32 KiB of LDS
//           traffic per frame), lane t = 4 q + p reading its sixteen c contiguously,
//   pass B  radix-16 over c: lane t ends with bins k = 64 q' + t, q' = 0 .. 15 -- for every q' the
//           wavefront stores 64 consecutive outputs (256 B of f32 / 512 B of f64), lane-contiguous.
// f64 operations per frame: 192 + 64 + 148 + 32 (|X|^2) = 436 against 484, LDS bytes halved, no
// workgroup barrier (one wavefront per frame).  Same results as spectrum_f64_fused.hip to rounding
// (strict-metric error ~1e-12); tests/test_f64_1024x_gpu.py.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rtlws_internal.h"
#include "fft_regs_f64.h"

#define RTLWS_X_LDS_ORDER 0

namespace rtlws {

using namespace f64;

typedef short pk_i16 __attribute__((ext_vector_type(2)));      // (re, im) of one integer point
typedef unsigned short pk_u16 __attribute__((ext_vector_type(2)));
typedef int v4i __attribute__((ext_vector_type(4)));
#define RTLWS_GLOBAL __attribute__((address_space(1)))          // a pointer the compiler need not prove global

// Row p of the radix-4 as an int8 A operand: eight bytes, element 2 a + ri = the coefficient of x[a].re (ri = 0) /
// x[a].im (ri = 1) in the real (im = false) or imaginary part of x[a] (-i)^(a p)
constexpr long radix4_coef(int p, bool im)
{
    unsigned long v = 0;
    for (int a = 0; a < 4; ++a) {
        const int e = (a * p) & 3;                                          // (cr, ci) = (-i)^e
        const int cr = e == 0 ? 1 : e == 2 ? -1 : 0, ci = e == 1 ? -1 : e == 3 ? 1 : 0;
        v |= (unsigned long)(unsigned char)(im ? ci : cr) << (16 * a);
        v |= (unsigned long)(unsigned char)(im ? cr : -ci) << (16 * a + 8);
    }
    return (long)v;
}

// V_PERMLANE16_SWAP: odd rows (16 lanes) of a <-> even rows of b; V_PERMLANE32_SWAP: upper half of a
// <-> lower half of b (tools/permlane_probe.hip)
__device__ __forceinline__ void swap_rows16(unsigned& a, unsigned& b)
{
    const auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
    a = r[0];
    b = r[1];
}
__device__ __forceinline__ void swap_rows32(unsigned& a, unsigned& b)
{
    const auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    a = r[0];
    b = r[1];
}

// V_WRITELANE_B32 as the compiler's own intrinsic (hipcc 7.2 has the readlane builtin but not this one): lane `lane`
// of `old` replaced by the scalar `src`.  Not inline assembly: a VALU-written SGPR needs wait states before a VALU
// reads it, which the compiler inserts around its own instructions only.
extern "C" __device__ int rtlws_writelane(int src, int lane, int old) __asm("llvm.amdgcn.writelane.i32");

// WAVES = 1: one wavefront per workgroup, output rows dealt statically (row = workgroup + i * grid) -- small
// batches and the drop-in calls.  WAVES > 1: ONE workgroup of WAVES wavefronts per CU (WAVES / 4 per SIMD),
// the workgroup's rows (b + i * grid) handed to its wavefronts one at a time through a counter in LDS.  Why
// (profiles/r05_wave_timeline_2_per_simd.txt): the SIMD arbitrates its vector pipe by age, the older of two
// co-resident wavefronts runs at 0.95 of its solo rate and the younger gets the leftover slots -- with rows dealt
// statically the older one left after 122 of 198 k cycles and the younger finished its last 21 rows alone, at
// the solo rate (3 640 cycles per row against 2 820 for the pair).  Nothing but the row-to-wavefront map differs:
// no barrier in the frame loop (the wavefronts share no LDS data), results bit-identical.
template <int OUT, bool KONE, bool ROWF32, int WAVES>
__global__ __launch_bounds__(64 * WAVES, WAVES == 1 ? 2 : WAVES / 4) void spectra_f64_1024x(const SpectraParamsF64 p)
{
    constexpr int N = 1024;
    static_assert(!(ROWF32 && OUT == OUT_PAYLOAD), "payload rows are bytes in either form");
    static_assert(WAVES == 1 || WAVES % 4 == 0, "whole wavefronts per SIMD");
    extern __shared__ __attribute__((aligned(16))) double2 lds_all[];
    // (three wavefronts per SIMD -- WAVES = 12 at 164 VGPRs, inner twiddles and a two-halves transposition in LDS --
    // was built and measured slower, profiles/r05_ab_three_wavefronts_per_simd.txt; tools/variants/csrc_hooks.patch)
    constexpr int SLICE_F2 = 17 * 64;                                  // double2 elements per wavefront
    double2* const ldsd = lds_all + (WAVES == 1 ? 0 : (threadIdx.x >> 6) * SLICE_F2);   // this wavefront's own slice
    unsigned* const row_counter = reinterpret_cast<unsigned*>(lds_all + WAVES * SLICE_F2);    // (WAVES > 1)

    const int t = threadIdx.x & 63;
    const int K = KONE ? 1 : p.k_avg;
    // rows and frames are counted in 32 bits (2^31 frames are 4 TiB of samples): the scalar unit compares 32-bit
    // integers, a 64-bit signed compare goes to the vector pipe.  Addresses are 64-bit scalar arithmetic.
    const int ngroups = (int)p.ngroups;
    // this workgroup's output rows: blockIdx.x + i * gridDim.x; the first WAVES indices i are dealt statically.
    // The row index is wave-uniform and is carried on the scalar unit (readfirstlane: the wavefront's number is
    // uniform, which the compiler cannot see), so every frame, prefetch and row address below is scalar arithmetic
    // and the loads and stores take the form scalar base + per-lane byte offset + immediate.
    int g = blockIdx.x;
    if constexpr (WAVES > 1) {
        g = __builtin_amdgcn_readfirstlane((int)(blockIdx.x + (threadIdx.x >> 6) * gridDim.x));
        if (threadIdx.x == 0) *row_counter = WAVES;
    }
    // the row after `cur`: WAVES = 1 strides, WAVES > 1 takes the workgroup's next undone row (lane 0's LDS
    // atomic, broadcast); >= ngroups: none left.  The atomic is spelt as an increment that wraps at 2^32 - 1
    // (ds_inc_rtn_u32), which is a fetch-and-add of one for every count a launch can reach: around a fetch_add the
    // compiler's atomic optimiser puts a v_mbcnt / popcount / v_readfirstlane wrapper, nine vector instructions
    // per row for an atomic that one lane issues anyway.
    auto next_row = [&](int cur) -> int {
        if constexpr (WAVES == 1) {
            return cur + (int)gridDim.x;
        } else {
            unsigned v = 0;
            if (t == 0) v = __builtin_amdgcn_atomic_inc32(row_counter, 0xffffffffu, __ATOMIC_RELAXED, "workgroup");
            return (int)(blockIdx.x + (unsigned)__builtin_amdgcn_readfirstlane((int)v) * gridDim.x);
        }
    };

    // The front end (radix-4 + cross-row transpose) on the matrix pipe: the K = 1 instantiations.  The K-frame
    // accumulators sit at 256 VGPRs and spill with it; they keep the vector-pipe form.
    constexpr bool MFMA_FE = KONE;
    // vector form: raw[j] = x[64 j + t].  Matrix form: raw[2 b + h] = the samples a = 2 h (low half) and 2 h + 1
    // of j = 4 a + b: the lane's B operand of MFMA b is (raw[2 b], raw[2 b + 1]), bytes in order (a, re / im)
    unsigned raw[MFMA_FE ? 8 : 16];
    unsigned lane_in = 2u * t;                    // the lane's byte offset in a frame's 128-byte lines
    auto load_raw = [&](int frame) {
        const char* base = reinterpret_cast<const char*>(p.in) + (long)frame * (2 * N);          // uniform
        // kept whole, the base in a scalar pair and the lane's offset in 32 bits (passed through in place, so no copy):
        // else p.in + lane is hoisted as a 64-bit vector value and the frame added to it per lane (v_lshl_add_u64)
        asm("" : "+s"(base), "+v"(lane_in));
        const RTLWS_GLOBAL uint16_t* const src = (const RTLWS_GLOBAL uint16_t*)(base + lane_in);
        if constexpr (MFMA_FE) {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    pk_u16 w;
                    w.x = __builtin_nontemporal_load(src + 64 * (8 * h + b));
                    w.y = __builtin_nontemporal_load(src + 64 * (8 * h + 4 + b));
                    raw[2 * b + h] = __builtin_bit_cast(unsigned, w);
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) raw[j] = __builtin_nontemporal_load(src + 64 * j);
        }
    };
    // constant operands of the matrix form.  A (16 x 32, lane l holds row l & 15, k = 8 (l >> 4) + e): row 4 p + gg
    // takes row p of the radix-4 from k-block gg alone, so lane (g, 4 p + gg) is zero unless g == gg.  C: the samples
    // enter as signed bytes (x ^ 0x80); the 128 (1 + i) per sample the vector form carries -- it reaches X[0] only --
    // is 512 (1 + i) in y_0 = result rows 0 .. 3 = lanes 0 .. 15: added back, every integer is the vector form's.
    long a_re = 0, a_im = 0;
    if ((t >> 4) == (t & 3)) {
        const int pp = (t & 15) >> 2;
        a_re = pp == 0 ? radix4_coef(0, false) : pp == 1 ? radix4_coef(1, false) : pp == 2 ? radix4_coef(2, false) : radix4_coef(3, false);
        a_im = pp == 0 ? radix4_coef(0, true) : pp == 1 ? radix4_coef(1, true) : pp == 2 ? radix4_coef(2, true) : radix4_coef(3, true);
    }
    const int c_dc = t < 16 ? 512 : 0;
    const v4i c_off = {c_dc, c_dc, c_dc, c_dc};

    // lane constants, resident for the life of the (persistent) workgroup.  The 24 table loads and the first
    // frame's samples are issued together, ahead of the barrier: one memory round trip in the head of a launch, not
    // two.  twxb is [slot][lane] on the device: a wave-instruction reads 1 KiB contiguous.
    f2 twA[8], twB[16];
#pragma unroll
    for (int m = 0; m < 8; ++m) twA[m] = p.twxa[(t >> 4) * 8 + m];
#pragma unroll
    for (int s = 0; s < 16; ++s) twB[s] = p.twxb[s * 64 + t];
    if (g < ngroups) load_raw(g * K);
    if constexpr (WAVES > 1) __syncthreads();                  // the only barrier of the kernel (the row counter)
#pragma unroll
    for (int m = 0; m < 8; ++m) asm volatile("" ::"v"(twA[m].x), "v"(twA[m].y));      // retired before the loop
#pragma unroll
    for (int s = 0; s < 16; ++s) asm volatile("" ::"v"(twB[s].x), "v"(twB[s].y));

    const int wp = t >> 4, wc = t & 15;         // writer side of the transposition: lane (p, c)
    unsigned lane_out = (OUT == OUT_PAYLOAD ? 1u : ROWF32 ? 4u : 8u) * t;     // the lane's byte offset in a row's 64 outputs

    while (g < ngroups) {
        const int g_next = next_row(g);
        double acc[16];
        double wdc = 0.0;
#pragma unroll
        for (int u = 0; u < 16; ++u) acc[u] = 0.0;

#pragma nounroll      // (left alone the compiler unrolls the 32-bit frame loop by two: twice the code, nothing gained)
        for (int kf = 0; kf < K; ++kf) {
            const int frame = g * K + kf;

            auto prefetch = [&]() {
                int nf = frame + 1;
                if (kf + 1 == K) nf = g_next * K;
                if (nf >= ngroups * K) nf = frame;        // in bounds, result unused  (this form: the ternary
                                                          // spelling costs the K > 1 instantiations 12-15 spilled VGPRs)
                load_raw(nf);
            };
            f2 v[16];
            if constexpr (MFMA_FE) {
                // ---- pass 0 and the cross-row transpose as eight v_mfma_i32_16x16x32_i8: D = A B + C with B
                // (32 x 16, lane l holds column l & 15, k = 8 (l >> 4) + e) = this lane's four samples of
                // m = 64 b + t, so column c, k-block t >> 4; D (lane l holds column l & 15, rows 4 (l >> 4) + i):
                // lane (p, c), register i of MFMA b = Re | Im y_p[c + 16 (4 b + i)], as int32 -- pass A's layout.
                v4i yre[4], yim[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const unsigned lo = raw[2 * b] ^ 0x80808080u, hi = raw[2 * b + 1] ^ 0x80808080u;
                    const long xb = (long)(((unsigned long)hi << 32) | lo);
                    yre[b] = __builtin_amdgcn_mfma_i32_16x16x32_i8(a_re, xb, c_off, 0, 0, 0);
                    yim[b] = __builtin_amdgcn_mfma_i32_16x16x32_i8(a_im, xb, c_off, 0, 0, 0);
                }
                // the eight MFMAs back to back, the conversions behind the last one: left alone the scheduler
                // converts each quad as it lands and waits (s_nop 5 .. 7) eight times a frame
                __builtin_amdgcn_sched_barrier(0);
                prefetch();
#pragma unroll
                for (int r = 0; r < 16; ++r) v[r] = mk((double)yre[r >> 2][r & 3], (double)yim[r >> 2][r & 3]);
            } else {
                // ---- pass 0: radix-4 over a on packed int16 points.  The 128 offset of the samples
                // only reaches y_0 -> bin 0 of every 256-point transform p = 0 -> bins k = 4 k' + 0 ...
                // no: it reaches exactly X[0] (a constant sequence has a single non-zero bin), which is
                // never output (src/spectrum.c:31); it is kept, as in the other kernels.
                unsigned y[16];                     // y[4 b + pp]
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    pk_i16 x[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        const unsigned r = raw[4 * a + b];
                        // bytes (re, im) -> int16 pair (re | im << 16): one v_perm_b32
                        x[a] = __builtin_bit_cast(pk_i16, __builtin_amdgcn_perm(r, r, 0x0c010c00u));
                    }
                    const pk_i16 s0 = x[0] + x[2], s1 = x[0] - x[2], s2 = x[1] + x[3], s3 = x[1] - x[3];
                    const pk_i16 rot = {s3.y, (short)-s3.x};                 // -i * s3
                    y[4 * b + 0] = __builtin_bit_cast(unsigned, (pk_i16)(s0 + s2));
                    y[4 * b + 1] = __builtin_bit_cast(unsigned, (pk_i16)(s1 + rot));
                    y[4 * b + 2] = __builtin_bit_cast(unsigned, (pk_i16)(s0 - s2));
                    y[4 * b + 3] = __builtin_bit_cast(unsigned, (pk_i16)(s1 - rot));
                }
                prefetch();

                // ---- cross-row 4 x 4 transpose (lane row <-> p): afterwards lane (row p, column c)
                // holds y_p[c + 16 (4 b + g)] in y[4 b + g]
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    swap_rows16(y[4 * b + 0], y[4 * b + 1]);
                    swap_rows16(y[4 * b + 2], y[4 * b + 3]);
                    swap_rows32(y[4 * b + 0], y[4 * b + 2]);
                    swap_rows32(y[4 * b + 1], y[4 * b + 3]);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    v[r] = mk((double)(short)(y[r] & 0xffffu), (double)((int)y[r] >> 16));
            }

            // ---- pass A: radix-16 over r with the geometric pre-twiddle (W_64^p)^r absorbed;
            // slot s holds index q = rev16(s)
            fft_last<16>(v, 0, twA);
            // inner twiddles W_256^(c q) x the lane constant W_1024^(p c) x 1/128
#pragma unroll
            for (int s = 0; s < 16; ++s) v[s] = cmul(v[s], twB[s]);

            // ---- the one transposition: (p, c; q) -> lane 4 q + p, sixteen c contiguous (rows
            // padded 16 -> 17 double2: conflict-free ds_write_b128 and ds_read_b128)
            // the slice is this wavefront's own: ordering within the wavefront only, never an s_barrier.
            // Wavefront-scope fences: the compiler may spread the writes over pass A's tail and start pass B
            // under the reads.
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int s = 0; s < 16; ++s) ldsd[17 * (4 * rev16(s) + wp) + wc] = v[s];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int c = 0; c < 16; ++c) v[c] = ldsd[17 * t + c];

            // ---- pass B: radix-16 over c; slot s holds q' = rev16(s): bin k = 64 q' + t
            fft16_sel(v);

#pragma unroll
            for (int u = 0; u < 16; ++u) {
                if (u == 15) {      // bin N-1 (lane 63) also feeds the DC slot, weight K - kf
                    const double pw = fma(v[u].y, v[u].y, v[u].x * v[u].x);
                    acc[u] = KONE ? pw : acc[u] + pw;
                    wdc = KONE ? pw : fma((double)(K - kf), pw, wdc);
                } else if constexpr (KONE) {
                    acc[u] = fma(v[u].y, v[u].y, v[u].x * v[u].x);
                } else {
                    acc[u] = fma(v[u].y, v[u].y, fma(v[u].x, v[u].x, acc[u]));
                }
            }
        }

        // ---- DC-slot rule (src/spectrum.c:25-33): slot N/2 (bin 0: lane 0, u = 0) takes
        // sum_k (K-k) * P_k[N-1] (bin N-1: lane 63, u = 15)
        // (two v_readlane + two v_writelane: lane 0's halves of acc[0] replaced in place)
        {
            const unsigned long long w = __builtin_bit_cast(unsigned long long, wdc);
            const unsigned long long a0 = __builtin_bit_cast(unsigned long long, acc[0]);
            const unsigned lo = rtlws_writelane(__builtin_amdgcn_readlane((int)(unsigned)w, 63), 0, (int)(unsigned)a0);
            const unsigned hi = rtlws_writelane(__builtin_amdgcn_readlane((int)(unsigned)(w >> 32), 63), 0, (int)(unsigned)(a0 >> 32));
            acc[0] = __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
        }

        // ---- epilogue + store: slot u holds bin 64 q' + t, q' = rev16(u); fft-shift = flip the top
        // bit of the bin index = q' ^ 8.
        // Every store instruction writes 64 consecutive outputs, one per lane.  (Measured and not kept:
        // the row staged through the idle transposition buffer so that a lane stores 16 bytes -- 111.2 us
        // against 109.3 for these 4-byte-per-lane stores; profiles/r04_x1024_store_ab.txt.)
        {
            constexpr unsigned ELEM = OUT == OUT_PAYLOAD ? 1 : ROWF32 ? 4 : 8;             // bytes per output
            char* base = reinterpret_cast<char*>(p.out) + g * (long)(N * ELEM);        // uniform (as in load_raw)
            char* base_hi = base + 4096;            // f64 rows are 8 KiB and a store's immediate ends at 4 095: a second base
            asm("" : "+s"(base), "+s"(base_hi), "+v"(lane_out));
            RTLWS_GLOBAL char* const row = (RTLWS_GLOBAL char*)(base + lane_out);
            RTLWS_GLOBAL char* const row_hi = (RTLWS_GLOBAL char*)(base_hi + lane_out);
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const unsigned off = 64 * ELEM * (rev16(u) ^ 8);           // a constant once unrolled
                RTLWS_GLOBAL char* const dst = (off < 4096 ? row : row_hi) + (off & 4095);
                const double a = acc[u];
                if constexpr (OUT == OUT_PAYLOAD) {
                    *(RTLWS_GLOBAL uint8_t*)dst = (uint8_t)payload_f64(p.lin_gain * a, p.count);
                } else {
                    const double o = (OUT == OUT_DB) ? db_f64(a, p.count) : a;
                    if constexpr (ROWF32) __builtin_nontemporal_store((float)o, (RTLWS_GLOBAL float*)dst);
                    else __builtin_nontemporal_store(o, (RTLWS_GLOBAL double*)dst);
                }
            }
        }
        g = g_next;
    }
}

// LDS: one 16 x 17 x 64-byte transposition slice per wavefront (+ the row counter)
constexpr size_t x_lds_bytes(int waves) { return (size_t)waves * 16 * 17 * 64 + (waves > 1 ? 16 : 0); }
size_t spectra_f64_1024x_lds_bytes(int waves) { return x_lds_bytes(waves >= 8 ? 8 : 1); }

// leaf(kernel, threads, dynamic LDS bytes) for the instantiation the fields select (pick) or for each one the
// launcher can reach (visit_all).  waves = 1: one-wavefront workgroups; waves = 8: workgroups of eight wavefronts
// (one per CU), 136 KiB of LDS.
template <typename Choose, typename Leaf>
static hipError_t x_table(Choose choose, const SpectraParamsF64& p, int waves, Leaf&& leaf)
{
    return choose(Vals<1, 8>{}, waves >= 8 ? 8 : 1, [&](auto w) {
        return choose(OutModes{}, p.out_mode, [&](auto out) {
            // K-frame accumulators beside the dB / payload epilogues: spectrum_f64_fused.hip
            using Kone = std::conditional_t<out == OUT_SUM, Bools, Vals<true>>;
            return choose(Kone{}, p.k_avg == 1, [&](auto kone) {
                return choose(Flag<out != OUT_PAYLOAD>{}, p.rows_f32 != 0, [&](auto rowf32) {
                    return leaf(&spectra_f64_1024x<out, kone, rowf32, w>, 64 * w, x_lds_bytes(w));
                });
            });
        });
    });
}

hipError_t launch_spectra_f64_1024x(const SpectraParamsF64& p, int blocks, int waves, hipStream_t st, int device)
{
    return x_table(pick, p, waves, [&](auto kernel, int threads, size_t lds_bytes) {
        const hipError_t e = lds_opt_in(kernel, device, lds_bytes);
        return e != hipSuccess ? e : launch(kernel, dim3(blocks), dim3(threads), lds_bytes, st, p);
    });
}

hipError_t prepare_spectra_f64_1024x(int device)
{
    return x_table(visit_all, SpectraParamsF64{}, 0, [&](auto kernel, int, size_t lds_bytes) {
        return lds_opt_in(kernel, device, lds_bytes);
    });
}

}  // namespace rtlws
