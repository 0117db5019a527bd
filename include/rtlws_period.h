/*
 * rtlws_period.h -- periodicity search over dedispersed time series: every trial's series is transformed, its power
 * spectrum whitened, harmonics 1 .. 2^l added for every level l, and the largest sums of every stretch of the frequency
 * axis reported, all trials in one launch (librtlws_period.so).
 *
 * rtlws_dedisp_run (rtlws_dedisp.h) leaves ntrials f32 series on the device; this library reads them where they lie and
 * names the periods that rtlws_fold_run (rtlws_fold.h) then folds at (tests/period_ref.py restates it in
 * numpy).
 *
 *   D[t][n]   f32 on the device, trial t at d_in + t * in_stride; t = 0 .. ntrials-1, n = 0 .. nsamp-1, nsamp 1 .. N
 *   log2n     10 .. 15: N = 2^log2n samples of a frame, M = N / 2 bins
 *   levels    1 .. 5: level l = 0 .. levels-1 adds H = 2^l harmonics
 *   norm      a power of two 16 .. M: the whitening block, in bins
 *   seg       a power of two 64 .. M: the length of a peak segment; nseg = M / seg
 *   klo       1 .. M-1: bins below it take no part in the peaks
 *
 * Stage 1, held within a bound (DESIGN.md 4.22 derives it):
 *   mu_t = the mean of the trial's nsamp samples, accumulated in f64 (in any order)
 *   y[n] = (float)((double)D[t][n] - mu_t) for n < nsamp, 0 for nsamp <= n < N     -- the mean removed, then zeros
 *   X    = the N-point DFT of y in f32 arithmetic;  P[k] = |X[k]|^2, k = 0 .. M-1  -- the Nyquist bin is dropped
 * Stage 2, every bit defined from P:  block b is bins b norm .. (b+1) norm - 1;
 *   sum_b  = the balanced halving tree over the block: adjacent pairs first, one f32 rounding per addition
 *   mean_b = fl(sum_b * 2^-log2(norm));   W[k] = fl(P[k] / mean_b), the IEEE division; 0 / 0 is NaN
 * Stage 3, every bit defined from W:  for every k:  acc = W[k];  S_0[k] = acc;
 *   for l = 1 .. levels-1:  for odd h = 1, 3, .. 2^l - 1 ascending:  acc = fl(acc + W[(k h + 2^(l-1)) >> l]);  S_l[k] = acc
 *   -- S_l[k] is the sum over h = 1 .. H of W[floor(k h / H + 1/2)], H = 2^l: the even harmonics of level l are level
 *   l - 1's terms at the same k.  k is the bin of the highest harmonic: the fundamental's period is N 2^l / k samples
 *   (rtlws_period_samples).  Every index is <= k.
 * Stage 4, the peaks:  for every trial t, level l, segment s, over the k of [s seg, (s+1) seg) that are >= klo, ascending:
 *   best = -Inf, at = -1;  S_l[k] is taken if S_l[k] > best  -- strict: ties go to the smaller k, a NaN is never taken,
 *   and a segment wholly below klo gives (-Inf, -1).
 *
 * The run reads samples 0 .. nsamp - 1 of every trial and nothing else: nothing in the stride's padding, nothing at or
 * behind nsamp.  It writes d_best[(t levels + l) nseg + s] (f32), d_at[the same] (int32), and where they are not NULL
 * d_power[t M + k] = P and d_white[t M + k] = W, and nothing else; best and at have the same bits with and without the
 * optional rows.  Strides are in elements.  The input layout is what rtlws_dedisp_run writes when out_stride is a
 * multiple of 4.  A trial with a non-finite sample has unspecified rows, and the peaks the rule gives on them; every other
 * trial is untouched.
 *
 * One workgroup owns one trial, max(64, M / 16) threads and 17 M / 2 bytes of LDS (136 KiB at log2n 15); the series stays
 * in LDS from the load to the peaks.  rtlws_period_geometry says what a plan launches.
 *
 * Refused with -1 or NULL (rtlws_period_last_error() says why): log2n outside 10 .. 15, levels outside 1 .. 5, norm not
 * a power of two 16 .. M, seg not a power of two 64 .. M, klo outside 1 .. M-1, ntrials outside 1 .. 65536, nsamp
 * outside 1 .. N, in_stride below nsamp or not a multiple of 4, null pointers, d_in not 16-byte aligned, an output not
 * 4-byte aligned.
 *
 * Not built: frames above 2^15 samples (a four-step transform through device memory), median whitening, interbinning,
 * acceleration search.
 */
#ifndef RTLWS_PERIOD_H
#define RTLWS_PERIOD_H

#include <stdint.h>

#include "rtlws_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* librtlws_period.so exports these declarations and nothing else (exports/period.map) */
#pragma GCC visibility push(default)

#define RTLWS_PERIOD_MIN_LOG2N 10
#define RTLWS_PERIOD_MAX_LOG2N 15
#define RTLWS_PERIOD_MAX_LEVELS 5
#define RTLWS_PERIOD_MIN_NORM 16
#define RTLWS_PERIOD_MIN_SEG 64
#define RTLWS_PERIOD_MAX_TRIALS 65536

typedef struct rtlws_period_plan rtlws_period_plan;

/* 1 when the plan is served, else 0 (rtlws_period_last_error() says why).  The rules in this order: log2n, levels, norm,
 * seg, klo.  Needs no GPU. */
int rtlws_period_supported(int log2n, int levels, int norm, int seg, int klo);

/* What a plan launches for ntrials trials: workgroups (ntrials), threads per workgroup (max(64, M / 16)), bytes of LDS
 * per workgroup (17 M / 2) and nseg = M / seg.  Any of the pointers may be NULL.  0, or -1 when the plan is not served
 * or ntrials is outside its range (the plan's rules first, then ntrials).  Needs no GPU. */
int rtlws_period_geometry(int log2n, int levels, int norm, int seg, int klo, int ntrials, int* blocks, int* threads, int* lds_bytes,
                          int* nseg);

/* The transform's table on the engine's device and the kernel loaded, so that rtlws_period_run makes no runtime call
 * other than its launch and may be captured into a hipGraph.  NULL on failure (a null engine among them: without a
 * device there is no engine, and no CPU path). */
rtlws_period_plan* rtlws_period_open(rtlws_engine* e, int log2n, int levels, int norm, int seg, int klo);

/* d_in: ntrials series of nsamp f32, in_stride apart, 16-byte aligned; d_best, d_at: ntrials * levels * nseg f32 and
 * int32; d_power, d_white: ntrials * M f32 each, or NULL: not written.  Asynchronous on `stream` (NULL = the engine's own
 * stream, RTLWS_STREAM_DEFAULT = HIP's: "Streams" in rtlws_hip.h); one kernel launch and no other runtime call.  Every
 * refusal is made before the device is asked for anything, in this order: ntrials, nsamp (1 .. 32768), in_stride at
 * least nsamp and a multiple of 4, null pointers (d_in, d_best, d_at), the alignments of d_in, d_best, d_at, d_power
 * and d_white, then a null plan, then what the plan decides (nsamp at most N).
 * 0; -1 bad argument; -3 HIP failure. */
int rtlws_period_run(rtlws_period_plan* p, const float* d_in, long in_stride, int ntrials, int nsamp, float* d_best, int32_t* d_at,
                     float* d_power, float* d_white, void* stream);

/* The fundamental's period in samples of bin k at level `level`: N 2^level / k as a double, exact up to the one
 * division; what rtlws_fold_step takes.  0 with the error text set where log2n is outside 10 .. 15, level outside 0 .. 4
 * or k outside 1 .. M-1.  Needs no GPU. */
double rtlws_period_samples(int log2n, int level, int k);

/* The natural logarithm of the false-alarm probability of a sum S of H whitened powers over exponential noise,
 * ln(e^-S sum_{j<H} S^j / j!), in double through a log-sum-exp (S = 500 does not underflow), never above 0.  0 for S <= 0; NaN for H
 * outside 1 .. 16 or S not finite.  Needs no GPU. */
double rtlws_period_lnq(double S, int H);

void rtlws_period_close(rtlws_period_plan* p);

/* Last error text of the calling thread from this library ("" when none). */
const char* rtlws_period_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* RTLWS_PERIOD_H */
