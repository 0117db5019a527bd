/*
 * rtlws_periodlong.h -- the periodicity search of rtlws_period.h for long series: frames of 2^16 .. 2^22 samples, the
 * transform a four-step one through device memory (librtlws_periodlong.so).  The same four stages, the same output
 * layout and, from the power spectrum on, the same bits as rtlws_period.h defines.
 *
 * rtlws_dedisp_run (rtlws_dedisp.h) leaves ntrials f32 series on the device; this library reads them where they lie and
 * names the periods that rtlws_fold_run (rtlws_fold.h) then folds at (tests/periodlong_ref.py and
 * tests/period_ref.py restate it in numpy).
 *
 *   D[t][n]   f32 on the device, trial t at d_in + t * in_stride; t = 0 .. ntrials-1, n = 0 .. nsamp-1, nsamp 1 .. N
 *   log2n     16 .. 22: N = 2^log2n samples of a frame, M = N / 2 bins
 *   levels    1 .. 5: level l = 0 .. levels-1 adds H = 2^l harmonics
 *   norm      a power of two 16 .. 16384: the whitening block, in bins
 *   seg       a power of two 64 .. 16384: the length of a peak segment; nseg = M / seg
 *   klo       1 .. M-1: bins below it take no part in the peaks
 * The caps on norm and seg are rtlws_period.h's own largest values: one workgroup owns whole blocks and segments.
 *
 * Stage 1, held within a bound (DESIGN.md 4.23 derives it):
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
 *   (rtlws_periodlong_samples).  Every index is <= k.
 * Stage 4, the peaks:  for every trial t, level l, segment s, over the k of [s seg, (s+1) seg) that are >= klo, ascending:
 *   best = -Inf, at = -1;  S_l[k] is taken if S_l[k] > best  -- strict: ties go to the smaller k, a NaN is never taken,
 *   and a segment wholly below klo gives (-Inf, -1).
 *
 * The run reads samples 0 .. nsamp - 1 of every trial and nothing else: nothing in the stride's padding, nothing at or
 * behind nsamp.  It writes d_best[(t levels + l) nseg + s] (f32), d_at[the same] (int32: M <= 2^21), and where they are
 * not NULL d_power[t M + k] = P and d_white[t M + k] = W (the index a long: 65536 * 2^21 does not fit an int), and
 * nothing else of the caller's; best and at have the same bits with and without the optional rows.  Strides are in
 * elements.  The input layout is what rtlws_dedisp_run writes when out_stride is a multiple of 4.  A trial with a
 * non-finite sample has unspecified rows, and the peaks the rule gives on them; every other trial is untouched.
 *
 * M = M1 M2 complex points, M1 = 16 (log2n <= 19) or 256, M2 = 2^11 .. 2^14.  Six launches a group of trials: the
 * mean's partial sums, the M1-point transforms with the twist, the M2-point rows in LDS, the untangling and the square,
 * the whitening, the harmonic sums and peaks.  Between them a trial lies in the plan's workspace, 12 M + 512 bytes.
 * rtlws_periodlong_geometry says what a plan launches.
 *
 * Refused with -1 or NULL (rtlws_periodlong_last_error() says why): log2n outside 16 .. 22, levels outside 1 .. 5, norm
 * not a power of two 16 .. 16384, seg not a power of two 64 .. 16384, klo outside 1 .. M-1, max_trials below 1, ntrials
 * outside 1 .. 65536, nsamp outside 1 .. N, in_stride below nsamp or not a multiple of 4, null pointers, d_in not
 * 16-byte aligned, an output not 4-byte aligned.
 *
 * The false-alarm probability of a sum is rtlws_period_lnq (rtlws_period.h): it does not depend on the frame length and
 * is not repeated here.
 *
 * Not built: frames of other than a power of two samples, median whitening, interbinning.  (Acceleration search is
 * rtlws_accel.h's, on top of this library's stages.)
 */
#ifndef RTLWS_PERIODLONG_H
#define RTLWS_PERIODLONG_H

#include <stddef.h>
#include <stdint.h>

#include "rtlws_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* librtlws_periodlong.so exports these declarations and nothing else (exports/periodlong.map) */
#pragma GCC visibility push(default)

#define RTLWS_PERIODLONG_MIN_LOG2N 16
#define RTLWS_PERIODLONG_MAX_LOG2N 22
#define RTLWS_PERIODLONG_MAX_LEVELS 5
#define RTLWS_PERIODLONG_MIN_NORM 16
#define RTLWS_PERIODLONG_MAX_NORM 16384
#define RTLWS_PERIODLONG_MIN_SEG 64
#define RTLWS_PERIODLONG_MAX_SEG 16384
#define RTLWS_PERIODLONG_MAX_TRIALS 65536
/* the launches of a group of trials, in this order: mean, columns, rows, untangling, whitening, peaks */
#define RTLWS_PERIODLONG_STAGES 6

/* The workspace of a plan holds 12 M + 512 bytes per trial in flight.  It is capped at this many bytes -- or at one
 * trial's, which is less at every frame length: a batch of more trials than the workspace holds is run as consecutive
 * groups on the stream. */
#define RTLWS_PERIODLONG_WORKSPACE_CAP ((size_t)1 << 30)

typedef struct rtlws_periodlong_plan rtlws_periodlong_plan;

/* 1 when the plan is served, else 0 (rtlws_periodlong_last_error() says why).  The rules in this order: log2n, levels,
 * norm, seg, klo.  Needs no GPU. */
int rtlws_periodlong_supported(int log2n, int levels, int norm, int seg, int klo);

/* What a plan launches for ntrials trials, stage by stage (RTLWS_PERIODLONG_STAGES entries each): workgroups over all
 * trials, threads per workgroup, bytes of LDS per workgroup; and nseg = M / seg.  Any of the pointers may be NULL.
 * 0, or -1 when the plan is not served or ntrials is outside its range (the plan's rules first, then ntrials).  Needs
 * no GPU. */
int rtlws_periodlong_geometry(int log2n, int levels, int norm, int seg, int klo, int ntrials, int* blocks, int* threads,
                              int* lds_bytes, int* nseg);

/* The tables and the workspace on the engine's device and the kernels loaded, so that rtlws_periodlong_run only
 * enqueues kernels and may be captured into a hipGraph.  max_trials >= 1 is the largest batch the caller expects: the
 * workspace holds min(max_trials, what fits under RTLWS_PERIODLONG_WORKSPACE_CAP) trials in flight, and larger batches
 * still run, in groups.  The rules in this order: the plan's as above, max_trials, the engine.  NULL on failure (a null
 * engine among them: without a device there is no engine, and no CPU path). */
rtlws_periodlong_plan* rtlws_periodlong_open(rtlws_engine* e, int log2n, int levels, int norm, int seg, int klo, int max_trials);

/* Bytes of device memory the plan's workspace occupies (0 for NULL). */
size_t rtlws_periodlong_workspace_bytes(const rtlws_periodlong_plan* p);

/* d_in: ntrials series of nsamp f32, in_stride apart, 16-byte aligned; d_best, d_at: ntrials * levels * nseg f32 and
 * int32; d_power, d_white: ntrials * M f32 each, or NULL: not written.  Asynchronous on `stream` (NULL = the engine's own
 * stream, RTLWS_STREAM_DEFAULT = HIP's: "Streams" in rtlws_hip.h); kernel launches, six a group of trials, and no other
 * runtime call.  Runs of one plan share its workspace: they must be ordered (one stream, or events).  Every refusal is
 * made before the device is asked for anything, in this order: ntrials, nsamp (1 .. 4194304), in_stride at least nsamp
 * and a multiple of 4, null pointers (d_in, d_best, d_at), the alignments of d_in, d_best, d_at, d_power and d_white,
 * then a null plan, then what the plan decides (nsamp at most N).
 * 0; -1 bad argument; -3 HIP failure. */
int rtlws_periodlong_run(rtlws_periodlong_plan* p, const float* d_in, long in_stride, int ntrials, int nsamp, float* d_best,
                         int32_t* d_at, float* d_power, float* d_white, void* stream);

/* The fundamental's period in samples of bin k at level `level`: N 2^level / k as a double, exact up to the one
 * division; what rtlws_fold_step takes.  0 with the error text set where log2n is outside 16 .. 22, level outside 0 .. 4
 * or k outside 1 .. M-1.  Needs no GPU. */
double rtlws_periodlong_samples(int log2n, int level, int k);

/* Frees the tables and the workspace (after the caller has synchronised the streams it ran on). */
void rtlws_periodlong_close(rtlws_periodlong_plan* p);

/* Last error text of the calling thread from this library ("" when none). */
const char* rtlws_periodlong_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* RTLWS_PERIODLONG_H */
