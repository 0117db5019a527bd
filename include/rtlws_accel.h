/*
 * rtlws_accel.h -- acceleration search: the long-frame periodicity search of rtlws_periodlong.h over every series read
 * through a table of quadratic index maps, one virtual trial per (trial, acceleration), with no resampled copy in
 * memory (librtlws_accel.so).  A pulsar in a binary drifts by a T^2 / (8 c) samples at the middle of a frame of T
 * samples; resampling the series along the drift gives its harmonics back to single bins (DESIGN.md 4.24;
 * tests/accel_ref.py restates the map and the search in numpy).
 *
 * The map, every bit defined in integers.  L = nsamp - 1; a coefficient c is an int64, |c| <= 2^40, in units of 2^-64
 * samples per sample^2:
 *   s_c(n) = floor((c n (L - n) + 2^63) / 2^64)    -- exact integers, the floor towards -Inf: a half goes up for either
 *                                                      sign of c (rtlws_accel_shift)
 *   f_c(n) = n + s_c(n)
 *   R_c[n] = D[f_c(n)],  n = 0 .. nsamp-1           -- a copy of a sample: nothing is rounded
 * A positive c reads later samples at mid-frame (f_c(n) >= n).  With |c| <= 2^40 and nsamp <= 2^22 the slope of
 * n + c 2^-64 n (L - n) lies in [3/4, 5/4]: f_c(0) = 0, f_c(L) = L, f_c does not decrease and stays in 0 .. nsamp-1, so
 * a run reads samples 0 .. nsamp-1 of a trial and nothing else, with no clamp (DESIGN.md 4.24 proves it).
 *
 *   D[t][n]   f32 on the device, trial t at d_in + t * in_stride; t = 0 .. ntrials-1, n = 0 .. nsamp-1, nsamp 1 .. N
 *   coefs     naccel 1 .. 1024 coefficients, in any order, duplicates allowed
 *   log2n, levels, norm, seg, klo    rtlws_periodlong.h's plan parameters, with its limits
 *
 * rtlws_accel_search: virtual trial v = t * naccel + a is the search of R_{coefs[a]} of trial t.  Every word it writes
 * for v has the bits that rtlws_periodlong_run, under the same plan parameters, writes for the series that
 * rtlws_accel_resample gives for (t, a): d_best, d_at, d_power and d_white in rtlws_periodlong_run's layout with v in
 * place of t.  With coefficient 0 that is rtlws_periodlong_run on the source itself.  Only the mean and the columns of
 * the six stages read the input; they read it through the map, the four stages behind them are rtlws_periodlong.h's.
 * The stage-1 bound of rtlws_periodlong.h holds for R as it does for any series (its premises are R's).
 *
 * Refused with -1, 0 or NULL (rtlws_accel_last_error() says why): what rtlws_periodlong.h refuses, naccel outside
 * 1 .. 1024, a NULL table, a coefficient beyond +-2^40, ntrials * naccel above 65536, out_stride below nsamp or not a
 * multiple of 4, d_out not 16-byte aligned, a_count below 1, a_first below 0, a_first + a_count above naccel.
 *
 * Not built: frames below 2^16 samples (the drift of a physical acceleration is a fraction of a sample there), jerk
 * terms, a Fourier-domain correlation search, interpolating resamplers (this one copies samples: that keeps it
 * bit-defined).
 */
#ifndef RTLWS_ACCEL_H
#define RTLWS_ACCEL_H

#include <stddef.h>
#include <stdint.h>

#include "rtlws_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* librtlws_accel.so exports these declarations and nothing else (exports/accel.map) */
#pragma GCC visibility push(default)

#define RTLWS_ACCEL_MAX_NACCEL 1024
/* the largest |coefficient|: 2^40 */
#define RTLWS_ACCEL_MAX_COEF ((int64_t)1 << 40)
/* the most virtual trials ntrials * naccel of a run */
#define RTLWS_ACCEL_MAX_VIRTUAL 65536
/* the launches of a group of virtual trials: rtlws_periodlong.h's stages */
#define RTLWS_ACCEL_STAGES 6

typedef struct rtlws_accel_plan rtlws_accel_plan;

/* 1 when the plan is served, else 0 (rtlws_accel_last_error() says why).  The rules in this order: log2n, levels, norm,
 * seg, klo (rtlws_periodlong.h's), naccel, a NULL table, the coefficients in the table's order.  Needs no GPU. */
int rtlws_accel_supported(int log2n, int levels, int norm, int seg, int klo, int naccel, const int64_t* coefs);

/* What a plan launches for ntrials trials, stage by stage (RTLWS_ACCEL_STAGES entries each): workgroups over all
 * ntrials * naccel virtual trials, threads per workgroup, bytes of LDS per workgroup; and nseg = M / seg.  Any of the
 * four pointers may be NULL.  0, or -1 when the plan is not served or ntrials is outside 1 .. 65536 or ntrials * naccel
 * above 65536 (the plan's rules first, then ntrials).  Needs no GPU. */
int rtlws_accel_geometry(int log2n, int levels, int norm, int seg, int klo, int naccel, const int64_t* coefs, int ntrials, int* blocks,
                         int* threads, int* lds_bytes, int* nseg);

/* rtlws_periodlong.h's tables, the table of coefficients (copied from the host's `coefs`) and a workspace of 12 M + 512
 * bytes per virtual trial in flight on the engine's device, the kernels loaded, so that the runs only enqueue kernels
 * and may be captured into a hipGraph.  max_trials >= 1 counts virtual trials: the workspace holds min(max_trials, what
 * fits under RTLWS_PERIODLONG_WORKSPACE_CAP) of them, and larger batches still run, in groups; a group's border may
 * fall inside a trial's accelerations.  The rules in this order: the plan's as above, max_trials, the engine.  NULL on
 * failure (a null engine among them: without a device there is no engine, and no CPU path). */
rtlws_accel_plan* rtlws_accel_open(rtlws_engine* e, int log2n, int levels, int norm, int seg, int klo, int naccel, const int64_t* coefs,
                                   int max_trials);

/* Bytes of device memory the plan's workspace occupies (0 for NULL). */
size_t rtlws_accel_workspace_bytes(const rtlws_accel_plan* p);

/* The fused search.  d_in: ntrials series of nsamp f32, in_stride apart, 16-byte aligned; d_best, d_at: ntrials * naccel
 * * levels * nseg f32 and int32; d_power, d_white: ntrials * naccel * M f32 each, or NULL: not written.  Asynchronous on
 * `stream` (NULL = the engine's own stream, RTLWS_STREAM_DEFAULT = HIP's: "Streams" in rtlws_hip.h); kernel launches, six
 * a group of virtual trials, and no other runtime call.  Runs of one plan share its workspace: they must be ordered (one
 * stream, or events).  Every refusal is made before the device is asked for anything, in this order: ntrials
 * (1 .. 65536), nsamp (1 .. 4194304), in_stride at least nsamp and a multiple of 4, null pointers (d_in, d_best, d_at),
 * the alignments of d_in, d_best, d_at, d_power and d_white, then a null plan, then what the plan decides (ntrials *
 * naccel at most 65536, nsamp at most N).
 * 0; -1 bad argument; -3 HIP failure. */
int rtlws_accel_search(rtlws_accel_plan* p, const float* d_in, long in_stride, int ntrials, int nsamp, float* d_best, int32_t* d_at,
                       float* d_power, float* d_white, void* stream);

/* The materialised series, for the few candidates that go on to rtlws_fold_run: R of accelerations a_first .. a_first +
 * a_count - 1 of every trial, that of (t, a) at d_out + (t * a_count + (a - a_first)) * out_stride -- the layout
 * rtlws_fold_run and rtlws_periodlong_run read.  One launch; it writes elements 0 .. nsamp-1 of a row and nothing else.
 * Every refusal is made before the device is asked for anything, in this order: ntrials (1 .. 65536), nsamp
 * (1 .. 4194304), in_stride at least nsamp and a multiple of 4, out_stride at least nsamp and a multiple of 4, a_count
 * at least 1, a_first at least 0, a_first + a_count at most 1024, null pointers (d_in, d_out), the alignments of d_in and
 * d_out (16 bytes), then a null plan, then what the plan decides (a_first + a_count at most naccel, ntrials * a_count
 * at most 65536, nsamp at most N).
 * 0; -1 bad argument; -3 HIP failure. */
int rtlws_accel_resample(rtlws_accel_plan* p, const float* d_in, long in_stride, int ntrials, int nsamp, int a_first, int a_count,
                         float* d_out, long out_stride, void* stream);

/* The coefficient of a line-of-sight acceleration in m/s^2 at a sampling interval in seconds: the integer nearest
 * accel * tsamp / (2 * 299792458) * 2^64, exactly (a half away from zero).  Positive: the map reads later samples at
 * mid-frame.  0 with the error text set for a non-finite argument or a result beyond +-2^40.  Needs no GPU. */
int64_t rtlws_accel_coef(double accel_m_s2, double tsamp_s);

/* The coefficient whose shift at mid-frame is mid_shift_samples: the integer nearest shift * 4 / (nsamp - 1)^2 * 2^64,
 * exactly (a half away from zero); what one chooses the spacing of the table with.  0 with the error text set for a
 * non-finite shift, nsamp outside 2 .. 4194304 or a result beyond +-2^40.  Needs no GPU. */
int64_t rtlws_accel_coef_from_shift(double mid_shift_samples, int nsamp);

/* s_c(n), exactly.  0 with the error text set where |coef| is beyond 2^40, nsamp outside 1 .. 4194304 or n outside
 * 0 .. nsamp-1.  Needs no GPU. */
long rtlws_accel_shift(int64_t coef, int nsamp, int n);

/* Frees the tables and the workspace (after the caller has synchronised the streams it ran on). */
void rtlws_accel_close(rtlws_accel_plan* p);

/* Last error text of the calling thread from this library ("" when none). */
const char* rtlws_accel_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* RTLWS_ACCEL_H */
