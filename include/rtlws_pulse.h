/*
 * rtlws_pulse.h -- single-pulse search over dedispersed time series: every trial's series is filtered with boxcars of
 * a ladder of widths, and for every segment of the series the largest filtered value, where it lies and the first two
 * moments of the samples come back, all trials and widths in one launch (librtlws_pulse.so).
 *
 * rtlws_dedisp_run (rtlws_dedisp.h) leaves ntrials f32 series on the device; this library reads them where they lie
 * (tests/pulse_ref.py restates it in numpy).
 *
 *   D[t][n]   f32 on the device, trial t at d_in + t * in_stride; t = 0 .. ntrials-1
 *   w_k       widths, k = 0 .. nwidths-1: int32 table in host memory at open, strictly ascending, 1 .. 1024; nwidths 1 .. 16
 *   seg       outputs per segment: 64 .. 1048576, a multiple of 4 (the plan's)
 *   nout      outputs per trial and width, 0 .. 2^30; nseg = ceil(nout / seg)
 *
 *   P_0[n]     = D[t][n]
 *   P_(l+1)[n] = fl(P_l[n] + P_l[n + 2^l])                  (one f32 rounding)
 *
 *   w = 2^a1 + 2^a2 + .. + 2^am,  a1 > a2 > .. > am:
 *   B_w[n] = fl(..fl(fl(P_a1[n] + P_a2[n + 2^a1]) + P_a3[n + 2^a1 + 2^a2]) ..)     (m = 1: B_w[n] = P_a1[n])
 *
 *   peak[t][k][s], at[t][k][s]:  best = -Inf; at = -1;
 *         for n = s*seg .. min((s+1)*seg, nout) - 1 ascending:  if B_wk[n] > best: best = B_wk[n]; at = n
 *   mom[t][s][0..1]:  x_j = (double) D[t][s*seg + j], j = 0 .. len-1 (len = this segment's outputs)
 *         q1[r] = sum of x_j, q2[r] = sum of x_j * x_j  over j == r (mod 256), ascending j, f64 from +0.0, r = 0 .. 255
 *         for h = 128, 64, .., 1:  q[i] = q[i] + q[i + h], i < h;     mom = (q1[0], q2[0])
 *
 * B_w[n] is the sum of D[t][n .. n + w - 1] in a fixed balanced order that depends on w alone -- not on n, nout, seg,
 * the trial, the grid or the tile -- and no atomics take part: two runs give the same bits, a run over the samples from
 * n0 on gives B of the whole run from n0 on bit for bit, and where n0 is a multiple of seg the same peaks with `at`
 * shifted by n0.  Against the f64 sum, |B_w - sum| <= depth 2^-24 sum|terms|, depth = floor(log2 w) + popcount(w) - 1.
 * The comparison of the peak is strict: NaN never wins, among equal values (+0.0 and -0.0 are equal) the least n wins
 * with its own bits, and a segment with nothing above -Inf gives (-Inf, -1).  A product of two f32 is exact in f64, so
 * the residue classes and the halving tree define every bit of the moments.  Maximising B over n at fixed (t, k) is
 * maximising rtlws_pulse_snr, which is why the run needs no statistics to find the peak.
 *
 * The run reads samples 0 .. nout + w_max - 2 of every trial (rtlws_pulse_samples_needed; 0 for nout = 0), nothing at
 * or beyond that index and nothing in the stride's padding.  It writes d_peak[(t * nwidths + k) * nseg + s] (f32),
 * d_at in the same layout (int32) and d_mom[(t * nseg + s) * 2 + {0, 1}] (f64; d_mom may be NULL: no moments are
 * computed or written), and nothing else.  Strides are in elements.  The input layout is what rtlws_dedisp_run writes
 * when out_stride is a multiple of 4: the two libraries chain on the device with no copy.
 *
 * A workgroup of 256 threads owns one segment of one trial (the grid is ntrials * nseg) and walks it in tiles of
 * tile_out outputs.  A tile's samples and their sums over 2^l are rows of LDS, each roundup4(tile_out + w_max - 1) f32:
 * one row for every level that the binary form of some width uses (levels_kept of them), and for the levels in between
 * at most two more, used in turn.  tile_out is the largest of 1024, 512, 256 whose rows fit in 64 KiB, and lds_bytes
 * the smallest of 16, 32, 64 KiB that holds them; every table within the limits is served (the rows of {.., 1023, 1024}
 * take 55 KiB at tile_out 256), what a table costs is speed.  rtlws_pulse_geometry says what a table gets.
 *
 * Refused with -1 (rtlws_pulse_last_error() says why): nwidths outside 1 .. 16, a null table, a width outside
 * 1 .. 1024 or not above the one before, seg outside 64 .. 1048576 or not a multiple of 4, ntrials outside 1 .. 65536,
 * nout outside 0 .. 2^30, in_stride below samples_needed or not a multiple of 4, null pointers, d_in not 16-byte
 * aligned, d_peak or d_at not 4-byte aligned, d_mom not 8-byte aligned, more workgroups than one grid holds.
 */
#ifndef RTLWS_PULSE_H
#define RTLWS_PULSE_H

#include <stdint.h>

#include "rtlws_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* librtlws_pulse.so exports these declarations and nothing else (exports/pulse.map) */
#pragma GCC visibility push(default)

#define RTLWS_PULSE_MAX_WIDTHS 16
#define RTLWS_PULSE_MAX_WIDTH 1024
#define RTLWS_PULSE_MIN_SEG 64
#define RTLWS_PULSE_MAX_SEG 1048576
#define RTLWS_PULSE_MAX_TRIALS 65536
#define RTLWS_PULSE_MAX_NOUT 1073741824

typedef struct rtlws_pulse_plan rtlws_pulse_plan;

/* 1 when the table and the segment length are served, else 0 (rtlws_pulse_last_error() says why).  Needs no GPU. */
int rtlws_pulse_supported(int nwidths, const int32_t* widths, long seg);

/* What a plan of this table launches for nout outputs of each of ntrials trials: workgroups (ntrials * nseg), threads
 * per workgroup (256), bytes of LDS per workgroup, outputs per tile, the number of distinct bits set over the table,
 * and nseg = ceil(nout / seg).  Any of the pointers behind nout may be NULL.  0, or -1 when the table or seg is not
 * served, ntrials or nout is outside its range or the grid does not hold the workgroups.  Needs no GPU. */
int rtlws_pulse_geometry(int nwidths, const int32_t* widths, long seg, int ntrials, long nout, int* blocks, int* threads,
                         int* lds_bytes, int* tile_out, int* levels_kept, long* nseg);

/* The table (nwidths int32 in host memory, read before the call returns) on the engine's device in the kernel's form,
 * and the kernel loaded, so that rtlws_pulse_run makes no runtime call other than its launch and may be captured into a
 * hipGraph.  A new table or seg is a new plan.  NULL on failure (a null engine among them: without a device there is
 * no engine, and no CPU path). */
rtlws_pulse_plan* rtlws_pulse_open(rtlws_engine* e, int nwidths, const int32_t* widths, long seg);

/* Samples of a trial that nout outputs read: nout + w_max - 1, 0 for nout == 0; -1 for a null plan or nout outside
 * 0 .. 2^30. */
long rtlws_pulse_samples_needed(const rtlws_pulse_plan* p, long nout);

/* ceil(nout / seg); -1 for a null plan or nout outside 0 .. 2^30. */
long rtlws_pulse_segments(const rtlws_pulse_plan* p, long nout);

/* d_in: ntrials series of rtlws_pulse_samples_needed() f32, in_stride apart, 16-byte aligned; d_peak and d_at:
 * ntrials * nwidths * nseg f32 and int32; d_mom: ntrials * nseg * 2 f64, or NULL.  Asynchronous on `stream` (NULL = the
 * engine's own stream, RTLWS_STREAM_DEFAULT = HIP's: "Streams" in rtlws_hip.h); one kernel launch and no other runtime
 * call.  nout == 0 does nothing.  Every refusal is made before the device is asked for anything, in this order:
 * ntrials, nout, in_stride at least nout and a multiple of 4, null pointers (d_in, d_peak, d_at), the alignments of
 * d_in, d_peak, d_at and d_mom, then a null plan, then what the plan decides (in_stride >= samples_needed, the grid).
 * 0; -1 bad argument; -3 HIP failure. */
int rtlws_pulse_run(rtlws_pulse_plan* p, const float* d_in, long in_stride, int ntrials, long nout, float* d_peak,
                    int32_t* d_at, double* d_mom, void* stream);

/* The signal-to-noise ratio of a boxcar sum `peak` of `width` samples over noise whose `count` samples add to sum1 and
 * whose squares add to sum2 (a segment's moments, or several segments' added), in double on the host:
 *   mean = sum1 / count;  var = sum2 / count - mean * mean;  snr = (peak - width * mean) / sqrt(width * var)
 * NaN where count < 2, width < 1 or var is not positive.  Needs no GPU. */
double rtlws_pulse_snr(double peak, int width, double sum1, double sum2, long count);

void rtlws_pulse_close(rtlws_pulse_plan* p);

/* Last error text of the calling thread from this library ("" when none). */
const char* rtlws_pulse_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* RTLWS_PULSE_H */
