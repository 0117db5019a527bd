/*
 * rtlws_subdedisp.h -- two-stage (subband) incoherent dedispersion of spectrometer rows: the channels of a waterfall
 * are summed inside subbands under a few nominal trials, and every trial then sums the subband series of its nominal,
 * two launches (librtlws_subdedisp.so).
 *
 * rtlws_dedisp_run (rtlws_dedisp.h) spends ntrials * nchan additions per output.  Neighbouring trials delay the
 * neighbouring channels of a subband almost alike: with B subbands of C = M / B channels and A nominal trials that
 * each serve T / A trials, A M + T B additions per output do (T / A = C = 16: an eighth).  What is lost is that a
 * trial's channels are delayed inside their subband as its nominal delays them: rtlws_subdedisp_delays says by how many
 * rows at most (smear_rows), and an observer chooses nsub and per_nominal by it.  It is another order of summation
 * than rtlws_dedisp.h's, so another definition (tests/subdedisp_ref.py restates it in numpy).
 *
 *   M = nchan       values per row, 4 .. 4096 and a multiple of 4
 *   B = nsub        subbands, 1 .. M / 4, M % B == 0 and C = M / B a multiple of 4; subband s is positions s C .. s C + C - 1
 *   A = nnominal    nominal trials, 1 .. 4096;  T = ntrials, 1 .. 4096, A <= T
 *   first[0 .. A]   int32, first[0] = 0, first[A] = T, strictly ascending: trial t belongs to nominal a(t),
 *                   first[a] <= t < first[a + 1]
 *   S[j][i]         value i of row j: f32 in device memory, row j at d_rows + j * in_stride
 *   d1[a][i]        delay in rows of position i inside its subband under nominal a: int32, A * M at open, 0 .. 65535
 *   d2[t][s]        delay in rows of subband s under trial t: int32, T * B at open, 0 .. 65535
 *   mask[i]         bytes, optional (NULL: all ones); 0 leaves value i out of every sum
 *
 *   nmid = nout + max_d2      max_d2 the largest d2 over the subbands that keep a position, max_d1 the largest d1 over
 *                             the positions the mask keeps (0 where it keeps none)
 *   P[a][s][m] = acc after:  acc = +0.0f;  for i = s C, .., s C + C - 1 ascending: if mask[i]: acc = fl(acc + S[m + d1[a][i]][i])
 *                a = 0 .. A - 1,  s = 0 .. B - 1,  m = 0 .. nmid - 1
 *   D[t][n]    = acc after:  acc = +0.0f;  for s = 0, .., B - 1 ascending: acc = fl(acc + P[a(t)][s][n + d2[t][s]])
 *                t = 0 .. T - 1,  n = 0 .. nout - 1        (a subband that keeps no position is left out: its P is +0.0)
 *
 * One f32 accumulator per value, one rounding per addition, in ascending position and then in ascending subband.  The
 * order depends on nothing else -- not the trial, n, nout, the grid or how the plan tiled the tables -- and no atomics
 * take part: two runs give the same bits, and a run over the rows from j0 on gives outputs j0 .. of the whole run bit
 * for bit.  A subband with nothing kept is a series of +0.0: it is written, and it leaves every acc as it is.  The
 * library only adds floats: non-finite values propagate as IEEE addition propagates them.
 *
 * The run reads rows_needed = nout + max_d2 + max_d1 rows; no row beyond them is read, nor any element of a row at or
 * beyond nchan.  P lives in a workspace of the caller's, subband-major, so that each subband's series is contiguous in
 * time (both stages run lanes along time, and these are the subband series an observer archives): P[a][s][m] is at
 * d_work + (a B + s) * mid_stride + m, mid_stride = nmid rounded up to a multiple of 4; the words m >= nmid are not
 * written.  Trial t is the nout contiguous f32 at d_out + t * out_stride; nothing else is written.  Strides are in
 * elements.
 *
 * Every table within the limits is served; what a table costs is speed.  Stage 1 is rtlws_dedisp.h's tile over d1 as
 * a table of A trials (its plan by the same rule: nominals_per_block 8, 4, 2 or 1), its sums stored at every subband's
 * last position.  In stage 2 a workgroup owns 256 consecutive outputs of up to trials_per_block consecutive trials of
 * one nominal (a group never holds trials of two) and stages, 32 subbands at a time, the part of each subband's series
 * between the least and the largest d2 its trials have: the plan takes the largest trials_per_block of 8, 4, 2, 1 (no
 * larger than the largest nominal fills half of) whose widest such spread stays within 248 rows (within 24 rows a
 * workgroup takes 36 KiB of LDS, else 64 KiB); one trial spreads nothing.  rtlws_subdedisp_geometry says what tables
 * get.  Measured on one MI355X (profiles/subdedisp_rates.txt) at 256 trials, T / A = 8 .. 32 and
 * C = 8 .. 32, where A M + T B is 0.13 .. 0.16 of T M: the library pays for long runs (65 536 rows: 0.27 .. 0.56 of
 * rtlws_dedisp_run's time at 1024 and at 64 channels) and does not for short ones (8192 rows: 0.95 .. 1.26), where stage 1,
 * ceil(nmid / 256) ceil(A / 8) workgroups, leaves most of the device idle; nor will it for a handful of trials.
 *
 * Refused with -1 (rtlws_subdedisp_last_error() says why), in this order: nchan outside 4 .. 4096 or not a multiple of
 * 4, nsub that is not such a divisor, nnominal outside 1 .. 4096, ntrials outside 1 .. 4096, nnominal > ntrials, a
 * null first, a first that does not ascend strictly from 0 to ntrials, a null table, a delay outside 0 .. 65535,
 * nout < 0, in_stride < nchan or not a multiple of 4, out_stride < nout, null pointers, d_rows not 16-byte aligned,
 * d_work or d_out not 4-byte aligned, more workgroups than one grid holds.
 */
#ifndef RTLWS_SUBDEDISP_H
#define RTLWS_SUBDEDISP_H

#include <stdint.h>

#include "rtlws_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* librtlws_subdedisp.so exports these declarations and nothing else (exports/subdedisp.map) */
#pragma GCC visibility push(default)

#define RTLWS_SUBDEDISP_MIN_NCHAN 4
#define RTLWS_SUBDEDISP_MAX_NCHAN 4096
#define RTLWS_SUBDEDISP_MIN_PER_SUB 4
#define RTLWS_SUBDEDISP_MAX_NOMINALS 4096
#define RTLWS_SUBDEDISP_MAX_TRIALS 4096
#define RTLWS_SUBDEDISP_MAX_DELAY 65535

typedef struct rtlws_subdedisp_plan rtlws_subdedisp_plan;

/* 1 when the shape is served, else 0 (rtlws_subdedisp_last_error() says why).  Needs no GPU. */
int rtlws_subdedisp_supported(int nchan, int nsub, int nnominal, int ntrials);

/* The tables of a dispersion sweep: ntrials dispersion measures DM_t = dm0 + t dm_step (pc cm^-3) over the band of
 * rtlws_dedisp_delays (rtlws_dedisp.h: nu_i, and x_i = nu_i^-2 - nu_max^-2), nominal a = 0 .. A - 1,
 * A = ceil(ntrials / per_nominal), owning trials a per_nominal .. (first[a] = a per_nominal, first[A] = ntrials), in
 * double:
 *   DM_a = (DM_first[a] + DM_(first[a + 1] - 1)) / 2: the mean of its own trials, the ragged last nominal's too,
 *   ref(s) the position of subband s with the least x (its highest frequency, whichever `shifted` wrote the rows),
 *   d1[a * M + i] = rint(4.148808e3 DM_a (x_i - x_ref(s)) / row_seconds),  s the subband of i,
 *   d2[t * B + s] = rint(4.148808e3 DM_t x_ref(s) / row_seconds),
 *   *smear_rows  = the largest |DM_t - DM_a(t)| 4.148808e3 (x_i - x_ref(s)) / row_seconds over (t, i): by how many
 *                  rows a trial's delay of a position differs from d1 + d2, roundings aside (smear_rows may be NULL).
 * first holds A + 1, d1 A * M and d2 ntrials * B int32.  0; -1, in this order, for nchan, nsub or ntrials that is not
 * served, shifted other than 0 or 1, per_nominal < 1, a null table, a frequency (the lowest nu_i), bandwidth or row
 * time that is not positive and finite, a negative or non-finite DM (the text names the trial), or a delay above 65535
 * (the text names the trial or the nominal).  Needs no GPU. */
int rtlws_subdedisp_delays(int nchan, int nsub, int shifted, double f_centre_hz, double bandwidth_hz, double row_seconds,
                           int ntrials, double dm0, double dm_step, int per_nominal, int32_t* first, int32_t* d1,
                           int32_t* d2, double* smear_rows);

/* What a plan of these tables launches for nout outputs per trial, stage 1 at [0] and stage 2 at [1]: workgroups,
 * threads per workgroup and bytes of LDS per workgroup (arrays of two), outputs per workgroup (256, both stages), the
 * nominals per workgroup of stage 1 and the trials per workgroup of stage 2 (8, 4, 2 or 1), max_d1 and max_d2;
 * blocks[0] = ceil(nmid / tile_out) ceil(A / nominals_per_block), blocks[1] = ceil(nout / tile_out) times the groups
 * of stage 2, the sum over the nominals of ceil(trials of the nominal / trials_per_block).  mask may be NULL, and so
 * may any of the pointers behind nout.  0, or -1 when the tables are not served, nout < 0 or a grid does not hold the
 * workgroups.  Needs no GPU. */
int rtlws_subdedisp_geometry(int nchan, int nsub, int nnominal, int ntrials, const int32_t* first, const int32_t* d1,
                             const int32_t* d2, const uint8_t* mask, long nout, int* blocks, int* threads,
                             int* lds_bytes, int* tile_out, int* nominals_per_block, int* trials_per_block, int* max_d1,
                             int* max_d2);

/* The tables (first: nnominal + 1, d1: nnominal * nchan, d2: ntrials * nsub int32) and the mask (nchan bytes or NULL),
 * all in host memory and read before the call returns, on the engine's device in the kernels' form, and both kernels
 * loaded, so that rtlws_subdedisp_run makes no runtime call other than its two launches and may be captured into a
 * hipGraph.  New tables or a new mask are a new plan.  NULL on failure (a null engine among them: without a device
 * there is no engine, and no CPU path). */
rtlws_subdedisp_plan* rtlws_subdedisp_open(rtlws_engine* e, int nchan, int nsub, int nnominal, int ntrials,
                                           const int32_t* first, const int32_t* d1, const int32_t* d2, const uint8_t* mask);

/* Rows that nout outputs per trial read: nout + max_d2 + max_d1, 0 for nout == 0; -1 for a null plan or nout < 0. */
long rtlws_subdedisp_rows_needed(const rtlws_subdedisp_plan* p, long nout);
/* Elements between two subband series of the workspace: nout + max_d2 rounded up to a multiple of 4, 0 for nout == 0;
 * and the f32 the workspace holds, nnominal * nsub * mid_stride.  -1 for a null plan or nout < 0. */
long rtlws_subdedisp_mid_stride(const rtlws_subdedisp_plan* p, long nout);
long rtlws_subdedisp_work_floats(const rtlws_subdedisp_plan* p, long nout);

/* d_rows: rtlws_subdedisp_rows_needed() rows of f32, 16-byte aligned; d_work: rtlws_subdedisp_work_floats() f32, the
 * subband series P behind the run; d_out: ntrials rows of nout f32.  Asynchronous on `stream` (NULL = the engine's own
 * stream, RTLWS_STREAM_DEFAULT = HIP's: "Streams" in rtlws_hip.h); exactly two kernel launches and no other runtime
 * call.  nout == 0 does nothing.  Every refusal is made before the device is asked for anything: nout, in_stride at
 * least 4 and a multiple of 4, out_stride, null pointers, the three alignments, then a null plan, then what the plan
 * decides (in_stride >= nchan, the grid of stage 1, the grid of stage 2).  0; -1 bad argument; -3 HIP failure. */
int rtlws_subdedisp_run(rtlws_subdedisp_plan* p, const float* d_rows, long in_stride, long nout, float* d_work,
                        float* d_out, long out_stride, void* stream);

void rtlws_subdedisp_close(rtlws_subdedisp_plan* p);

/* Last error text of the calling thread from this library ("" when none). */
const char* rtlws_subdedisp_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* RTLWS_SUBDEDISP_H */
