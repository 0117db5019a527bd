/*
 * rtlws_fold.h -- epoch folding of dedispersed time series: every trial's series is phase-binned at every period of a
 * table and added, per sub-integration, all trials and periods in one launch (librtlws_fold.so).
 *
 * rtlws_dedisp_run (rtlws_dedisp.h) leaves ntrials f32 series on the device; this library reads them where they lie
 * (tests/fold_ref.py restates it in numpy).
 *
 *   D[t][n]     f32 on the device, trial t at d_in + t * in_stride; t = 0 .. ntrials-1, n = 0 .. nsamp-1
 *   (step_p, phi0_p)   p = 0 .. nperiods-1: two uint64 tables in host memory at open; phase in units of 2^-64 turn
 *   nbins       phase bins, 2 .. 256 (any integer)            sub   samples per sub-integration, 64 .. 2^24, a multiple of 4
 *   nsub = ceil(nsamp / sub)
 *
 *   phase_p(n) = (phi0_p + n * step_p) mod 2^64
 *   bin_p(n)   = (((phase_p(n) >> 32) * nbins) >> 32)                      -- 0 .. nbins-1, integers only
 *
 *   prof[t][p][s][b]:  acc = +0.0f;  for n = s*sub .. min((s+1)*sub, nsamp) - 1 ascending:
 *                           if bin_p(n) == b:  acc = fl(acc + D[t][n])     (one f32 rounding per addition)
 *   hits[p][s][b]   :  the number of such n (uint32)
 *
 * The order of the additions depends on n alone -- not on the trial, the period's place in the table, the grid or the
 * tile -- and no atomic whose order is open takes part: two runs give the same bits, and a run over the samples from
 * n0 = s0 * sub on with every phi0_p replaced by phase_p(n0) (rtlws_fold_phase_at) gives sub-integrations s0 .. of the
 * whole run bit for bit.  The library only adds floats: a non-finite sample reaches the one bin it falls in and no
 * other, subnormal sums are kept, and an empty bin is +0.0 with hits 0.  Every step is served, 0 (all samples in one
 * bin), 2^63 and 2^64 - 1 among them; what a table costs is speed.
 *
 * The run reads samples 0 .. nsamp - 1 of every trial and nothing else: nothing in the stride's padding, nothing at or
 * beyond nsamp.  It writes d_prof[((t * nperiods + p) * nsub + s) * nbins + b] (f32) and, if d_hits is not NULL,
 * d_hits[(p * nsub + s) * nbins + b] (uint32; hits does not depend on the trial: written once), and nothing else.
 * Strides are in elements.  The input layout is what rtlws_dedisp_run writes when out_stride is a multiple of 4: the
 * two libraries chain on the device with no copy.
 *
 * A wavefront owns 64 consecutive periods of the table (a lane a period), one trial and one sub-integration, and walks
 * the sub-integration's samples in ascending n, `tile` samples staged per step.  Its histogram is [bin][lane] f32 in
 * LDS, nbins * 256 bytes; a workgroup is waves_per_block wavefronts of one trial and sub-integration: 4 for nbins up to
 * 64, 2 up to 128, 1 up to 256, never more than 64 KiB.  The grid is ntrials * ceil(nperiods / (64 waves_per_block)) *
 * nsub workgroups.  rtlws_fold_geometry says what a plan launches.
 *
 * Refused with -1 (rtlws_fold_last_error() says why): nperiods outside 1 .. 4096, a null table, nbins outside
 * 2 .. 256, sub outside 64 .. 2^24 or not a multiple of 4, ntrials outside 1 .. 65536, nsamp outside 0 .. 2^30,
 * in_stride below nsamp or not a multiple of 4, null pointers, d_in not 16-byte aligned, d_prof or d_hits not 4-byte
 * aligned, more workgroups than one grid holds.
 */
#ifndef RTLWS_FOLD_H
#define RTLWS_FOLD_H

#include <stdint.h>

#include "rtlws_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* librtlws_fold.so exports these declarations and nothing else (exports/fold.map) */
#pragma GCC visibility push(default)

#define RTLWS_FOLD_MAX_PERIODS 4096
#define RTLWS_FOLD_MIN_BINS 2
#define RTLWS_FOLD_MAX_BINS 256
#define RTLWS_FOLD_MIN_SUB 64
#define RTLWS_FOLD_MAX_SUB 16777216
#define RTLWS_FOLD_MAX_TRIALS 65536
#define RTLWS_FOLD_MAX_NSAMP 1073741824

typedef struct rtlws_fold_plan rtlws_fold_plan;

/* 1 when the tables, nbins and sub are served, else 0 (rtlws_fold_last_error() says why).  Needs no GPU. */
int rtlws_fold_supported(int nperiods, const uint64_t* steps, const uint64_t* phases, int nbins, long sub);

/* What a plan of nperiods periods launches for nsamp samples of each of ntrials trials: workgroups (ntrials *
 * ceil(nperiods / (64 waves_per_block)) * nsub), threads per workgroup (64 waves_per_block), bytes of LDS per workgroup
 * (waves_per_block * nbins * 256), samples a wavefront stages per step, wavefronts per workgroup, and nsub =
 * ceil(nsamp / sub).  Any of the pointers behind nsamp may be NULL.  0, or -1 when nperiods, nbins or sub is not
 * served, ntrials or nsamp is outside its range or the grid does not hold the workgroups.  Needs no GPU. */
int rtlws_fold_geometry(int nperiods, int nbins, long sub, int ntrials, long nsamp, int* blocks, int* threads, int* lds_bytes,
                        int* tile, int* waves_per_block, long* nsub);

/* The tables (nperiods uint64 each in host memory, read before the call returns) on the engine's device, and the
 * kernel loaded, so that rtlws_fold_run makes no runtime call other than its launch and may be captured into a
 * hipGraph.  New tables, nbins or sub are a new plan.  NULL on failure (a null engine among them: without a device there
 * is no engine, and no CPU path). */
rtlws_fold_plan* rtlws_fold_open(rtlws_engine* e, int nperiods, const uint64_t* steps, const uint64_t* phases, int nbins, long sub);

/* ceil(nsamp / sub); -1 for a null plan or nsamp outside 0 .. 2^30. */
long rtlws_fold_subints(const rtlws_fold_plan* p, long nsamp);

/* d_in: ntrials series of nsamp f32, in_stride apart, 16-byte aligned; d_prof: ntrials * nperiods * nsub * nbins f32;
 * d_hits: nperiods * nsub * nbins uint32, or NULL: no hits are counted or written.  Asynchronous on `stream` (NULL = the
 * engine's own stream, RTLWS_STREAM_DEFAULT = HIP's: "Streams" in rtlws_hip.h); one kernel launch and no other runtime
 * call.  nsamp == 0 does nothing.  Every refusal is made before the device is asked for anything, in this order:
 * ntrials, nsamp, in_stride at least nsamp and a multiple of 4, null pointers (d_in, d_prof), the alignments of d_in,
 * d_prof and d_hits, then a null plan, then what the plan decides (the grid).
 * 0; -1 bad argument; -3 HIP failure. */
int rtlws_fold_run(rtlws_fold_plan* p, const float* d_in, long in_stride, int ntrials, long nsamp, float* d_prof, uint32_t* d_hits,
                   void* stream);

/* The step of a period of period_in_samples samples: the integer nearest to 2^64 / P, exactly (a double is m 2^e, so
 * the quotient 2^(64-e) / m is one integer division; halves round up).  0 with the error text set where P is outside
 * 2 .. 2^32 or NaN.  Needs no GPU. */
uint64_t rtlws_fold_step(double period_in_samples);

/* phase(n0) = (phi0 + n0 * step) mod 2^64: the phi0 of a run that starts at sample n0.  Needs no GPU. */
uint64_t rtlws_fold_phase_at(uint64_t step, uint64_t phi0, long n0);

/* The epoch-folding statistic of one profile (nbins f32) and its hits over noise whose `count` samples add to sum1 and
 * whose squares add to sum2 (rtlws_pulse_run's moments of the trial), in double on the host, b ascending:
 *   mean = sum1 / count;  var = sum2 / count - mean * mean;  chi2 = sum_b (prof_b - hits_b mean)^2 / (hits_b var)
 * NaN where count < 2, nbins < 1, a pointer is null, var is not positive or some hits_b is 0.  Needs no GPU. */
double rtlws_fold_chi2(const float* prof, const uint32_t* hits, int nbins, double sum1, double sum2, long count);

void rtlws_fold_close(rtlws_fold_plan* p);

/* Last error text of the calling thread from this library ("" when none). */
const char* rtlws_fold_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* RTLWS_FOLD_H */
