/*
 * rtlws_cand.h -- candidate folding: the waterfall itself is folded at a candidate's period into a cube of
 * (sub-integration, channel, phase) profiles, each channel behind its own dispersion delay, all candidates in one
 * launch; the cube is then shifted and added over a grid of DM offsets and of period / period-derivative offsets, and
 * every trial's profile is reduced to the two sums of its chi-square (librtlws_cand.so).
 *
 * The searches (rtlws_pulse.h, rtlws_period.h, rtlws_periodlong.h, rtlws_accel.h, rtlws_ffa.h) and rtlws_fold_run work on
 * series that rtlws_dedisp_run summed over the band at a DM of its grid.  What a candidate (period, DM) is asked next --
 * is it broadband, is it there in every sub-integration, which DM, period and period derivative near the grid point is
 * the best one -- is answered from the waterfall, which this library reads exactly as rtlws_dedisp_run reads it
 * (tests/cand_ref.py restates everything below in numpy as plain loops).
 *
 * 1. The cube: rtlws_cand_fold_open / _run
 *
 *   S[j][i]       value i of row j: f32 in device memory, row j at d_rows + j * in_stride; nchan 4 .. 4096, a multiple of 4
 *   ncand         1 .. 64
 *   (step_c, phi0_c)   two uint64 tables in host memory at open, in rtlws_fold.h's units: phase in 2^-64 turn (rtlws_fold_step)
 *   delays[c][i]  int32, 0 .. 65535 rows, ncand * nchan in host memory at open or NULL (all zeros): the layout
 *                 rtlws_dedisp_delays writes, one trial per candidate
 *   mask[i]       bytes, optional (NULL: all ones); 0 leaves channel i out
 *   nbins         2 .. 256            sub   16 .. 2^24 rows per sub-integration
 *   nsamp         0 .. 2^30 at the run;  nsub = ceil(nsamp / sub)
 *
 *   phase_c(n) = (phi0_c + n * step_c) mod 2^64
 *   bin_c(n)   = ((phase_c(n) >> 32) * nbins) >> 32                          -- rtlws_fold.h's, integers only
 *   cube[c][s][i][b]:  acc = +0.0f;  for n = s*sub .. min((s+1)*sub, nsamp) - 1 ascending:
 *                          if bin_c(n) == b:  acc = fl(acc + S[n + delays[c][i]][i])    (one f32 rounding per addition)
 *   hits[c][s][b]   :  the number of such n (uint32; it does not depend on the channel: written once)
 *
 * The order of the additions depends on n alone and no atomics take part: two runs give the same bits, and a run over
 * the rows from n0 = s0 * sub on with every phi0_c replaced by rtlws_fold_phase_at(step_c, phi0_c, n0) gives
 * sub-integrations s0 .. of the whole run bit for bit.  The library only adds floats: a non-finite sample reaches the
 * one bin it falls in and no other, subnormal sums are kept, an empty bin is +0.0.  Every step is served, 0, 2^63 and
 * 2^64 - 1 among them.  A masked channel's entries are +0.0 and its rows are never read.
 *
 * The run reads rows 0 .. nsamp + max_delay - 1 (rtlws_cand_fold_rows_needed), max_delay the largest delay over the
 * channels the mask keeps and all candidates; nothing at or beyond nchan in a row and nothing behind those rows.  It
 * writes d_cube[((c * nsub + s) * nchan + i) * nbins + b] (f32) and, if d_hits is not NULL,
 * d_hits[(c * nsub + s) * nbins + b], and nothing else.  Strides are in elements.
 *
 * A wavefront owns 64 consecutive channels (a lane a channel), one candidate and one sub-integration; its histogram is
 * rtlws_fold.h's [bin][lane] f32 in LDS, and a workgroup is waves_per_block wavefronts by that header's rule (4 for
 * nbins up to 64, 2 up to 128, 1 up to 256).  The grid is ncand * nsub * ceil(nchan / (64 waves_per_block)) workgroups.
 *
 * 2. The refinement: rtlws_cand_search_open / _run
 *
 *   ncand 1 .. 64, nsub 1 .. 1024, nchan and nbins as above
 *   a[c][q][i]    int32 in 0 .. nbins - 1, q < ndm, ndm 1 .. 256: the phase shift of channel i under DM trial q
 *   g[c][r][s]    int32 in 0 .. nbins - 1, r < ntr, ntr 1 .. 4096: the phase shift of sub-integration s under the
 *                 period / period-derivative trial r
 *
 *   T[c][q][s][b] = acc after:  acc = +0.0f;  for i = 0 .. nchan-1 ascending: acc = fl(acc + cube[c][s][i][(b + a[c][q][i]) mod nbins])
 *   P[c][q][r][b] = acc after:  acc = +0.0f;  for s = 0 .. nsub-1 ascending:  acc = fl(acc + T[c][q][s][(b + g[c][r][s]) mod nbins])
 *   stat[c][q][r]  (f64) = acc after:  acc = 0.0;  for b ascending: acc = fl64(acc + (double)P_b * (double)P_b)
 *   total[c][q][r] (f64) = the same over (double)P_b
 *
 * The product of two f32 is exact in f64 (48 bits of significand at most), so a fused multiply-add and a multiplication
 * followed by an addition round the same number once: both forms give the same bits.  Masked channels are zeros in the
 * cube, and adding them changes no sum but a -0.0 into +0.0.  The cube is read where rtlws_cand_fold_run left it.  T
 * lives in a workspace the plan owns (ncand * ndm * nsub * nbins f32, at most 2^30 bytes); stat and total are always
 * written, P and a copy of T (the time-phase plot at DM trial q) where the caller passes a pointer.  The run is two
 * launches with nothing between them but the stream order.  In both a wavefront takes one trial with its lanes along the
 * bins, and 8 trials form a workgroup that stages 32 rows of nbins values at a time in LDS: ncand * nsub * ceil(ndm / 8)
 * workgroups, then ncand * ndm * ceil(ntr / 8).
 *
 * Refused with -1 (rtlws_cand_last_error() says why): a count outside its range, null tables or pointers, a delay
 * outside 0 .. 65535, a shift outside 0 .. nbins - 1, nchan not a multiple of 4, in_stride below nchan or not a multiple
 * of 4, d_rows not 16-byte aligned, d_cube or d_hits not 4-byte aligned, d_stat or d_total not 8-byte aligned, a
 * workspace above 2^30 bytes, more workgroups than one grid holds.
 */
#ifndef RTLWS_CAND_H
#define RTLWS_CAND_H

#include <stdint.h>

#include "rtlws_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* librtlws_cand.so exports these declarations and nothing else (exports/cand.map) */
#pragma GCC visibility push(default)

#define RTLWS_CAND_MAX_CANDS 64
#define RTLWS_CAND_MIN_NCHAN 4
#define RTLWS_CAND_MAX_NCHAN 4096
#define RTLWS_CAND_MAX_DELAY 65535
#define RTLWS_CAND_MIN_BINS 2
#define RTLWS_CAND_MAX_BINS 256
#define RTLWS_CAND_MIN_SUB 16
#define RTLWS_CAND_MAX_SUB 16777216
#define RTLWS_CAND_MAX_NSAMP 1073741824
#define RTLWS_CAND_MAX_NSUB 1024
#define RTLWS_CAND_MAX_NDM 256
#define RTLWS_CAND_MAX_NTR 4096
#define RTLWS_CAND_MAX_WORKSPACE 1073741824

typedef struct rtlws_cand_fold_plan rtlws_cand_fold_plan;
typedef struct rtlws_cand_search_plan rtlws_cand_search_plan;

/* 1 when the cube's shape is served, else 0 (rtlws_cand_last_error() says why).  Needs no GPU. */
int rtlws_cand_fold_supported(int ncand, int nchan, int nbins, long sub);

/* What a plan of that shape launches for nsamp rows: workgroups (ncand * nsub * ceil(nchan / (64 waves_per_block))),
 * threads per workgroup (64 waves_per_block), bytes of LDS per workgroup (waves_per_block * nbins * 256), wavefronts per
 * workgroup and nsub = ceil(nsamp / sub).  Any of the pointers behind nsamp may be NULL.  0, or -1 when the shape is not
 * served, nsamp is outside 0 .. 2^30 or the grid does not hold the workgroups.  Needs no GPU. */
int rtlws_cand_fold_geometry(int ncand, int nchan, int nbins, long sub, long nsamp, int* blocks, int* threads, int* lds_bytes,
                             int* waves_per_block, long* nsub);

/* The tables (steps and phases: ncand uint64 each; delays: ncand * nchan int32 or NULL; mask: nchan bytes or NULL; all in
 * host memory, read before the call returns) on the engine's device and the kernel loaded, so that rtlws_cand_fold_run
 * makes no runtime call other than its launch and may be captured into a hipGraph.  Refused in this order, all before
 * the device is asked for anything: ncand, nchan, nbins, sub, null steps, null phases, a delay outside 0 .. 65535 (at
 * a masked channel too), then the null engine.  NULL on failure (without a device there is no engine, and no CPU
 * path). */
rtlws_cand_fold_plan* rtlws_cand_fold_open(rtlws_engine* e, int ncand, const uint64_t* steps, const uint64_t* phases, int nchan,
                                           const int32_t* delays, const uint8_t* mask, int nbins, long sub);

/* Rows that nsamp samples read: nsamp + max_delay, 0 for nsamp == 0; -1 for nsamp outside 0 .. 2^30 or a null plan. */
long rtlws_cand_fold_rows_needed(const rtlws_cand_fold_plan* p, long nsamp);

/* d_rows: rtlws_cand_fold_rows_needed() rows of f32, in_stride apart, 16-byte aligned; d_cube: ncand * nsub * nchan *
 * nbins f32; d_hits: ncand * nsub * nbins uint32, or NULL: no hits are counted or written.  Asynchronous on `stream`
 * (NULL = the engine's own stream, RTLWS_STREAM_DEFAULT = HIP's: "Streams" in rtlws_hip.h); one kernel launch and no
 * other runtime call.  nsamp == 0 does nothing.  Every refusal is made before the device is asked for anything, in this
 * order: nsamp, in_stride at least 4 and a multiple of 4, null pointers (d_rows, d_cube), the alignments of d_rows,
 * d_cube and d_hits, then a null plan, then what the plan decides (in_stride at least nchan, the grid).
 * 0; -1 bad argument; -3 HIP failure. */
int rtlws_cand_fold_run(rtlws_cand_fold_plan* p, const float* d_rows, long in_stride, long nsamp, float* d_cube, uint32_t* d_hits,
                        void* stream);

void rtlws_cand_fold_close(rtlws_cand_fold_plan* p);

/* 1 when the refinement's shape is served, else 0 (rtlws_cand_last_error() says why).  Needs no GPU. */
int rtlws_cand_search_supported(int ncand, int nsub, int nchan, int nbins, int ndm, int ntr);

/* What a plan of that shape launches: the workgroups of stage 1 (ncand * nsub * ceil(ndm / 8)) and of stage 2 (ncand * ndm
 * * ceil(ntr / 8)), threads per workgroup (512), the bytes of LDS of a workgroup of stage 1 (32 * nbins * 4) and of
 * stage 2 (40 * nbins * 4), and the bytes of the plan's workspace (ncand * ndm * nsub * nbins * 4).  Any of the pointers
 * may be NULL.  0, or -1 when the shape is not served.  Needs no GPU. */
int rtlws_cand_search_geometry(int ncand, int nsub, int nchan, int nbins, int ndm, int ntr, int* blocks1, int* blocks2, int* threads,
                               int* lds_bytes1, int* lds_bytes2, long* workspace_bytes);

/* The two shift tables (a: ncand * ndm * nchan int32, g: ncand * ntr * nsub int32, in host memory, read before the call
 * returns) and the workspace on the engine's device and both kernels loaded, so that rtlws_cand_search_run makes no
 * runtime call other than its two launches and may be captured into a hipGraph.  Refused in this order, all before the
 * device is asked for anything: ncand, nsub, nchan, nbins, ndm, ntr, the workspace, null a, null g, an entry of a and
 * then of g outside 0 .. nbins - 1, then the null engine.  NULL on failure. */
rtlws_cand_search_plan* rtlws_cand_search_open(rtlws_engine* e, int ncand, int nsub, int nchan, int nbins, int ndm, const int32_t* a,
                                               int ntr, const int32_t* g);

/* d_cube: ncand * nsub * nchan * nbins f32 as rtlws_cand_fold_run writes them; d_stat, d_total: ncand * ndm * ntr f64;
 * d_prof: ncand * ndm * ntr * nbins f32 (P) or NULL; d_tphase: ncand * ndm * nsub * nbins f32 (T) or NULL.  Asynchronous
 * on `stream` as above; two kernel launches and no other runtime call.  Every refusal is made before the device is
 * asked for anything, in this order: null pointers (d_cube, d_stat, d_total), the alignments of d_cube (4 bytes),
 * d_stat and d_total (8 bytes), d_prof and d_tphase (4 bytes), then a null plan.  0; -1 bad argument; -3 HIP failure. */
int rtlws_cand_search_run(rtlws_cand_search_plan* p, const float* d_cube, double* d_stat, double* d_total, float* d_prof, float* d_tphase,
                          void* stream);

void rtlws_cand_search_close(rtlws_cand_search_plan* p);

/* The per-channel phase shifts of ndm DM offsets dDM_q = ddm0 + q ddm_step (pc cm^-3; signed: they lie around the DM the
 * cube was folded at) for a period of period_rows rows, over rtlws_dedisp_delays' description of the band, in double:
 *   position i is channel c = i (shifted = 0) or (i + M / 2) mod M (shifted = 1), M = nchan,
 *   nu_i = f_centre + (c < M / 2 ? c : c - M) bandwidth / M, in MHz; nu_max the highest of them,
 *   dt_i(dDM) = 4.148808e3 dDM (nu_i^-2 - nu_max^-2) / row_seconds                     rows against the highest channel
 *   a[q * M + i] = rint(nbins dt_i(dDM_q) / period_rows) mod nbins, reduced into 0 .. nbins - 1.
 * A pulse whose DM exceeds the cube's by dDM_q arrives dt_i rows late in channel i, a[q][i] bins late in the cube; T reads
 * the cube that many bins further on, which lines the channels up.  0; -1 for nchan outside 4 .. 4096 or not a multiple
 * of 4, shifted other than 0 or 1, a frequency (the lowest nu_i), bandwidth, row time or period that is not positive and
 * finite, nbins outside 2 .. 256, ndm outside 1 .. 256, an offset that is not finite, a null table, or a shift of 2^31
 * bins or more.  Needs no GPU. */
int rtlws_cand_dm_shifts(int nchan, int shifted, double f_centre_hz, double bandwidth_hz, double row_seconds, double period_rows, int nbins,
                         int ndm, double ddm0, double ddm_step, int32_t* a);

/* The per-sub-integration phase shifts of a grid of nf frequency offsets df_j = df0 + j df_step (turns per row) by nfd
 * derivative offsets dfd_k = dfd0 + k dfd_step (turns per row^2), r = k * nf + j (the frequency index runs fastest), in
 * double:
 *   t_s = (s + 1/2) sub                                                                 the middle of sub-integration s, rows
 *   g[r * nsub + s] = rint(nbins (df_j t_s + dfd_k t_s^2 / 2)) mod nbins, reduced into 0 .. nbins - 1.
 * The offsets are the fold's against the pulsar's, as the DM offsets are the pulsar's delay against the fold's: df is
 * the folding frequency less the pulsar's, dfd the same of the derivatives.  A pulsar slower than the fold by df arrives
 * df turns later every row and drifts df t + dfd t^2 / 2 turns forward through the folded phase; P reads T that many
 * bins further on, and the trial's frequency is the folding frequency less df_j.  0; -1 for nbins outside 2 .. 256, sub outside 16 .. 2^24, nsub outside 1 .. 1024, nf or nfd below 1 or
 * nf * nfd above 4096, an offset that is not finite, a null table, or a shift of 2^31 bins or more.  Needs no GPU. */
int rtlws_cand_drift_shifts(int nbins, long sub, int nsub, int nf, double df0, double df_step, int nfd, double dfd0, double dfd_step,
                            int32_t* g);

/* (stat - total^2 / nbins) / ((nbins - 1) bin_variance): the reduced chi-square of a profile of nbins bins against a flat
 * one, from rtlws_cand_search_run's two sums and the variance of one bin of P under noise.  NaN where nbins < 2 or the
 * variance is not positive.  Needs no GPU. */
double rtlws_cand_chi2(double stat, double total, int nbins, double bin_variance);

/* Last error text of the calling thread from this library ("" when none). */
const char* rtlws_cand_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* RTLWS_CAND_H */
