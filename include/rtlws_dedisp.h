/*
 * rtlws_dedisp.h -- incoherent dedispersion of spectrometer rows: for every trial of a table of per-channel delays,
 * each channel of a waterfall is delayed by its own number of rows and the channels are added, one time series per
 * trial, all trials in one launch (librtlws_dedisp.so).
 *
 * rtlws_pfbspec_run and rtlws_pfbsk_run (rtlws_pfbspec.h, rtlws_pfbsk.h) turn a capture into f32 rows, one per K
 * frames; so does rtlws_spectra_batch (rtlws_hip.h).  A pulse that sweeps down the band arrives in channel i some
 * rows after it arrived in the highest channel; dedispersion undoes that for a trial dispersion measure and sums what
 * is left (tests/dedisp_ref.py restates it in numpy).
 *
 *   M = nchan       values per row, 4 .. 4096 and a multiple of 4
 *   S[j][i]         value i of row j: f32 in device memory, row j at d_rows + j * in_stride
 *   d[t][i]         delay in rows of value i under trial t: int32, ntrials * M in host memory at open, 0 .. 65535
 *   mask[i]         bytes, optional (NULL: all ones); 0 leaves value i out of every sum
 *
 *   D[t][n] = acc after:  acc = +0.0f;  for i = 0, 1, .., M - 1 ascending: if mask[i]: acc = fl(acc + S[n + d[t][i]][i])
 *             t = 0 .. ntrials - 1,  n = 0 .. nout - 1
 *
 * One f32 accumulator per output, one rounding per addition, in ascending position in the row.  The order depends on
 * nothing else -- not the trial, n, nout, the grid or how the plan tiled the table -- and no atomics take part: two
 * runs give the same bits, and a run over the rows from j0 on gives outputs j0 .. of the whole run bit for bit.  i is
 * the position in the row, whatever `shifted` the rows were written with; the table is indexed the same way.  The
 * library only adds floats: non-finite values propagate as IEEE addition propagates them, and a mask of all zeros
 * gives +0.0 everywhere.
 *
 * The run reads rows_needed = nout + max_delay rows, max_delay the largest table entry over the positions the mask
 * keeps; no row beyond them is read, nor any element of a row at or beyond nchan.  Trial t is the nout contiguous f32
 * at d_out + t * out_stride; nothing outside those ranges is written.  Strides are in elements.
 *
 * Every table within the limits is served; what a table costs is speed.  A workgroup owns 256 consecutive outputs of
 * trials_per_block consecutive trials and stages, for every four neighbouring positions, the rows between the least
 * and the largest delay those positions have under its trials.  The plan takes the largest trials_per_block of 8, 4,
 * 2, 1 (8 from five trials on, 4 for three and four) whose widest such spread stays within 247 rows (the rows are
 * then read once per trials_per_block trials, in 128-byte pieces; within 23 rows a workgroup takes 36 KiB of LDS, else
 * 64 KiB); where one trial alone spreads four neighbours further apart it stages narrower pieces (down to 16 bytes of a
 * row, spreads up to 3776 rows), and beyond that each position by itself, which reads every row four times.  A
 * dispersion sweep (rtlws_dedisp_delays) is far inside the first case; rtlws_dedisp_geometry says what a table gets.
 * (The figures 23, 247 and 3776 follow from the tile's rule; tests/test_dedisp_forms_cpu.py holds them to it.)
 *
 * Refused with -1 (rtlws_dedisp_last_error() says why): nchan outside 4 .. 4096 or not a multiple of 4, ntrials
 * outside 1 .. 4096, a null table, a delay outside 0 .. 65535, nout < 0, in_stride < nchan or not a multiple of 4,
 * out_stride < nout, null pointers, d_rows not 16-byte aligned, d_out not 4-byte aligned, more workgroups than one
 * grid holds.
 */
#ifndef RTLWS_DEDISP_H
#define RTLWS_DEDISP_H

#include <stdint.h>

#include "rtlws_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* librtlws_dedisp.so exports these declarations and nothing else (exports/dedisp.map) */
#pragma GCC visibility push(default)

#define RTLWS_DEDISP_MIN_NCHAN 4
#define RTLWS_DEDISP_MAX_NCHAN 4096
#define RTLWS_DEDISP_MAX_TRIALS 4096
#define RTLWS_DEDISP_MAX_DELAY 65535

typedef struct rtlws_dedisp_plan rtlws_dedisp_plan;

/* 1 when the shape is served, else 0 (rtlws_dedisp_last_error() says why).  Needs no GPU. */
int rtlws_dedisp_supported(int nchan, int ntrials);

/* The cold-plasma delays of ntrials dispersion measures DM_t = dm0 + t dm_step (pc cm^-3) for rows of M = nchan
 * values, row_seconds apart, of a band of bandwidth_hz centred on f_centre_hz, in double:
 *   position i is channel c = i (shifted = 0) or (i + M / 2) mod M (shifted = 1),
 *   nu_i = f_centre + (c < M / 2 ? c : c - M) bandwidth / M, in MHz; nu_max the highest of them (c = M / 2 - 1),
 *   delays[t * M + i] = rint(4.148808e3 DM_t (nu_i^-2 - nu_max^-2) / row_seconds).
 * 0; -1 for a shape that is not served, shifted other than 0 or 1, a null table, a frequency (the lowest nu_i),
 * bandwidth or row time that is not positive and finite, a negative or non-finite DM, or a delay above 65535 (the text
 * names the trial).  Needs no GPU. */
int rtlws_dedisp_delays(int nchan, int shifted, double f_centre_hz, double bandwidth_hz, double row_seconds, int ntrials,
                        double dm0, double dm_step, int32_t* delays);

/* What a plan of this table launches for nout outputs per trial: workgroups, threads per workgroup, bytes of LDS per
 * workgroup, outputs (256) and trials (8, 4, 2 or 1) per workgroup, and the largest delay over the positions the mask
 * keeps (0 where it keeps none); blocks = ceil(nout / tile_out) ceil(ntrials / trials_per_block).  mask may be NULL,
 * and so may any of the pointers behind nout.  0, or -1 when the table is not served, nout < 0 or the grid does not
 * hold the workgroups.  Needs no GPU. */
int rtlws_dedisp_geometry(int nchan, int ntrials, const int32_t* delays, const uint8_t* mask, long nout, int* blocks,
                          int* threads, int* lds_bytes, int* tile_out, int* trials_per_block, int* max_delay);

/* The table (ntrials * nchan int32) and the mask (nchan bytes or NULL), both in host memory and read before the call
 * returns, on the engine's device in the kernel's form, and the kernel loaded, so that rtlws_dedisp_run makes no
 * runtime call other than its launch and may be captured into a hipGraph.  A new table or mask is a new plan.  NULL
 * on failure (a null engine among them: without a device there is no engine, and no CPU path). */
rtlws_dedisp_plan* rtlws_dedisp_open(rtlws_engine* e, int nchan, int ntrials, const int32_t* delays, const uint8_t* mask);

/* Rows that nout outputs per trial read: nout + max_delay, 0 for nout == 0; -1 for a null plan or nout < 0. */
long rtlws_dedisp_rows_needed(const rtlws_dedisp_plan* p, long nout);

/* d_rows: rtlws_dedisp_rows_needed() rows of f32, 16-byte aligned; d_out: ntrials rows of nout f32.  Asynchronous on
 * `stream` (NULL = the engine's own stream, RTLWS_STREAM_DEFAULT = HIP's: "Streams" in rtlws_hip.h); one kernel launch
 * and no other runtime call.  nout == 0 does nothing.  Every refusal is made before the device is asked for anything:
 * nout, in_stride at least 4 and a multiple of 4, out_stride, null pointers, the two alignments, then a null plan,
 * then what the plan decides (in_stride >= nchan, the grid).  0; -1 bad argument; -3 HIP failure. */
int rtlws_dedisp_run(rtlws_dedisp_plan* p, const float* d_rows, long in_stride, long nout, float* d_out, long out_stride,
                     void* stream);

void rtlws_dedisp_close(rtlws_dedisp_plan* p);

/* Last error text of the calling thread from this library ("" when none). */
const char* rtlws_dedisp_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* RTLWS_DEDISP_H */
