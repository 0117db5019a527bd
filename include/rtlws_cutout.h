/*
 * rtlws_cutout.h -- cutouts of single-pulse candidates: for every candidate of the list that rtlws_sift_run
 * (rtlws_sift.h) leaves on the device, the band against time around the pulse, dedispersed at the candidate's trial
 * and summed into subbands and time bins, and the dedispersed series of the neighbouring trials against time (the
 * "bow tie"), in two launches that read the list where the sift left it (librtlws_cutout.so).
 *
 * DESIGN.md 4.31; tests/cutout_ref.py restates every word below in numpy.
 *
 *   S[j][i]    the waterfall as rtlws_dedisp_run reads it: f32 on the device, row j at d_rows + j * in_stride;
 *              nchan values a row, 4 .. 4096 and a multiple of 4
 *   mask[i]    bytes in host memory at open, optional (NULL: all ones); 0 leaves value i out of every sum
 *   d[t][i]    the table of the dedispersion that made the series: int32 in host memory at open, ntrials * nchan
 *              entries, each 0 .. 65535; ntrials 1 .. 4096 (the table and the rules of rtlws_dedisp_open)
 *   D[t][n]    the series rtlws_dedisp_run wrote, trial t at d_series + t * series_stride, nsamp long
 *   w_k        the pulse plan's widths: int32 table in host memory at open, strictly ascending, 1 .. 1024;
 *              K = nwidths 1 .. 16
 *   bin_k      rows per time bin for a candidate of width k: int32 table of K entries at open, each 1 .. 1024
 *   nx         time bins of a plane, 4 .. 256 and a multiple of 4
 *   nf         subbands of the band-time plane, 1 .. nchan, dividing nchan; cpb = nchan / nf
 *   rq, dq     the DM-time plane has ndm = 2 rq + 1 rows at trials t + (r - rq) dq; rq 0 .. 64, dq 1 .. 64
 *   nsamp      the outputs per trial of the dedispersion, 1 .. 2^30: rows 0 .. nsamp + max_delay - 1 exist (max_delay
 *              the largest table entry over the positions the mask keeps) and the series are nsamp long
 *   d_cand     the sift's list: candidate i is the eight 32-bit words at d_cand[8 i ..], of which word 0 (t), word 2
 *              (k) and word 3 (at) are read, as int32; a caller may write a list of its own in that form
 *   d_count    the sift's two counts; the candidates served are i = 0 .. min(d_count[0], max_cand) - 1, and it is the
 *              kernel that reads d_count[0], not the host; max_cand 1 .. 4096 sizes the grid and the outputs
 *
 * For candidate i = (t, k, at):  b = bin_k;  centre = at + w_k / 2 (integer division);  n0 = centre - (nx / 2) b, which
 * may be negative.  Bin x = 0 .. nx - 1 covers n = n0 + x b + j, j = 0 .. b - 1.  The candidate is valid when t is
 * 0 .. ntrials - 1, k is 0 .. K - 1 and at is 0 .. nsamp - 1.  rtlws_cutout_window states the rule on the host.
 *
 * The band-time plane, d_ft[(i * nf + f) * nx + x]:
 *   R[c][x]    = acc after:  acc = +0.0f;  for j = 0 .. b - 1 ascending:  n = n0 + x b + j;
 *                            if 0 <= n < nsamp: acc = fl(acc + S[n + d[t][c]][c])
 *   F[i][f][x] = acc after:  acc = +0.0f;  for c = f cpb .. (f + 1) cpb - 1 ascending: if mask[c]: acc = fl(acc + R[c][x])
 * The DM-time plane, d_dmt[(i * ndm + r) * nx + x]:
 *   G[i][r][x] = acc after:  acc = +0.0f;  q = t + (r - rq) dq;  if 0 <= q < ntrials: for j = 0 .. b - 1 ascending:
 *                            n = n0 + x b + j;  if 0 <= n < nsamp: acc = fl(acc + D[q][n])
 * d_info[4 i ..] = { n0, b, 1, the number of n of n0 .. n0 + nx b - 1 inside 0 .. nsamp - 1 }, four int32.
 * An invalid candidate's planes are +0.0 everywhere and its d_info is { 0, 0, 0, 0 }.
 *
 * One f32 rounding per addition, nothing contracted, time first and then ascending channel; the order depends on
 * nothing else, no atomic operation takes part and no workgroup waits for another: two runs give the same bytes.  An
 * accumulator starts at +0.0 and an addition never makes it -0.0, so:
 *   - with nf = 1 and b = 1, F[i][0][x] is D[t][n0 + x] of rtlws_dedisp_run bit for bit wherever n0 + x lies in
 *     0 .. nsamp - 1 (R is the sample itself but for -0.0, which leaves the sum as it is);
 *   - with b = 1, G[i][rq][x] is that same series value with -0.0 turned into +0.0.
 * Non-finite samples propagate as IEEE addition propagates them, into the one bin they fall in.
 *
 * A masked channel's rows are never read.  No row at or beyond nsamp + max_delay is read, no element of a row at or
 * beyond nchan, no sample of a series at or beyond nsamp.  d_ft (max_cand * nf * nx f32) and d_dmt (max_cand * ndm * nx
 * f32) may each be NULL, but not both; a NULL output's launch is not made, and what only it reads (d_rows for d_ft,
 * d_series for d_dmt) may be NULL with it.  d_info (max_cand * 4 int32) is always written for the served candidates.
 * Nothing is written behind the served candidates or outside the buffers: with d_count[0] = 0 nothing at all.
 *
 * The launches.  Band-time: a workgroup of 256 threads owns one candidate, a group of 32 time bins and whole subbands:
 * 256 / cpb of them where cpb <= 256, else one, walked in chunks of 256 channels with the running sums carried.  Lanes
 * run along channels; a lane adds its channel's b rows of every bin in a register and leaves R in a tile of LDS, and
 * behind one barrier thread (f, x) adds its subband's channels in ascending order.  DM-time: a workgroup a (candidate,
 * r), a thread a bin.  The candidate's words, n0, b and the clip of the window are scalars of the workgroup; the
 * workgroups of candidates at or beyond the count leave at once.  rtlws_cutout_geometry gives the figures.
 *
 * Refused with -1 (rtlws_cutout_last_error() says why), in this order: nchan outside 4 .. 4096 or not a multiple of 4,
 * ntrials outside 1 .. 4096, nwidths outside 1 .. 16, a null table of widths, a width outside 1 .. 1024 or not above
 * the one before, a null table of bins, a bin outside 1 .. 1024, nx outside 4 .. 256 or not a multiple of 4, nf outside
 * 1 .. nchan or not dividing nchan, rq outside 0 .. 64, dq outside 1 .. 64; then a null table of delays and a delay
 * outside 0 .. 65535; then what a run is given (rtlws_cutout_run).
 */
#ifndef RTLWS_CUTOUT_H
#define RTLWS_CUTOUT_H

#include <stdint.h>

#include "rtlws_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* librtlws_cutout.so exports these declarations and nothing else (exports/cutout.map) */
#pragma GCC visibility push(default)

#define RTLWS_CUTOUT_MIN_NCHAN 4
#define RTLWS_CUTOUT_MAX_NCHAN 4096
#define RTLWS_CUTOUT_MAX_TRIALS 4096
#define RTLWS_CUTOUT_MAX_DELAY 65535
#define RTLWS_CUTOUT_MAX_WIDTHS 16
#define RTLWS_CUTOUT_MAX_WIDTH 1024
#define RTLWS_CUTOUT_MAX_BIN 1024
#define RTLWS_CUTOUT_MIN_NX 4
#define RTLWS_CUTOUT_MAX_NX 256
#define RTLWS_CUTOUT_MAX_NF 4096
#define RTLWS_CUTOUT_MAX_RQ 64
#define RTLWS_CUTOUT_MAX_DQ 64
#define RTLWS_CUTOUT_MAX_NSAMP 1073741824
#define RTLWS_CUTOUT_MAX_CAND 4096
#define RTLWS_CUTOUT_CAND_WORDS 8
#define RTLWS_CUTOUT_INFO_WORDS 4

typedef struct rtlws_cutout_plan rtlws_cutout_plan;

/* 1 when the shape, the two tables of K entries and the planes' extents are served, else 0
 * (rtlws_cutout_last_error() says why).  Needs no GPU. */
int rtlws_cutout_supported(int nchan, int ntrials, int nwidths, const int32_t* widths, const int32_t* bins, int nx, int nf,
                           int rq, int dq);

/* What a plan of these arguments launches for max_cand candidates: workgroups, threads per workgroup and bytes of LDS
 * per workgroup of the two launches (band-time, DM-time: arrays of 2), ndm = 2 rq + 1, and the largest delay over the
 * positions the mask keeps (0 where it keeps none).  Band-time: max_cand * ceil(nx / 32) * ceil(nf / per) workgroups of
 * 256 threads, per = 256 / cpb subbands where cpb <= 256, else 1.  DM-time: max_cand * ndm workgroups of nx threads
 * rounded up to a multiple of 64, no LDS.  mask may be NULL, and so may any of the pointers behind max_cand.  0, or -1
 * for what the head of this file lists, max_cand outside 1 .. 4096 or more workgroups than one grid holds.  Needs no
 * GPU. */
int rtlws_cutout_geometry(int nchan, int ntrials, const int32_t* delays, const uint8_t* mask, int nwidths, const int32_t* widths,
                          const int32_t* bins, int nx, int nf, int rq, int dq, int max_cand, int* blocks, int* threads,
                          int* lds_bytes, int* ndm, int* max_delay);

/* The tables (delays ntrials * nchan int32, mask nchan bytes or NULL, widths and bins nwidths int32 each, all in host
 * memory and read before the call returns) on the engine's device as the kernels read them, and the kernels loaded, so
 * that rtlws_cutout_run makes no runtime call other than its launches and may be captured into a hipGraph.  NULL on
 * failure (a null engine among them: without a device there is no engine, and no CPU path). */
rtlws_cutout_plan* rtlws_cutout_open(rtlws_engine* e, int nchan, int ntrials, const int32_t* delays, const uint8_t* mask,
                                     int nwidths, const int32_t* widths, const int32_t* bins, int nx, int nf, int rq, int dq);

/* Rows of the waterfall that a run over series of nsamp outputs may read: nsamp + max_delay; -1 for nsamp outside
 * 1 .. 2^30 or a null plan. */
long rtlws_cutout_rows_needed(const rtlws_cutout_plan* p, long nsamp);

/* The window of a candidate at `at` of a boxcar of `width` samples in nx bins of `bin` rows: *n0 = at + width / 2 -
 * (nx / 2) bin, and *inside the number of n0 .. n0 + nx bin - 1 that lie in 0 .. nsamp - 1.  Either pointer may be NULL.
 * 0, or -1 for at < 0 or at >= nsamp, width or bin outside 1 .. 1024, nx outside 4 .. 256 or not a multiple of 4, or nsamp
 * outside 1 .. 2^30.  Needs no GPU. */
int rtlws_cutout_window(long at, int width, int bin, int nx, long nsamp, long* n0, long* inside);

/* d_rows: rtlws_cutout_rows_needed() rows of f32, 16-byte aligned; d_series: ntrials series of nsamp f32; d_cand and
 * d_count as rtlws_sift_run leaves them (d_cand 16-byte aligned); d_ft, d_dmt, d_info as the head of this file says.
 * Asynchronous on `stream` (NULL = the engine's own stream, RTLWS_STREAM_DEFAULT = HIP's: "Streams" in rtlws_hip.h);
 * one kernel launch for each of d_ft and d_dmt that is not NULL and no other runtime call.  Every refusal is made
 * before the device is asked for anything, in this order: nsamp outside 1 .. 2^30, max_cand outside 1 .. 4096,
 * in_stride below 4 or not a multiple of 4, series_stride below nsamp, d_ft and d_dmt both NULL, null pointers (d_cand,
 * d_count, d_info; d_rows with a d_ft, d_series with a d_dmt), the alignments (d_rows and d_cand 16 bytes; d_series,
 * d_count, d_ft, d_dmt and d_info 4), then a null plan, then what the plan decides (in_stride >= nchan, the grid).
 * 0; -1 bad argument; -3 HIP failure. */
int rtlws_cutout_run(rtlws_cutout_plan* p, const float* d_rows, long in_stride, const float* d_series, long series_stride,
                     long nsamp, const uint32_t* d_cand, const int32_t* d_count, int max_cand, float* d_ft, float* d_dmt,
                     int32_t* d_info, void* stream);

void rtlws_cutout_close(rtlws_cutout_plan* p);

/* Last error text of the calling thread from this library ("" when none). */
const char* rtlws_cutout_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* RTLWS_CUTOUT_H */
