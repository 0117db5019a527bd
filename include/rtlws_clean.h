/*
 * rtlws_clean.h -- cleaning of a waterfall between the stage that writes it and the searches that read it: per block of
 * rows, every channel's mean and standard deviation, the channels whose statistics lie off the block's medians flagged,
 * the kept channels normalised to zero mean and unit variance, and (on request) the mean over the kept channels taken
 * off every row -- the zero-DM filter (librtlws_clean.so).
 *
 * rtlws_pfbspec_run, rtlws_pfbsk_run and rtlws_cdd_run write a time-major f32 waterfall; rtlws_dedisp_run, rtlws_cand_fold_run
 * and everything behind them read it as it was written.  This library reads it twice and writes it once (DESIGN.md 4.28;
 * tests/clean_ref.py restates it as plain loops).
 *
 *   M = nchan          4 .. 4096, a multiple of 4
 *   B = block_rows     32 .. 16384 (the plan's)
 *   S[j][i]            f32 on the device, row j at d_rows + j * in_stride; j = 0 .. nrows-1; B <= nrows <= 2^24
 *   mask[i]            bytes in host memory at open, optional (NULL: all ones)
 *   t_mean, t_sigma    doubles at open, >= 0 or +Inf (+Inf: that test is not made); NaN or negative refused
 *   flags              RTLWS_CLEAN_ZERODM = 1
 *
 *   nblocks = ceil(nrows / B); block b owns rows b*B .. min((b+1)*B, nrows) - 1;
 *   its statistics window is the B rows from j0 = min(b*B, nrows - B)   (the last block looks back; every row lies in
 *   its block's window)
 *
 *   Stage 1, per (b, i):
 *     x_k = (double) S[j0 + k][i], k = 0 .. B-1
 *     q1[r] = sum x_k, q2[r] = sum x_k * x_k over k == r (mod 8), ascending k, f64 from +0.0, r = 0 .. 7
 *     for h = 4, 2, 1: q[r] = q[r] + q[r + h], r < h;   s1 = q1[0], s2 = q2[0]
 *     mu = s1 / B;  var = fl(fl(s2 / B) - fl(mu * mu));  sd = sqrt(var);  m = (float) mu;  r = (float)(1.0 / sd)
 *     valid = mask[i] and s1, s2 finite and var > 0 and r finite
 *
 *   Stage 2, per b:  V = { i : valid };  med(X) = element floor((|X| - 1) / 2) of X in ascending order (an element: no
 *     arithmetic)
 *     med_mu = med{mu_i : V},  mad_mu = med{|mu_i - med_mu| : V};  the same for sd
 *     keep[b][i] = valid and (t_mean  == +Inf or |mu_i - med_mu| <= fl(t_mean  * mad_mu))
 *                        and (t_sigma == +Inf or |sd_i - med_sd| <= fl(t_sigma * mad_sd))
 *     nkept[b] = number kept.   V empty: nothing kept.   (thresholds are in MADs; 1.4826 MAD = 1 sigma for a normal)
 *
 *   Stage 3, per row j of block b:
 *     v_i = keep ? fl(fl(S[j][i] - m_i) * r_i) : +0.0f                      (f32, two roundings)
 *     without ZERODM: out[j][i] = v_i
 *     with ZERODM:    g_q = fl(fl(fl(v_4q + v_4q+1) + v_4q+2) + v_4q+3), q < M/4; g_q = +0.0f up to G = the power of two >= M/4
 *                     for h = G/2 .. 1: g[q] = fl(g[q] + g[q + h]), q < h
 *                     z = fl(g[0] / (float) nkept[b]);  out[j][i] = keep ? fl(v_i - z) : +0.0f;   nkept[b] == 0: the row is
 *                     +0.0f and no division is made
 *
 * Outputs, and nothing else is written: row j of the cleaned waterfall, the first M elements at d_out + j * out_stride;
 * d_keep uint8 [nblocks][M]; d_stats f32 [nblocks][M][2] holding (m, r), or (0, 0) where the channel is not valid;
 * d_nkept int32 [nblocks].  The last three may each be NULL.  Strides are in elements.  d_out == d_rows with equal
 * strides cleans in place: stage 1 has read every window before stage 3 writes a row.
 *
 * - Nothing depends on the grid and no atomics take part: two runs give the same bits.
 * - A run over the rows from b0 * B on gives blocks b0 .. of the whole run bit for bit (every window lies at or behind
 *   its block's first row or, for the last block, ends at the last row).
 * - A flagged channel is written as +0.0f.  rtlws_dedisp_run's accumulator starts at +0.0f and can never become -0.0f, so
 *   dedispersing the cleaned rows with no mask gives the bits of dedispersing them with keep[b] as the mask.
 * - A product of two f32 is exact in f64, so the residue classes and the tree define every bit of s1 and s2.  mu is never
 *   -0.0 and sd and the deviations are never negative zero: equal values have equal bits, and the element a median picks
 *   does not depend on how the sort orders equal ones.
 * - A non-finite sample makes its channel invalid in the blocks whose window holds it, and only there.  A constant channel
 *   has var <= 0 and is invalid.
 * - With ZERODM the f64 sum of a row's outputs is within (6 + log2 G) 2^-24 sum|v_i| of zero, to first order: the row's
 *   mean over the kept channels is gone (DESIGN.md 4.28 derives the constant).
 * - A finite threshold with a MAD of zero keeps only the channels whose statistic equals the median.
 *
 * The plan owns the workspace between the stages: 16 bytes per (block, channel) and 4 per block, allocated at open for
 * the most blocks one run may have, min(ceil(2^24 / B), 2^22 / M) -- 64 MiB at the most.  A waterfall of more blocks is
 * cleaned in pieces of whole blocks, which by the second property gives the bits of one run, save that every piece's
 * last block looks back inside the piece.  rtlws_clean_geometry says what a run launches.  Stage 1 has
 * nblocks * ceil(M / 256) workgroups of 512 threads, each reading its 256 channels of B rows once: a waterfall of few
 * blocks leaves most of the device idle during stage 1 (at M = 1024 eight blocks are 32 workgroups on 256 compute units),
 * and since one wavefront adds a residue's rows in order, halving B does not shorten a workgroup's work per row.  Choose
 * B so that nblocks * M / 256 is some hundreds where the time matters.
 *
 * Refused with -1 (rtlws_clean_last_error() says why): nchan outside 4 .. 4096 or not a multiple of 4, block_rows outside
 * 32 .. 16384, a threshold that is negative or NaN, unknown flag bits, nrows outside 0 .. 2^24 or between 1 and B - 1,
 * a stride below nchan or not a multiple of 4, null d_rows or d_out, d_rows or d_out not 16-byte aligned, d_out
 * overlapping d_rows in any other way than d_out == d_rows with equal strides, d_stats or d_nkept not 4-byte aligned,
 * more blocks than the workspace holds, more workgroups than one grid holds.
 */
#ifndef RTLWS_CLEAN_H
#define RTLWS_CLEAN_H

#include <stdint.h>

#include "rtlws_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* librtlws_clean.so exports these declarations and nothing else (exports/clean.map) */
#pragma GCC visibility push(default)

#define RTLWS_CLEAN_MIN_NCHAN 4
#define RTLWS_CLEAN_MAX_NCHAN 4096
#define RTLWS_CLEAN_MIN_BLOCK 32
#define RTLWS_CLEAN_MAX_BLOCK 16384
#define RTLWS_CLEAN_MAX_NROWS 16777216
#define RTLWS_CLEAN_MAX_CELLS 4194304
#define RTLWS_CLEAN_ZERODM 1

typedef struct rtlws_clean_plan rtlws_clean_plan;

/* 1 when the channel count and the block length are served, else 0 (rtlws_clean_last_error() says why).  Needs no GPU. */
int rtlws_clean_supported(int nchan, long block_rows);

/* What a plan launches for nrows rows (0, or B .. 2^24): the workgroups, the threads per workgroup and the bytes of LDS
 * per workgroup of the three launches in their order (three ints each), nblocks = ceil(nrows / B), and the bytes of the
 * workspace this run uses (the plan allocates for max_blocks = min(ceil(2^24 / B), 2^22 / M) blocks).
 *   stage 1: nblocks * ceil(M / 256) workgroups, 512 threads, 32768 bytes
 *   stage 2: nblocks workgroups, P / 2 threads within 64 .. 1024 (P the power of two >= M), 16 P + 128 bytes
 *   stage 3: a row takes G lanes (G the power of two >= M / 4), a workgroup T = max(256, G) threads and 16 T / G rows:
 *            nblocks * ceil(B / (16 T / G)) workgroups, T threads, 8 T bytes where G > 64 and none below
 * Any of the pointers may be NULL.  0, or -1 when nchan or block_rows is not served, nrows is outside its range, the
 * workspace does not hold the blocks or a grid does not hold the workgroups.  Needs no GPU. */
int rtlws_clean_geometry(int nchan, long block_rows, long nrows, int* blocks, int* threads, int* lds_bytes, long* nblocks,
                         long* workspace_bytes, long* max_blocks);

/* The mask (nchan bytes in host memory, read before the call returns; NULL: all ones) on the engine's device, the
 * workspace allocated and the three kernels loaded, so that rtlws_clean_run makes no runtime call other than its three
 * launches and may be captured into a hipGraph.  NULL on failure (a null engine among them: without a device there is no
 * engine, and no CPU path); the arguments are judged before the engine. */
rtlws_clean_plan* rtlws_clean_open(rtlws_engine* e, int nchan, long block_rows, const uint8_t* mask, double t_mean, double t_sigma,
                                   int flags);

/* ceil(nrows / B); -1 for a null plan or nrows outside 0 .. 2^24. */
long rtlws_clean_blocks(const rtlws_clean_plan* p, long nrows);

/* d_rows: nrows rows of nchan f32, in_stride apart, 16-byte aligned; d_out the same with out_stride; d_keep, d_stats,
 * d_nkept as above or NULL.  Asynchronous on `stream` (NULL = the engine's own stream, RTLWS_STREAM_DEFAULT = HIP's:
 * "Streams" in rtlws_hip.h); three kernel launches and no other runtime call.  nrows == 0 does nothing.  Every refusal is
 * made before the device is asked for anything, in this order: nrows within 0 .. 2^24, in_stride then out_stride at
 * least 4 and a multiple of 4, null pointers (d_rows, d_out), the alignments of d_rows, d_out, d_stats and d_nkept, then a
 * null plan, then what the plan decides: both strides at least nchan, nrows at least B, the overlap of d_out and d_rows,
 * the blocks the workspace holds, the grid.  0; -1 bad argument; -3 HIP failure. */
int rtlws_clean_run(rtlws_clean_plan* p, const float* d_rows, long in_stride, long nrows, float* d_out, long out_stride, uint8_t* d_keep,
                    float* d_stats, int32_t* d_nkept, void* stream);

/* The one mask rtlws_dedisp_open and rtlws_cand_fold_open take, from the flags of a run (keep: nblocks * nchan bytes in
 * host memory): mask_out[i] = 1 when the blocks that keep channel i are at least min_share of all, that is when
 * (double) count_i >= fl(min_share * (double) nblocks), else 0.  min_share 0 keeps everything, 1 only the channels every
 * block keeps.  -1: null pointers, nblocks < 1, nchan outside 4 .. 4096 or not a multiple of 4, min_share outside 0 .. 1
 * or NaN.  Needs no GPU. */
int rtlws_clean_union_mask(const uint8_t* keep, long nblocks, int nchan, double min_share, uint8_t* mask_out);

void rtlws_clean_close(rtlws_clean_plan* p);

/* Last error text of the calling thread from this library ("" when none). */
const char* rtlws_clean_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* RTLWS_CLEAN_H */
