/*
 * rtlws_sift.h -- the sift of single-pulse peaks: the peaks, places and moments that rtlws_pulse_run (rtlws_pulse.h)
 * leaves on the device become a short list of candidates -- the best width of every (trial, segment), what lies below a
 * threshold dropped, the neighbouring trials and segments in which one pulse shows up merged into one event with its
 * extent in trials -- in three launches, nothing copied in between (librtlws_sift.so).
 *
 * DESIGN.md 4.30; tests/sift_ref.py restates every word below in numpy.
 *
 *   peak[(t*K + k)*S + s]  f32 on the device, at[..] int32 in the same layout, mom[(t*S + s)*2 + {0, 1}] f64: what
 *                          rtlws_pulse_run writes; t = 0 .. T-1 trials, k = 0 .. K-1 widths, s = 0 .. S-1 segments
 *   w_k       the widths the peaks were made with: int32 table in host memory at open, strictly ascending, 1 .. 1024;
 *             K = nwidths 1 .. 16
 *   seg       outputs per segment, as the pulse plan's: 64 .. 1048576, a multiple of 4
 *   rt, rs    the radii of the box: 0 .. 32 trials, 0 .. 8 segments
 *   nout      outputs per trial and width of the pulse run, 1 .. 2^30; S = ceil(nout / seg), 1 .. 2^24
 *   threshold f32, not NaN (+Inf and -Inf are served);  max_cand 1 .. 2^24
 *
 * Stage 1, the score and the best width.  For event (t, s): len = min(seg, nout - s*seg), (q1, q2) = mom[t][s], and in
 * f64, one rounding per operation, nothing contracted:
 *     mean = q1 / len;   var = q2 / len - mean * mean;   snr_k = ((double) peak_k - w_k * mean) / sqrt(w_k * var)
 * score_k = (float) snr_k, one more rounding: the operations of rtlws_pulse_snr.  score_k is -Inf where len < 2, where
 * var is not above 0, where peak_k is -Inf or NaN, or where the result is NaN.  best = -Inf, k = 0, at = -1; for k
 * ascending: if score_k > best: (best, k, at) = (score_k, k, at_k).  E[t][s] = (best, k, at): ties go to the smaller k,
 * and an event every width of which scores -Inf is (-Inf, 0, -1).  No score is NaN.
 *
 * Stage 2, the local maxima.  Event a beats event b when a's score is greater, or the scores are equal (+0.0 equals
 * -0.0) and a has the smaller t, or scores and t are equal and a has the smaller s.  The box of (t, s) is the events
 * (t', s') with |t' - t| <= rt and |s' - s| <= rs inside the plane.  An event is a candidate when its score is
 * >= threshold and no other event of its box beats it.  It carries, over the events of its box whose score is
 * >= threshold (itself among them): members, their number; t_lo and t_hi, the least and the greatest t' among them.
 *
 * Stage 3, the list.  The candidates in ascending (s, t) order, time first, candidate i as eight 32-bit words at
 * d_cand[8*i ..]:
 *     { t, s, k, at, the bits of score, the bits of peak_k, members, (t_hi << 16) | t_lo }
 * d_count[0] is the number of candidates found; where it exceeds max_cand the first max_cand of the order are written
 * and nothing behind them.  d_count[1] is the number of events whose score is >= threshold.  d_score[t*S + s] (f32) and
 * d_k[t*S + s] (int32) are stage 1's plane, each written where its pointer is not NULL.  The run writes nothing else: no
 * word of d_cand behind the last candidate, nothing behind the planes.  No atomic operation takes part and no
 * workgroup waits for another: two runs give the same bytes.
 *
 * The launches.  Scoring: one thread an event, consecutive lanes consecutive s, the loop over k in registers, the
 * widths scalar loads; it writes the plane into the workspace.  The box: a workgroup of 256 threads owns a tile of
 * tile_t x tile_s = 64 x 64 events, stages their scores and a halo of rt x rs in LDS, walks the box of every event at
 * or above threshold, marks the candidates in the workspace and leaves the tile's count of every segment and its two
 * totals there.  The list: every workgroup with a candidate adds up the counts that precede its own -- the tiles of
 * the segments before its own by their totals, in blocks of 256, then its own 64 segments by tile -- and writes its
 * candidates; the last one writes d_count.  The order between workgroups comes from the launch boundaries alone.
 *
 * The workspace is the caller's: rtlws_sift_work_bytes bytes, 16-byte aligned, no content expected and none promised.
 *
 * Refused with -1 (rtlws_sift_last_error() says why): nwidths outside 1 .. 16, a null table, a width outside 1 .. 1024
 * or not above the one before, seg outside 64 .. 1048576 or not a multiple of 4, rt outside 0 .. 32, rs outside 0 .. 8,
 * ntrials outside 1 .. 65536, nout outside 1 .. 2^30 (0: there is no event to sift), a NaN threshold, max_cand outside
 * 1 .. 2^24, null pointers, d_cand or d_work not 16-byte aligned, d_mom not 8-byte aligned, the others not 4-byte
 * aligned, more than 2^31 - 1 events (ntrials * S) or more workgroups than one grid holds.
 */
#ifndef RTLWS_SIFT_H
#define RTLWS_SIFT_H

#include <stdint.h>

#include "rtlws_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* librtlws_sift.so exports these declarations and nothing else (exports/sift.map) */
#pragma GCC visibility push(default)

#define RTLWS_SIFT_MAX_WIDTHS 16
#define RTLWS_SIFT_MAX_WIDTH 1024
#define RTLWS_SIFT_MIN_SEG 64
#define RTLWS_SIFT_MAX_SEG 1048576
#define RTLWS_SIFT_MAX_TRIALS 65536
#define RTLWS_SIFT_MAX_NOUT 1073741824
#define RTLWS_SIFT_MAX_RT 32
#define RTLWS_SIFT_MAX_RS 8
#define RTLWS_SIFT_MAX_CAND 16777216
#define RTLWS_SIFT_CAND_WORDS 8

typedef struct rtlws_sift_plan rtlws_sift_plan;

/* 1 when the table, the segment length and the radii are served, else 0 (rtlws_sift_last_error() says why).  Needs no
 * GPU. */
int rtlws_sift_supported(int nwidths, const int32_t* widths, long seg, int rt, int rs);

/* What a plan of these launches for ntrials trials of nout outputs: workgroups, threads per workgroup and bytes of LDS
 * per workgroup of the three launches (scoring, the box, the list: arrays of 3), the tile's extent in trials and in
 * segments, and S = ceil(nout / seg).  Any of the pointers behind nout may be NULL.  0, or -1 when the table, seg or a
 * radius is not served, ntrials or nout is outside its range or the plane is more than one run holds.  Needs no GPU. */
int rtlws_sift_geometry(int nwidths, const int32_t* widths, long seg, int rt, int rs, int ntrials, long nout, int* blocks,
                        int* threads, int* lds_bytes, int* tile_t, int* tile_s, long* nseg);

/* The widths (nwidths int32 in host memory, read before the call returns) on the engine's device as the scoring reads
 * them, and the three kernels loaded, so that rtlws_sift_run makes no runtime call other than its launches and may be
 * captured into a hipGraph.  NULL on failure (a null engine among them: without a device there is no engine, and no CPU
 * path). */
rtlws_sift_plan* rtlws_sift_open(rtlws_engine* e, int nwidths, const int32_t* widths, long seg, int rt, int rs);

/* Bytes of the workspace of a run over ntrials trials of nout outputs; -1 for ntrials or nout outside its range, a
 * null plan, or a plane that is more than one run holds. */
long rtlws_sift_work_bytes(const rtlws_sift_plan* p, int ntrials, long nout);

/* d_peak, d_at: ntrials * nwidths * S f32 and int32; d_mom: ntrials * S * 2 f64; d_work: rtlws_sift_work_bytes() bytes;
 * d_cand: max_cand * 8 32-bit words; d_count: 2 int32; d_score, d_k: ntrials * S f32 and int32, or NULL.  Asynchronous on
 * `stream` (NULL = the engine's own stream, RTLWS_STREAM_DEFAULT = HIP's: "Streams" in rtlws_hip.h); three kernel
 * launches and no other runtime call.  Every refusal is made before the device is asked for anything, in this order:
 * ntrials, nout, a NaN threshold, max_cand, null pointers (d_peak, d_at, d_mom, d_work, d_cand, d_count), the
 * alignments (d_cand and d_work 16 bytes, d_mom 8, d_peak, d_at, d_count, d_score and d_k 4), then a null plan, then
 * what the plan decides (the events of the plane, the grid).  0; -1 bad argument; -3 HIP failure. */
int rtlws_sift_run(rtlws_sift_plan* p, const float* d_peak, const int32_t* d_at, const double* d_mom, int ntrials, long nout,
                   float threshold, int max_cand, void* d_work, uint32_t* d_cand, int32_t* d_count, float* d_score, int32_t* d_k,
                   void* stream);

void rtlws_sift_close(rtlws_sift_plan* p);

/* Last error text of the calling thread from this library ("" when none). */
const char* rtlws_sift_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* RTLWS_SIFT_H */
