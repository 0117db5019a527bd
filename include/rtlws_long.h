/*
 * rtlws_long.h -- f64 power spectra of frames longer than 8192 points (librtlws_long.so).
 *
 * rtlws_spectra_batch_f64 (rtlws_hip.h) keeps one frame in the LDS of one compute unit and therefore stops at
 * 8192 points.  The reference plans an FFT of any length (src/spectrum.c:37-45); this header serves the
 * power-of-two lengths 2^14 .. 2^20 with a four-step transform through device memory: N = N1 * N2, a pass of
 * N1-point transforms into a workspace of complex doubles, then a pass of N2-point transforms that ends in the
 * same |X|^2, K-frame sums, fft-shift, DC-slot rule and epilogues as rtlws_spectra_batch_f64.
 *
 * The transform needs twiddle tables and that workspace, and a launch must allocate nothing, so the interface
 * is plan-based: open once, run many times, close.
 *
 * Descriptors served (anything else: rtlws_long_supported() == 0, rtlws_long_open() == NULL, the text says why):
 *   n_fft    2^m, 14 <= m <= 20
 *   k_avg    >= 1
 *   input    RTLWS_IN_CU8, RTLWS_IN_CS32, RTLWS_IN_RF32
 *   window   RTLWS_WIN_RECT
 *   output   RTLWS_OUT_POWER_SUM, RTLWS_OUT_MEAN_DB, RTLWS_OUT_PAYLOAD_U8
 *   cic_r    0 or 1
 *   flags    0 or RTLWS_FLAG_ROWS_F32
 * Frame layout, row layout, the DC-slot rule (slot n_fft/2 shows bin n_fft-1 with the running-sum weights of
 * src/spectrum.c:25-33), dB and payload arithmetic are exactly those of rtlws_spectra_batch_f64.
 */
#ifndef RTLWS_LONG_H
#define RTLWS_LONG_H

#include "rtlws_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* librtlws_long.so exports these declarations and nothing else (exports/long.map) */
#pragma GCC visibility push(default)

typedef struct rtlws_long_plan rtlws_long_plan;

/* The workspace of a plan holds 16 * n_fft bytes per frame in flight.  It is capped at this many bytes -- or
 * at one row's k_avg frames, if those need more: a batch of more frames than the workspace holds is run as
 * consecutive groups of whole rows on the stream. */
#define RTLWS_LONG_WORKSPACE_CAP ((size_t)1 << 30)

/* 1 when the descriptor is served, else 0 (rtlws_long_last_error() says why).  Needs no GPU. */
int rtlws_long_supported(const rtlws_spectra_desc* desc);

/* A plan for `desc` on the engine's device: the twiddle tables, a workspace for
 * min(max_frames rounded up to whole rows, the cap above) frames, and the LDS opt-in of its two kernels.
 * max_frames is the largest batch the caller expects (larger ones still run, in groups); < 1 means one row.
 * NULL on a bad descriptor, a null engine (no device: there is no CPU path) or a HIP failure. */
rtlws_long_plan* rtlws_long_open(rtlws_engine* e, const rtlws_spectra_desc* desc, long max_frames);

/* Bytes of device memory the plan's workspace occupies (0 for NULL). */
size_t rtlws_long_workspace_bytes(const rtlws_long_plan* plan);

/* d_in: nframes * n_fft input samples; d_out: nframes / k_avg rows of n_fft doubles (floats with
 * RTLWS_FLAG_ROWS_F32, bytes for RTLWS_OUT_PAYLOAD_U8); device memory, d_in 8-byte aligned, d_out 8-byte
 * (4-byte for f32 rows and payload bytes); nframes a multiple of k_avg, 0 allowed.  Asynchronous on `stream`
 * (NULL = the engine's own stream, RTLWS_STREAM_DEFAULT = HIP's: "Streams" in rtlws_hip.h).  It enqueues kernels
 * and makes no other runtime call, so it may be captured into a hipGraph.  Launches of one plan share its
 * workspace: they must be ordered (one stream, or events).  0; -1 bad argument; -3 HIP failure. */
int rtlws_long_run(rtlws_long_plan* plan, const void* d_in, long nframes, void* d_out, void* stream);

/* Frees the tables and the workspace (after the caller has synchronised the streams it ran on). */
void rtlws_long_close(rtlws_long_plan* plan);

/* Last error text of the calling thread from this library ("" when none). */
const char* rtlws_long_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* RTLWS_LONG_H */
