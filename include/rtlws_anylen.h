/*
 * rtlws_anylen.h -- f64 power spectra of any frame length 2 .. 2^19 (librtlws_anylen.so).
 *
 * The reference plans an FFT of any length (src/spectrum.c:37-45).  rtlws_spectra_batch_f64 (rtlws_hip.h) serves a
 * length that is not a power of two with a direct O(N^2) sum and stops at 8192 points; rtlws_long.h serves the
 * powers of two above.  This header serves EVERY length with Bluestein's algorithm: an N-point DFT as a circular
 * convolution of length M = 2^m >= 2N - 1, done with the four-step power-of-two transform of rtlws_long.h
 * (DESIGN.md 4.11).  With w[n] = exp(-i pi n^2 / N): X[k] = w[k] * sum_n (x[n] w[n]) conj(w[k - n]), and because
 * |w[k]| = 1 the power |X[k]|^2 is the convolution's.  A frame costs two M-point transforms and a pointwise
 * product (the transform of the chirp is made once, at open).
 *
 * Like rtlws_long.h the interface is plan-based: open once, run many times, close.
 *
 * Descriptors served (anything else: rtlws_anylen_supported() == 0, rtlws_anylen_open() == NULL, the text says why):
 *   n_fft    2 .. 2^19, every integer (powers of two and primes included);
 *            M = max(2^14, the smallest power of two >= 2 n_fft - 1), so 2^14 <= M <= 2^20
 *   k_avg    >= 1
 *   input    RTLWS_IN_CU8, RTLWS_IN_CS32, RTLWS_IN_RF32
 *   window   RTLWS_WIN_RECT
 *   output   RTLWS_OUT_POWER_SUM, RTLWS_OUT_MEAN_DB, RTLWS_OUT_PAYLOAD_U8
 *   cic_r    0 or 1
 *   flags    0 or RTLWS_FLAG_ROWS_F32
 * Frame layout, row layout, dB and payload arithmetic are exactly those of rtlws_spectra_batch_f64 for that n_fft,
 * odd lengths included: slot i shows bin (n_fft/2 + i) mod n_fft; the slot that would show bin 0,
 * i0 = n_fft - n_fft/2, takes the running-sum rule of src/spectrum.c:25-33 instead (in closed form
 * sum_k (K - k) P_k[n_fft - 1]); its left neighbour i0 - 1 shows bin n_fft - 1.
 */
#ifndef RTLWS_ANYLEN_H
#define RTLWS_ANYLEN_H

#include "rtlws_long.h"

#ifdef __cplusplus
extern "C" {
#endif
/* librtlws_anylen.so exports these declarations and nothing else (exports/anylen.map) */
#pragma GCC visibility push(default)

typedef struct rtlws_anylen_plan rtlws_anylen_plan;

/* 1 when the descriptor is served, else 0 (rtlws_anylen_last_error() says why).  Needs no GPU. */
int rtlws_anylen_supported(const rtlws_spectra_desc* desc);

/* A plan for `desc` on the engine's device: the chirp w, the transform of its conjugate, the twiddle tables of
 * size M, two workspaces and the LDS opt-in of its four kernels.  The workspaces hold 2 * 16 * M bytes per frame
 * in flight, for min(max_frames rounded up to whole rows, what RTLWS_LONG_WORKSPACE_CAP holds) frames -- or for
 * one row's k_avg frames, if those need more: a larger batch runs as consecutive groups of whole rows on the
 * stream.  max_frames is the largest batch the caller expects; < 1 means one row.  Open transforms the chirp on
 * the device (engine's stream) and waits for it.
 * NULL on a bad descriptor, a null engine (no device: there is no CPU path) or a HIP failure. */
rtlws_anylen_plan* rtlws_anylen_open(rtlws_engine* e, const rtlws_spectra_desc* desc, long max_frames);

/* m of the convolution length M = 2^m the descriptor's n_fft runs at, -1 if the descriptor is not served.
 * Needs no GPU. */
int rtlws_anylen_conv_log2(const rtlws_spectra_desc* desc);

/* Bytes of device memory the plan's two workspaces occupy together (0 for NULL). */
size_t rtlws_anylen_workspace_bytes(const rtlws_anylen_plan* plan);

/* d_in: nframes * n_fft input samples, frame after frame without padding; d_out: nframes / k_avg rows of n_fft
 * doubles (floats with RTLWS_FLAG_ROWS_F32, bytes for RTLWS_OUT_PAYLOAD_U8); device memory.  d_in needs only its
 * sample's alignment (2 bytes for cmplx_u8 -- an odd-length frame starts on a 2-byte boundary --, 8 for cmplx_s32,
 * 4 for real f32), d_out 8 bytes (4 for f32 rows and payload bytes); nothing is read behind the last frame or
 * written behind the last row.  nframes a multiple of k_avg, 0 allowed.  Asynchronous on `stream` (NULL = the
 * engine's own stream, RTLWS_STREAM_DEFAULT = HIP's: "Streams" in rtlws_hip.h).  It enqueues kernels -- four per
 * group, a linear chain -- and makes no other runtime call, so it may be captured into a hipGraph.  Launches of
 * one plan share its workspaces: they must be ordered (one stream, or events).
 * 0; -1 bad argument; -3 HIP failure. */
int rtlws_anylen_run(rtlws_anylen_plan* plan, const void* d_in, long nframes, void* d_out, void* stream);

/* Frees the tables and the workspaces (after the caller has synchronised the streams it ran on). */
void rtlws_anylen_close(rtlws_anylen_plan* plan);

/* Last error text of the calling thread from this library ("" when none). */
const char* rtlws_anylen_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* RTLWS_ANYLEN_H */
