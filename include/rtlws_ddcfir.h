/*
 * rtlws_ddcfir.h -- tuned channels with a real channel filter: a bank of digital down-converters whose decimating
 * filter is an int16 FIR of up to 256 taps (librtlws_ddcfir.so).
 *
 * rtlws_ddc_run (rtlws_ddc.h) filters a channel with the CIC block sum of R samples and nothing else: a tone 1.5
 * output bandwidths off a channel's centre comes through at -13.2 dB.  rtlws_ddcfir_run moves up to
 * RTLWS_DDCFIR_MAX_CHANNELS bands of one device-resident cmplx_u8 capture to DC, filters each with the plan's taps
 * h[0 .. L - 1] and decimates by R = decim, in ONE launch.  The channels lie at any offset (a tuning word of
 * rtlws_ddc_tuning_word each), R is any factor 1 .. 128 and L any length 1 .. 256: the windows of consecutive outputs
 * overlap when L > R.  The output is the cmplx_s32 stream that rtlws_fm_audio_blocks and RTLWS_IN_CS32 spectra consume.
 *
 * The arithmetic is all-integer and every output integer is defined (tests/ddcfir_ref.py restates it
 * in numpy).  P = 2^16 and T[j] are rtlws_ddc.h's period and phasor table (rtlws_ddc_table), k a channel's tuning word
 * in [-P/2, P/2), s = out_shift, x the capture, m = 0 .. dec_len - 1 and g = first_dec_index + m:
 *   a_n = re[m R + n] - 128,  b_n = im[m R + n] - 128                (n = 0 .. L - 1)
 *   (c_n, s_n) = T[(k n) mod P]
 *   Gc_n = (h[n] c_n + 2^13) >> 14    Gs_n = (h[n] s_n + 2^13) >> 14   (arithmetic shift; |G| <= |h[n]|)
 *   Ur = sum_n a_n Gc_n + b_n Gs_n    Ui = sum_n b_n Gc_n - a_n Gs_n   (int32)
 *   (Cb, Sb) = T[(k R g) mod P]
 *   Vr = Ur Cb + Ui Sb                Vi = Ui Cb - Ur Sb               (int64)
 *   out[c][m] = ((Vr + r) >> (14 + s), (Vi + r) >> (14 + s)),  r = 2^(13 + s)
 * The capture holds rtlws_ddcfir_samples_needed = (dec_len - 1) R + L samples and no byte beyond them is read.  The
 * total phase k (g R + n) depends on absolute sample time only and nothing is carried between calls: chunked calls
 * that overlap by L - R samples and pass first_dec_index concatenate to one call's integers.  L = R, h = 16384
 * throughout and s = 14 is rtlws_ddc_run bit for bit (G = T); a capture of 128s gives zeros.
 *
 * Taps lie in [-RTLWS_DDCFIR_MAX_TAP, RTLWS_DDCFIR_MAX_TAP] = [-32639, 32639]: the kernel multiplies by G as two int8
 * operands, G = 256 Gh + Gl with Gl in [-128, 127], and 32640 = 256 * 128 - 128 is the first value whose Gh leaves
 * int8.  rtlws_ddcfir_open refuses a tap outside.  With that limit and L <= 256 nothing overflows at any s:
 *   |U|   <= 128 (sqrt(2) sum|h| + 2 L) < 1.52e9 < 2^31
 *   |out| <= 182 (sum|h| + L) / 2^s + 1 < 2^31
 * Every component lies within  0.5 + sqrt(2) (sum|h| / 128 + 128 L + 182 (sum|h| + L) / 2^15) / 2^s  of the ideal
 * 2^-s sum_n h[n] (x[m R + n] - 128 (1 + i)) exp(-2 pi i k (g R + n) / P)  (DESIGN.md 4.12a derives it).
 *
 * Refused with -1 (rtlws_ddcfir_last_error() says why): decim outside 1 .. 128, ntaps outside 1 .. 256, nchannels
 * outside 1 .. 32, a tap outside the limit, out_shift outside 0 .. 30, a tuning word outside [-P/2, P/2), dec_len < 0
 * or more than one grid holds, first_dec_index < 0, out_stride < dec_len, d_iq_cu8 not 16-byte or d_out_cs32 not 8-byte
 * aligned, null pointers.
 */
#ifndef RTLWS_DDCFIR_H
#define RTLWS_DDCFIR_H

#include <stdint.h>

#include "rtlws_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* librtlws_ddcfir.so exports these declarations and nothing else (exports/ddcfir.map) */
#pragma GCC visibility push(default)

#define RTLWS_DDCFIR_MAX_CHANNELS 32
#define RTLWS_DDCFIR_MAX_DECIM 128
#define RTLWS_DDCFIR_MAX_TAPS 256
#define RTLWS_DDCFIR_MAX_TAP 32639
#define RTLWS_DDCFIR_MAX_SHIFT 30

typedef struct rtlws_ddcfir_plan rtlws_ddcfir_plan;

/* 1 when the shape is served, else 0 (rtlws_ddcfir_last_error() says why).  Needs no GPU. */
int rtlws_ddcfir_supported(int decim, int ntaps, int nchannels);

/* Samples of the capture a run of dec_len outputs reads: (dec_len - 1) * decim + ntaps, 0 for dec_len == 0; -1 when
 * the shape is not served.  Needs no GPU. */
long rtlws_ddcfir_samples_needed(int decim, int ntaps, long dec_len);

/* Launch geometry of a served shape: workgroups (one per tile of tile_dec consecutive decimated samples of every
 * channel), threads per workgroup, bytes of LDS per workgroup (the filter's operands: 1 KiB per eight channels and 16
 * taps).  Any pointer may be NULL.  0, or -1 when the shape is not served.  Needs no GPU. */
int rtlws_ddcfir_grid(int decim, int ntaps, int nchannels, long dec_len, int* blocks, int* threads, int* lds_bytes,
                      int* tile_dec);

/* A low-pass for decimation by decim: a Hamming-windowed sinc with its cutoff at +-1 / (2 decim) cycles per sample.
 * With L = ntaps,
 *   p[n]    = sinc((n - (L - 1) / 2) / decim) * (0.54 - 0.46 cos(2 pi n / (L - 1)))     (sinc(x) = sin(pi x) / (pi x);
 *                                                                                        L = 1: p[0] = 1)
 *   A       = min(16384 decim / sum_n p[n], RTLWS_DDCFIR_MAX_TAP / max_n |p[n]|)
 *   taps[n] = rint(A p[n])                                                              (in double, ties to even)
 * The first term of A gives the filter the CIC's own DC gain at out_shift = 14 (sum taps = 16384 decim but for the
 * taps' rounding, what rtlws_fm_audio_blocks has been fed by rtlws_ddc_run); the second holds every tap inside the
 * limit where the first would not (short filters: ntaps below about 1.2 decim), at a lower gain.  0; -1 for a shape
 * that is not served or a null pointer.  Host only, needs no GPU. */
int rtlws_ddcfir_design(int decim, int ntaps, int16_t* taps);

/* *bound = 0.5 + sqrt(2) (sum|taps| / 128 + 128 ntaps + 182 (sum|taps| + ntaps) / 2^15) / 2^out_shift: how far a
 * component of the output lies from the ideal mixer and filter at most (above), for a caller who
 * chooses out_shift against the precision they need.  0; -1 for ntaps outside 1 .. 256, out_shift outside 0 .. 30 or a
 * null pointer.  Host only, needs no GPU. */
int rtlws_ddcfir_bound(int ntaps, const int16_t* taps, int out_shift, double* bound);

/* The taps (ntaps int16 in host memory, copied) and T on the engine's device and the plan's kernel loaded, so that
 * rtlws_ddcfir_run makes no runtime call other than its launch and may be captured into a hipGraph.  NULL on failure
 * (a null engine among them: without a device there is no engine, and no CPU path; a tap outside
 * +-RTLWS_DDCFIR_MAX_TAP: see above). */
rtlws_ddcfir_plan* rtlws_ddcfir_open(rtlws_engine* e, int decim, int ntaps, const int16_t* taps);

/* d_iq_cu8: rtlws_ddcfir_samples_needed cmplx_u8, 16-byte aligned.  d_out_cs32: channel-major, channel c is the
 * contiguous stream of dec_len cmplx_s32 at d_out_cs32 + c * out_stride samples (8-byte aligned, out_stride >=
 * dec_len); nothing outside [c * out_stride, c * out_stride + dec_len) is written.  tuning_words: nchannels ints in
 * host memory (rtlws_ddc_tuning_word makes them), read before the call returns: they travel in the kernel's
 * arguments, a retune is the next call.  out_shift = s, 0 .. 30.  Asynchronous on `stream` (NULL = the engine's own
 * stream, RTLWS_STREAM_DEFAULT = HIP's: "Streams" in rtlws_hip.h); one kernel launch and no other runtime call.
 * decim and ntaps both multiples of four is a compile-time instantiation (8-byte operand loads).  dec_len == 0 does
 * nothing.  Refusals come in rtlws_pfb_run's order: what needs no plan (every argument rule above), then a null plan; the
 * plan's shape (decim, ntaps) adds no rule of its own, every plan serves every count and shift.
 * 0; -1 bad argument; -3 HIP failure. */
int rtlws_ddcfir_run(rtlws_ddcfir_plan* p, const void* d_iq_cu8, long dec_len, long first_dec_index, int nchannels,
                     const int* tuning_words, int out_shift, void* d_out_cs32, long out_stride, void* stream);

void rtlws_ddcfir_close(rtlws_ddcfir_plan* p);

/* Last error text of the calling thread from this library ("" when none). */
const char* rtlws_ddcfir_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* RTLWS_DDCFIR_H */
