/*
 * rtlws_ddc.h -- tuned channels from one capture: a bank of digital down-converters (librtlws_ddc.so).
 *
 * Everything else downstream of a capture listens at offset 0 of the captured band (rtlws_cic_block_sums,
 * rtlws_fm_audio_blocks*, rtlws_spectra_batch* with cic_r); the reference tunes by retuning the dongle
 * (rtl_set_frequency), one station per capture.  rtlws_ddc_run moves up to RTLWS_DDC_MAX_CHANNELS bands of one
 * device-resident cmplx_u8 capture to DC and decimates each by cic_r in ONE launch that reads the capture once:
 * 2 * cic_r bytes in and 8 bytes out per channel and decimated sample.  The output is the cmplx_s32 stream that
 * rtlws_fm_audio_blocks and RTLWS_IN_CS32 spectra consume, at the CIC's own gain (cic_r).
 *
 * The arithmetic is all-integer and every output integer is defined (tests/ddc_ref.py restates
 * it in numpy).  P = 2^RTLWS_DDC_LOG2_PERIOD is the phase period, S = 2^14 the phasor scale,
 *   T[j] = (rint(S cos(2 pi j / P)), rint(S sin(2 pi j / P)))  as int16, j = 0 .. P - 1   (rtlws_ddc_table).
 * A channel has a tuning word k, an integer in [-P/2, P/2): the band centred at k / P cycles per input sample.
 * With x[n] = (re, im) the capture, R = cic_r, m = 0 .. dec_len - 1 and g = first_dec_index + m:
 *   a_n = re[m R + n] - 128,  b_n = im[m R + n] - 128                (n = 0 .. R - 1)
 *   (c_n, s_n) = T[(k n) mod P]
 *   Ur = sum_n a_n c_n + b_n s_n      Ui = sum_n b_n c_n - a_n s_n     (int32: |U| <= R * 128 * 23170 < 2^31)
 *   (C, Sn) = T[(k R g) mod P]
 *   Vr = Ur C + Ui Sn                 Vi = Ui C - Ur Sn                (int64)
 *   out[m] = ((Vr + 2^27) >> 28, (Vi + 2^27) >> 28)                    (arithmetic shift)
 * k = 0 is rtlws_cic_block_sums exactly.  Every component lies within 0.5 + R / 64 of the ideal mixer and block
 * sum.  The block phasor depends on the absolute index g only: chunked calls that pass first_dec_index
 * concatenate to what one call gives, and no state is carried between calls.
 *
 * Refused with -1 (rtlws_ddc_last_error() says why): cic_r outside 1 .. 128, nchannels outside 1 .. 32, a tuning
 * word outside [-P/2, P/2), dec_len < 0 or more than one grid holds, first_dec_index < 0, out_stride < dec_len,
 * d_iq_cu8 not 16-byte or d_out_cs32 not 8-byte aligned, null pointers.
 */
#ifndef RTLWS_DDC_H
#define RTLWS_DDC_H

#include <stdint.h>

#include "rtlws_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* librtlws_ddc.so exports these declarations and nothing else (exports/ddc.map) */
#pragma GCC visibility push(default)

#define RTLWS_DDC_LOG2_PERIOD 16
#define RTLWS_DDC_MAX_CHANNELS 32

typedef struct rtlws_ddc_plan rtlws_ddc_plan;

/* 1 when the shape is served, else 0 (rtlws_ddc_last_error() says why).  Needs no GPU. */
int rtlws_ddc_supported(int cic_r, int nchannels);

/* T as the library builds it: 2 * P int16, (cos, sin) interleaved.  0, or -1 for a null pointer.  Needs no GPU. */
int rtlws_ddc_table(int16_t* cos_sin);

/* *word = rint(offset_hz / sample_rate_hz * P) wrapped into [-P/2, P/2).  0; -1 for sample_rate_hz <= 0, a
 * non-finite argument or a null pointer.  Needs no GPU. */
int rtlws_ddc_tuning_word(double offset_hz, double sample_rate_hz, int* word);

/* T on the engine's device and the library's kernels loaded, so that rtlws_ddc_run makes no runtime call other
 * than its launch and may be captured into a hipGraph.  NULL on failure (a null engine among them: without a
 * device there is no engine, and no CPU path). */
rtlws_ddc_plan* rtlws_ddc_open(rtlws_engine* e);

/* Launch geometry of a served shape: workgroups (one per tile of tile_dec consecutive decimated samples of every
 * channel), threads per workgroup, bytes of LDS per workgroup.  Any pointer may be NULL.  0, or -1 when the
 * shape is not served.  Needs no GPU. */
int rtlws_ddc_grid(int cic_r, int nchannels, long dec_len, int* blocks, int* threads, int* lds_bytes, int* tile_dec);

/* d_iq_cu8: dec_len * cic_r cmplx_u8, 16-byte aligned.  d_out_cs32: channel-major, channel c is the contiguous
 * stream of dec_len cmplx_s32 at d_out_cs32 + c * out_stride samples (8-byte aligned, out_stride >= dec_len);
 * nothing outside [c * out_stride, c * out_stride + dec_len) is written.  tuning_words: nchannels ints in host
 * memory, read before the call returns: they travel in the kernel's arguments, a retune is the next call.
 * Asynchronous on `stream` (NULL = the engine's own stream, RTLWS_STREAM_DEFAULT = HIP's: "Streams" in
 * rtlws_hip.h); one kernel launch and no other runtime call.  cic_r = 8, 10 and 12 are compile-time
 * instantiations.  dec_len == 0 does nothing.  0; -1 bad argument; -3 HIP failure. */
int rtlws_ddc_run(rtlws_ddc_plan* p, int cic_r, const void* d_iq_cu8, long dec_len, long first_dec_index,
                  int nchannels, const int* tuning_words, void* d_out_cs32, long out_stride, void* stream);

void rtlws_ddc_close(rtlws_ddc_plan* p);

/* Last error text of the calling thread from this library ("" when none). */
const char* rtlws_ddc_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* RTLWS_DDC_H */
