/*
 * rtlws_fmfir.h -- up to 32 FM stations from one capture behind an int16 FIR, in one launch (librtlws_fmfir.so).
 *
 * rtlws_fmbank_run (rtlws_fmbank.h) makes audio from up to 32 stations of one device-resident cmplx_u8 capture in one
 * launch, but its channel filter is the CIC block sum of cic_r samples: a tone 1.5 output bandwidths off a channel's
 * centre comes through at -13.2 dB, and the discriminator behind it hears its neighbours.  rtlws_ddcfir_run
 * (rtlws_ddcfir.h) is the down-converter with a real channel filter, an int16 FIR of 1 .. 256 taps.  A caller who
 * wants filtered audio chains it with one rtlws_fm_audio_blocks launch per channel through 8 bytes per channel and
 * decimated sample of device memory.  rtlws_fmfir_run is that composition as ONE kernel with no device buffer between
 * the capture and the audio.
 *
 * Definition.  For channel c with tuning word k_c, the audio and the carried state are, bit for bit, what these two
 * steps give:
 *   1. rtlws_ddcfir_run(the plan's decim, ntaps and taps, the capture, dec_len = nblocks * block_len, first_dec_index,
 *      the one word k_c, out_shift)
 *      (rtlws_ddcfir.h: the phasor table, the taps' limit, the integer arithmetic, out_shift, first_dec_index);
 *   2. rtlws_fm_audio_blocks(that stream, block_len, nblocks, state c in, state c out, run_stage2 = 1, audio c)
 *      (rtlws_fm.h: the state's layout, the per-block semantics, half and quarter).
 * Nothing of either is restated here.  What follows from them:
 *   - The capture holds rtlws_fmfir_samples_needed = (nblocks * block_len - 1) * decim + ntaps samples, and no byte
 *     beyond them is read.
 *   - A call carries no hidden state.  Chunked calls concatenate to one call's floats when they are cut at block
 *     multiples, start their capture at sample blocks_done * block_len * decim (so neighbouring chunks' captures
 *     overlap by ntaps - decim samples when that is positive), pass first_dec_index + blocks_done * block_len and swap
 *     the state buffers.
 *   - ntaps = decim, every tap 16384 and out_shift = 14 is rtlws_fmbank_run bit for bit.
 *
 * rtlws_fm.h's run_stage2 == 0 (the reference's exhausted host pool) and the decimated-sample output are left out, for
 * rtlws_fmbank.h's reasons: the first has no meaning without that pool, the second is rtlws_ddcfir_run.
 *
 * Refused with -1 (rtlws_fmfir_last_error() says why): decim outside 1 .. 128, ntaps outside 1 .. 256, a tap outside
 * +-RTLWS_DDCFIR_MAX_TAP (at open); block_len < 20, nblocks < 0, nchannels outside 1 .. 32, a tuning word outside
 * [-P/2, P/2), out_shift outside 0 .. 30, first_dec_index < 0, audio_stride < nblocks * quarter, overlapping d_state_in
 * and d_state_out ranges, d_iq_cu8 not 16-byte aligned, d_state_in, d_state_out or d_audio not 4-byte aligned, null
 * pointers, nblocks * block_len too large for the capture's size in a long, more tiles than one grid holds.
 */
#ifndef RTLWS_FMFIR_H
#define RTLWS_FMFIR_H

#include <stdint.h>

#include "rtlws_ddcfir.h"
#include "rtlws_fm.h"
#include "rtlws_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* librtlws_fmfir.so exports these declarations and nothing else (exports/fmfir.map) */
#pragma GCC visibility push(default)

/* The limits of decim, ntaps, a tap and out_shift are rtlws_ddcfir.h's RTLWS_DDCFIR_MAX_*. */
#define RTLWS_FMFIR_MAX_CHANNELS 32

typedef struct rtlws_fmfir_plan rtlws_fmfir_plan;

/* 1 when the shape is served, else 0 (rtlws_fmfir_last_error() says why).  Needs no GPU. */
int rtlws_fmfir_supported(int decim, int ntaps, int nchannels, int block_len, long nblocks);

/* Samples of the capture a run reads: (nblocks * block_len - 1) * decim + ntaps, 0 for nblocks == 0; -1 when the shape
 * is not served.  Needs no GPU. */
long rtlws_fmfir_samples_needed(int decim, int ntaps, int block_len, long nblocks);

/* Launch geometry of a served shape, in rtlws_fmbank_grid's conventions: workgroups (per column tile of eight channels
 * one per tile of tile_audio consecutive audio samples, plus the one that writes the states; 1 for the state copy of
 * nblocks == 0), threads per workgroup, bytes of LDS per workgroup (the filter's operands lie inside them).  Any
 * pointer may be NULL.  0, or -1 when the shape is not served.  Needs no GPU. */
int rtlws_fmfir_grid(int decim, int ntaps, int nchannels, int block_len, long nblocks, int* blocks, int* threads,
                     int* lds_bytes, int* tile_audio);

/* The taps (ntaps int16 in host memory, copied; rtlws_ddcfir_design makes a low-pass for decim, or they are the
 * caller's) and the phasor table T on the engine's device, and the plan's own kernel instantiation loaded, so that
 * rtlws_fmfir_run makes no runtime call other than its launch and may be captured into a hipGraph.  NULL on failure (a
 * null engine among them: without a device there is no engine, and no CPU path; a tap outside +-RTLWS_DDCFIR_MAX_TAP,
 * refused in rtlws_ddcfir_open's words). */
rtlws_fmfir_plan* rtlws_fmfir_open(rtlws_engine* e, int decim, int ntaps, const int16_t* taps);

/* d_iq_cu8: rtlws_fmfir_samples_needed cmplx_u8, 16-byte aligned; block_len counts decimated samples.
 * tuning_words: nchannels ints in host memory, read before the call returns: they travel in the kernel's arguments.
 * out_shift = rtlws_ddcfir_run's s, 0 .. 30.  d_state_in, d_state_out, d_audio, audio_stride: rtlws_fmbank_run's
 * layouts (channel-major [c][21] states whose two ranges must not overlap; channel c's nblocks * quarter floats at
 * d_audio + c * audio_stride); nothing outside those ranges is written.  Asynchronous on `stream` (NULL = the engine's
 * own stream, RTLWS_STREAM_DEFAULT = HIP's: "Streams" in rtlws_hip.h); one kernel launch and no other runtime call.
 * decim and ntaps both multiples of four is a compile-time instantiation (8-byte operand loads).  nblocks == 0 copies
 * the states.  Refusals come in rtlws_ddcfir_run's order: what needs no plan (every argument rule above), then a null
 * plan; the plan's shape adds no rule of its own.  0; -1 bad argument; -3 HIP failure. */
int rtlws_fmfir_run(rtlws_fmfir_plan* p, const void* d_iq_cu8, int block_len, long nblocks, long first_dec_index,
                    int nchannels, const int* tuning_words, int out_shift, const float* d_state_in, float* d_state_out,
                    float* d_audio, long audio_stride, void* stream);

void rtlws_fmfir_close(rtlws_fmfir_plan* p);

/* Last error text of the calling thread from this library ("" when none). */
const char* rtlws_fmfir_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* RTLWS_FMFIR_H */
