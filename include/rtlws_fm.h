/*
 * rtlws_fm.h -- the FM receive chain of reference src/audio_main.c:110-142 in one launch (librtlws_fm.so).
 *
 * rtlws_hip.h has the pieces -- rtlws_cic_block_sums, rtlws_fm_demod, rtlws_halfband -- and a caller who chains
 * them pays six launches, three intermediate buffers and the delay-line upkeep per decimator block.  The entry
 * points here run CIC block sums (optional), atan2_approx, first difference, hard limit and both 11-tap half-bands
 * of any number of consecutive decimator blocks as one kernel: 2 * cic_r bytes (or 8) in and one byte out per
 * decimated sample.  Every float is bit-identical to the reference's per-block evaluation.
 *
 * State.  A chain carries 21 floats in device memory between calls:
 *   [0]       the phase of the last sample                   (src/audio_main.c:77, prev_sample's phase)
 *   [1..10]   delay line of the first half-band, oldest first (src/audio_main.c:78)
 *   [11..20]  delay line of the second half-band              (src/audio_main.c:79)
 * All zero is the reference's start.  A call reads d_state_in and writes d_state_out; the two must differ (as
 * rtlws_fm_demod requires of its carries), so a caller keeps two buffers and swaps them.
 *
 * Blocks.  Each of the nblocks consecutive blocks of block_len decimated samples has exactly the semantics of one
 * audio_fm_demodulator(signal, block_len) call: half = block_len / 2 outputs of the first half-band, quarter =
 * half / 2 of the second; an odd last sample of a block feeds the phase carry but not the first half-band, an odd
 * last output of the first half-band does not feed the second.  d_audio receives nblocks * quarter floats.
 *
 * run_stage2 == 0 is src/audio_main.c:137's exhausted buffer pool: the second half-band does not run, nothing is
 * written to d_audio (it may be NULL), state_out[11..20] = state_in[11..20]; the phase carry and delay line 1 advance.
 *
 * Refused with -1 (rtlws_fm_last_error() says why): block_len < 20 (the reference's own memcpy at
 * src/resample.c:66 reads in front of its input there), nblocks < 0, cic_r outside 1..128, null pointers,
 * d_state_in == d_state_out, d_iq_cs32 or d_dec not 8-byte aligned, d_iq_cu8 not 16-byte aligned, more audio than
 * one grid holds (2^31 - 2 tiles of rtlws_fm_grid's tile_audio samples).
 */
#ifndef RTLWS_FM_H
#define RTLWS_FM_H

#include "rtlws_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* librtlws_fm.so exports these declarations and nothing else (exports/fm.map) */
#pragma GCC visibility push(default)

#define RTLWS_FM_STATE_FLOATS 21
#define RTLWS_FM_MIN_BLOCK_LEN 20

/* 1 when the shape is served, else 0 (rtlws_fm_last_error() says why).  cic_r = 0: the cmplx_s32 form.
 * Needs no GPU. */
int rtlws_fm_supported(int block_len, long nblocks, int cic_r);

/* Launch geometry of a served shape with run_stage2 != 0: workgroups (one per tile of tile_audio consecutive audio
 * samples, plus the one that writes the state), threads per workgroup, bytes of LDS per workgroup.  Any pointer
 * may be NULL.  0, or -1 when the shape is not served.  Needs no GPU. */
int rtlws_fm_grid(int block_len, long nblocks, int cic_r, int* blocks, int* threads, int* lds_bytes, int* tile_audio);

/* One-time warm-up on the engine's device: loads the library's kernels, so that the launching entry points
 * below make no runtime call other than their launch and may be captured into a hipGraph.  0 / -1 / -3. */
int rtlws_fm_prepare(rtlws_engine* e);

/* d_iq_cs32: nblocks * block_len cmplx_s32 (what rf_decimator's callbacks receive).  d_audio: nblocks * quarter
 * floats.  Asynchronous on `stream` (NULL = the engine's own stream, RTLWS_STREAM_DEFAULT = HIP's: "Streams" in
 * rtlws_hip.h).  nblocks == 0 copies the state.  0; -1 bad argument (a null engine among them: without a device
 * there is no engine, and no CPU path); -3 HIP failure. */
int rtlws_fm_audio_blocks(rtlws_engine* e, const void* d_iq_cs32, int block_len, long nblocks,
                          const float* d_state_in, float* d_state_out, int run_stage2, float* d_audio, void* stream);

/* The same chain with the CIC block sum in front: d_iq_cu8 holds nblocks * block_len * cic_r cmplx_u8, every
 * decimated sample is the sum over cic_r consecutive ones of (x - 128) per component -- rtlws_cic_block_sums's
 * arithmetic, stateless.  block_len counts decimated samples.  If d_dec_or_null is not NULL it receives the
 * nblocks * block_len decimated cmplx_s32 (what rf_decimator's other callbacks want).  1 <= cic_r <= 128; 8, 10
 * and 12 are compile-time instantiations. */
int rtlws_fm_audio_blocks_cu8(rtlws_engine* e, int cic_r, const void* d_iq_cu8, int block_len, long nblocks,
                              const float* d_state_in, float* d_state_out, int run_stage2, float* d_audio,
                              void* d_dec_or_null, void* stream);

/* Last error text of the calling thread from this library ("" when none). */
const char* rtlws_fm_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* RTLWS_FM_H */
