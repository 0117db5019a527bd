/*
 * rtlws_fmbank.h -- up to 32 FM stations from one capture in one launch (librtlws_fmbank.so).
 *
 * rtlws_ddc.h tunes up to 32 channels out of one device-resident cmplx_u8 capture, and rtlws_fm.h runs the FM
 * receive chain of one cmplx_s32 stream; a caller who wants to hear every station of a capture chains them through
 * 8 bytes per channel and decimated sample of device memory and one rtlws_fm_audio_blocks launch per channel.
 * rtlws_fmbank_run is that composition as ONE kernel with no device buffer between the capture and the audio:
 * 2 * cic_r bytes in per decimated sample, one byte out per channel and decimated sample, and 2 * 84 bytes of state
 * per channel.
 *
 * Definition.  For channel c with tuning word k_c, the audio and the carried state are, bit for bit, what these two
 * steps give:
 *   1. rtlws_ddc_run(cic_r, the capture, dec_len = nblocks * block_len, first_dec_index, the one word k_c)
 *      (rtlws_ddc.h: the phasor table, the tuning word, the integer arithmetic, first_dec_index);
 *   2. rtlws_fm_audio_blocks(that stream, block_len, nblocks, state c in, state c out, run_stage2 = 1, audio c)
 *      (rtlws_fm.h: the state's layout, the per-block semantics, half and quarter).
 * Nothing of either is restated here.  As there, a call carries no hidden state: chunked calls cut at block multiples
 * that pass first_dec_index + blocks_done * block_len and swap the state buffers concatenate to what one call gives.
 *
 * rtlws_fm.h's run_stage2 == 0 (the reference's exhausted host pool) and the decimated-sample output are left out:
 * the first has no meaning without that pool, the second is rtlws_ddc_run.
 *
 * Refused with -1 (rtlws_fmbank_last_error() says why), all before the plan is asked for anything: block_len < 20,
 * nblocks < 0, cic_r outside 1 .. 128, nchannels outside 1 .. 32, a tuning word outside [-P/2, P/2),
 * first_dec_index < 0, audio_stride < nblocks * quarter, overlapping d_state_in and d_state_out ranges, d_iq_cu8 not
 * 16-byte aligned, null pointers, more tiles than one grid holds.
 */
#ifndef RTLWS_FMBANK_H
#define RTLWS_FMBANK_H

#include "rtlws_ddc.h"
#include "rtlws_fm.h"
#include "rtlws_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* librtlws_fmbank.so exports these declarations and nothing else (exports/fmbank.map) */
#pragma GCC visibility push(default)

#define RTLWS_FMBANK_MAX_CHANNELS 32

typedef struct rtlws_fmbank_plan rtlws_fmbank_plan;

/* 1 when the shape is served, else 0 (rtlws_fmbank_last_error() says why).  Needs no GPU. */
int rtlws_fmbank_supported(int cic_r, int nchannels, int block_len, long nblocks);

/* Launch geometry of a served shape: workgroups (per column tile of eight channels one per tile of tile_audio
 * consecutive audio samples, plus the one that writes the states), threads per workgroup, bytes of LDS per
 * workgroup.  Any pointer may be NULL.  0, or -1 when the shape is not served.  Needs no GPU. */
int rtlws_fmbank_grid(int cic_r, int nchannels, int block_len, long nblocks, int* blocks, int* threads, int* lds_bytes,
                      int* tile_audio);

/* The phasor table T of rtlws_ddc.h (rtlws_ddc_table's values, from the same builder) on the engine's device and the
 * library's kernels loaded, so that rtlws_fmbank_run makes no runtime call other than its launch and may be captured
 * into a hipGraph.  NULL on failure (a null engine among them: without a device there is no engine, and no CPU path). */
rtlws_fmbank_plan* rtlws_fmbank_open(rtlws_engine* e);

/* d_iq_cu8: nblocks * block_len * cic_r cmplx_u8, 16-byte aligned; block_len counts decimated samples.
 * tuning_words: nchannels ints in host memory, read before the call returns: they travel in the kernel's arguments.
 * d_state_in, d_state_out: channel-major, RTLWS_FM_STATE_FLOATS floats per channel ([c][21], rtlws_fm.h's layout);
 * the two ranges must not overlap.  d_audio: channel c is the contiguous nblocks * quarter floats at
 * d_audio + c * audio_stride (audio_stride >= nblocks * quarter).  Nothing outside those ranges is written.
 * Asynchronous on `stream` (NULL = the engine's own stream, RTLWS_STREAM_DEFAULT = HIP's: "Streams" in rtlws_hip.h);
 * one kernel launch and no other runtime call.  cic_r = 8, 10 and 12 are compile-time instantiations.
 * nblocks == 0 copies the states.  0; -1 bad argument; -3 HIP failure. */
int rtlws_fmbank_run(rtlws_fmbank_plan* p, int cic_r, const void* d_iq_cu8, int block_len, long nblocks,
                     long first_dec_index, int nchannels, const int* tuning_words, const float* d_state_in,
                     float* d_state_out, float* d_audio, long audio_stride, void* stream);

void rtlws_fmbank_close(rtlws_fmbank_plan* p);

/* Last error text of the calling thread from this library ("" when none). */
const char* rtlws_fmbank_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* RTLWS_FMBANK_H */
