/*
 * rtlws_pfb.h -- polyphase channelizer: all M = 2^k channels of one capture in one launch (librtlws_pfb.so).
 *
 * rtlws_ddc_run's channels are filtered by the CIC block sum alone and cost O(channels) per input sample
 * (DESIGN.md 4.12).  rtlws_pfb_run applies a prototype low-pass of T * M int16 taps as M branch filters and
 * transforms every frame of M branch outputs: all M channels at O(T + log M) per input sample, with the
 * prototype's stop-band between channels (tests/pfb_ref.py restates it in numpy).
 *
 * M = 2^log2_channels, 16 .. 1024.  T = taps_per_branch, 1 .. 32.  h[0 .. T M - 1] the prototype.  The hop D is M
 * (critically sampled) or M / 2 (oversampled by two).  With x[n] = (re - 128) + i (im - 128) the capture,
 * m = 0 .. nframes - 1 and g = first_frame_index + m:
 *   v_m[p]  = sum_{t<T} h[p + t M] x[m D + t M + p]                  p = 0 .. M - 1   (int32, exact)
 *   Y[m][c] = e^(-2 pi i c g D / M) sum_p v_m[p] e^(-2 pi i c p / M)   c = 0 .. M - 1   (f32)
 * The capture holds rtlws_pfb_samples_needed() = (nframes - 1) D + T M samples and no byte beyond is read.  The
 * leading factor is 1 at D = M and (-1)^(c g) at D = M / 2, applied as an exact sign flip: every channel's phase
 * refers to absolute sample time, so chunked calls that overlap by (T - 1) M samples and pass first_frame_index
 * concatenate to what one call gives, and no state is carried between calls.  Channel c is centred at c / M cycles
 * per sample (c >= M / 2: the negative offsets); the output is unnormalised, gain sum(h).  v is converted once to
 * f32; the transform is f32 with twiddles computed in f64 and rounded once (rtlws_pfb_twiddles).  All-128 input
 * gives all-zero output.
 *
 * Refused with -1 (rtlws_pfb_last_error() says why): log2_channels outside 4 .. 10, taps_per_branch outside
 * 1 .. 32, a hop that is neither M nor M / 2, nframes < 0 or more than one grid holds, first_frame_index < 0, an
 * unknown layout, out_stride too small for the layout, d_iq_cu8 not 16-byte or d_out_cf32 not 8-byte aligned,
 * null pointers.
 */
#ifndef RTLWS_PFB_H
#define RTLWS_PFB_H

#include <stdint.h>

#include "rtlws_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* librtlws_pfb.so exports these declarations and nothing else (exports/pfb.map) */
#pragma GCC visibility push(default)

#define RTLWS_PFB_MIN_LOG2_CHANNELS 4
#define RTLWS_PFB_MAX_LOG2_CHANNELS 10
#define RTLWS_PFB_MAX_TAPS 32

/* channel c is the contiguous stream of nframes values at out + c * out_stride (out_stride >= nframes) */
#define RTLWS_PFB_CHANNEL_MAJOR 0
/* frame m is the M values at out + m * out_stride (out_stride >= M): the waterfall */
#define RTLWS_PFB_TIME_MAJOR 1

typedef struct rtlws_pfb_plan rtlws_pfb_plan;

/* 1 when the shape is served, else 0 (rtlws_pfb_last_error() says why).  hop: M or M / 2.  Needs no GPU. */
int rtlws_pfb_supported(int log2_channels, int taps_per_branch, int hop);

/* A prototype: the Hamming-windowed sinc with its first zeros at +-M samples.  With N = T M,
 *   taps[n] = rint(32767 sinc((n - (N - 1) / 2) / M) (0.54 - 0.46 cos(2 pi n / (N - 1)))),  sinc(x) = sin(pi x) / (pi x).
 * 0; -1 for a shape that is not served or a null pointer.  Host only. */
int rtlws_pfb_design(int log2_channels, int taps_per_branch, int16_t* taps);

/* The transform's table as the library builds it: M pairs (cos, -sin)(2 pi j / M) = e^(-2 pi i j / M), computed in
 * f64 and rounded once.  0; -1 for a shape that is not served or a null pointer.  Needs no GPU. */
int rtlws_pfb_twiddles(int log2_channels, float* re_im);

/* Samples of the capture that nframes frames read: (nframes - 1) hop + T M, 0 for nframes == 0; -1 when the shape
 * is not served or nframes < 0.  Needs no GPU. */
long rtlws_pfb_samples_needed(int log2_channels, int taps_per_branch, int hop, long nframes);

/* Launch geometry: workgroups (one per tile of tile_frames consecutive frames), threads per workgroup, bytes of
 * LDS per workgroup.  Any pointer may be NULL.  0, or -1 when the shape is not served.  Needs no GPU. */
int rtlws_pfb_grid(int log2_channels, int taps_per_branch, int hop, long nframes, int* blocks, int* threads,
                   int* lds_bytes, int* tile_frames);

/* The prototype (taps_per_branch * M int16 in host memory, read before the call returns) and the transform's
 * table on the engine's device and the kernel loaded, so that rtlws_pfb_run makes no runtime call other than its
 * launch and may be captured into a hipGraph.  A new prototype is a new plan.  NULL on failure (a null engine
 * among them: without a device there is no engine, and no CPU path). */
rtlws_pfb_plan* rtlws_pfb_open(rtlws_engine* e, int log2_channels, int taps_per_branch, const int16_t* taps);

/* d_iq_cu8: rtlws_pfb_samples_needed() cmplx_u8, 16-byte aligned.  d_out_cf32: complex f32 (re, im), 8-byte
 * aligned, in `layout`; nothing outside the ranges the layout defines is written.  hop, layout and
 * first_frame_index travel in the kernel's arguments.  Asynchronous on `stream` (NULL = the engine's own stream,
 * RTLWS_STREAM_DEFAULT = HIP's: "Streams" in rtlws_hip.h); one kernel launch and no other runtime call.
 * nframes == 0 does nothing.  Every refusal is made before the device is asked for anything: first what needs no
 * plan (the hop a power of two 8 .. 1024, nframes, first_frame_index, the layout, out_stride >= nframes or >= 16,
 * the pointers), then a null plan, then what the plan's M decides (the hop, out_stride >= M, the grid).
 * 0; -1 bad argument; -3 HIP failure. */
int rtlws_pfb_run(rtlws_pfb_plan* p, const void* d_iq_cu8, long nframes, int hop, long first_frame_index, int layout,
                  void* d_out_cf32, long out_stride, void* stream);

void rtlws_pfb_close(rtlws_pfb_plan* p);

/* Last error text of the calling thread from this library ("" when none). */
const char* rtlws_pfb_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* RTLWS_PFB_H */
