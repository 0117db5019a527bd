/*
 * rtlws_pfbspec.h -- polyphase spectrometer: the power of all M = 2^k channels of one capture, summed over K
 * consecutive frames, in one launch (librtlws_pfbspec.so).
 *
 * rtlws_pfb_run (rtlws_pfb.h) delivers every channel's complex samples, 8 bytes per input sample.  A spectrum or a
 * waterfall row with the filter bank's leakage between channels needs only their power: rtlws_pfbspec_run squares
 * and sums the frames where the transform leaves them and writes one row per K frames (DESIGN.md 4.15;
 * tests/pfbspec_ref.py restates it in numpy).
 *
 * M = 2^log2_channels, 16 .. 1024.  T = taps_per_branch, 1 .. 32.  The prototype h, the hop D (M or M / 2), the
 * capture x and Y[m][c] are those of rtlws_pfb.h with first_frame_index = 0; its sign rule does not reach the power.
 * K = k_avg, 1 .. 65536, frames per spectrum; nframes = nspectra K.  With Y[m][c] = re + i im as rtlws_pfb_run
 * delivers it:
 *   P[m][c] = fl(fl(re re) + fl(im im))            three f32 operations, each rounded once, no fused multiply-add
 *   S[j][c] = sum_{m = j K .. j K + K - 1} P[m][c]   f32 additions, j = 0 .. nspectra - 1
 * The order of the additions is a function of (M, K) alone: not of j, nspectra, T, the hop, the output kind or the
 * place of a spectrum in the grid, and no atomics take part.  Two runs give the same bits, and a run over the
 * capture from sample j0 K D on gives rows j0 .. of the whole run bit for bit.
 *
 * The capture holds rtlws_pfbspec_samples_needed() = (nspectra K - 1) D + T M samples and no byte beyond is read.
 * Row j is M values at d_out + j * out_stride (out_stride in elements).  shifted = 0: value i is channel i.
 * shifted = 1: value i is channel (i + M / 2) mod M, DC in the middle: the order of spectrum.h's rows and of the
 * payload.  There is no DC-slot rule here: that rule is spectrum.c's, and nothing of the reference pins this path.
 *
 * Output kinds (the values of enum rtlws_output, rtlws_hip.h):
 *   RTLWS_OUT_POWER_SUM   f32 S, raw; scale is ignored
 *   RTLWS_OUT_MEAN_DB     f32 10 log10(S lin), lin = fl(scale / (float)K) formed on the host; f32 arithmetic
 *   RTLWS_OUT_PAYLOAD_U8  one byte per channel: that dB value truncated by (int) and clamped to 0 .. 255
 * scale is a finite float > 0.  The filter bank's gain is sum(h), not 1 / 128: scale = 1 / (128 sum(h))^2 makes a
 * full-scale tone on a channel centre read 0 dB.  All-128 input gives exact zeros, -inf, and bytes 0.
 *
 * Parallelism is across output spectra: a workgroup owns whole spectra, so a caller who integrates a whole capture
 * into one row (nspectra = 1) runs on one workgroup.  Ask for shorter groups and add the rows (they are plain f32
 * sums of non-negative terms).
 *
 * Refused with -1 (rtlws_pfbspec_last_error() says why): log2_channels outside 4 .. 10, taps_per_branch outside
 * 1 .. 32, a hop that is neither M nor M / 2, k_avg outside 1 .. 65536, an unknown output, shifted other than 0 or
 * 1, a scale that is not finite or <= 0 (dB and payload), nspectra < 0 or more than one grid holds, out_stride < M
 * or not a multiple of 4 (f32 rows) or 16 (byte rows), null pointers, d_iq_cu8 or d_out not 16-byte aligned.
 */
#ifndef RTLWS_PFBSPEC_H
#define RTLWS_PFBSPEC_H

#include <stdint.h>

#include "rtlws_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* librtlws_pfbspec.so exports these declarations and nothing else (exports/pfbspec.map) */
#pragma GCC visibility push(default)

#define RTLWS_PFBSPEC_MAX_K_AVG 65536

typedef struct rtlws_pfbspec_plan rtlws_pfbspec_plan;

/* 1 when the shape is served, else 0 (rtlws_pfbspec_last_error() says why).  hop: M or M / 2; output: a value of
 * enum rtlws_output.  Needs no GPU. */
int rtlws_pfbspec_supported(int log2_channels, int taps_per_branch, int hop, int k_avg, int output);

/* Samples of the capture that nspectra spectra read: (nspectra k_avg - 1) hop + T M, 0 for nspectra == 0; -1 when
 * the shape is not served or nspectra < 0.  Needs no GPU. */
long rtlws_pfbspec_samples_needed(int log2_channels, int taps_per_branch, int hop, int k_avg, long nspectra);

/* Launch geometry: workgroups, threads per workgroup, bytes of LDS per workgroup, spectra per workgroup (1 where
 * k_avg is at least the 4096 / M frames of a tile, else that many frames / k_avg, rounded down).  Any pointer may be
 * NULL.  0, or -1 when the shape is not served.  Needs no GPU. */
int rtlws_pfbspec_grid(int log2_channels, int taps_per_branch, int hop, int k_avg, long nspectra, int* blocks, int* threads,
                       int* lds_bytes, int* spectra_per_block);

/* The prototype (taps_per_branch * M int16 in host memory, read before the call returns) and the transform's table
 * (the bits of rtlws_pfb_twiddles) on the engine's device and the kernel loaded, so that rtlws_pfbspec_run makes no
 * runtime call other than its launch and may be captured into a hipGraph.  A new prototype is a new plan.  NULL on
 * failure (a null engine among them: without a device there is no engine, and no CPU path). */
rtlws_pfbspec_plan* rtlws_pfbspec_open(rtlws_engine* e, int log2_channels, int taps_per_branch, const int16_t* taps);

/* d_iq_cu8: rtlws_pfbspec_samples_needed() cmplx_u8, 16-byte aligned.  d_out: nspectra rows of M f32 or M bytes,
 * 16-byte aligned, out_stride elements apart; nothing outside the rows is written.  Asynchronous on `stream` (NULL =
 * the engine's own stream, RTLWS_STREAM_DEFAULT = HIP's: "Streams" in rtlws_hip.h); one kernel launch and no other
 * runtime call.  nspectra == 0 does nothing.  Every refusal is made before the device is asked for anything: first
 * what needs no plan (the hop a power of two 8 .. 1024, k_avg, the output, shifted, scale, nspectra, out_stride >= 16
 * and its multiple, the pointers), then a null plan, then what the plan's M decides (the hop, the grid,
 * out_stride >= M).  0; -1 bad argument; -3 HIP failure. */
int rtlws_pfbspec_run(rtlws_pfbspec_plan* p, const void* d_iq_cu8, long nspectra, int hop, int k_avg, int output, int shifted,
                      float scale, void* d_out, long out_stride, void* stream);

void rtlws_pfbspec_close(rtlws_pfbspec_plan* p);

/* Last error text of the calling thread from this library ("" when none). */
const char* rtlws_pfbspec_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* RTLWS_PFBSPEC_H */
