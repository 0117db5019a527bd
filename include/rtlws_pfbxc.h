/*
 * rtlws_pfbxc.h -- polyphase cross-correlator: per channel of the filter bank of rtlws_pfb.h, the power of each of
 * A = 2 .. 4 coherent captures and the cross-spectrum of every pair of them, summed over K consecutive frames, in one
 * launch (librtlws_pfbxc.so).
 *
 * Receivers that share one clock are used for what exists only between them: the phase of the cross-spectrum is time
 * delay and bearing, its magnitude against the two powers is coherence.  rtlws_pfb_run (rtlws_pfb.h) would deliver
 * every capture's complex samples, 8 bytes per input sample each, for a multiply-and-sum of the caller's;
 * rtlws_pfbxc_run multiplies and sums the frames where the transform leaves them and writes A real and A (A - 1) / 2
 * complex rows per K frames (tests/pfbxc_ref.py restates it in numpy).
 *
 * M = 2^log2_channels, 16 .. 1024.  T = taps_per_branch, 1 .. 32.  The prototype h and the hop D (M or M / 2) are those
 * of rtlws_pfb.h.  A = ninputs = 2, 3 or 4 captures x_0 .. x_(A-1) of equal length; Y_a[m][c] is what rtlws_pfb_run
 * delivers for x_a with first_frame_index = 0 (its sign rule multiplies Y_a and Y_b by the same +-1 and reaches no
 * product).  K = k_avg, 1 .. 65536, frames per spectrum; nframes = nspectra K.  With Y_a = ar + i ai, Y_b = br + i bi:
 *   P_a[m][c]     = fl(fl(ar ar) + fl(ai ai))            rtlws_pfbspec.h's P, the same three roundings
 *   X_ab[m][c].re = fl(fl(ar br) + fl(ai bi))            a < b: Y_a conj(Y_b)
 *   X_ab[m][c].im = fl(fl(ai br) - fl(ar bi))            f32 operations, each rounded once, no fused multiply-add
 *   S_a[j][c]  = sum_{m = j K .. j K + K - 1} P_a[m][c]     f32 additions, j = 0 .. nspectra - 1
 *   V_ab[j][c] = sum_{m = j K .. j K + K - 1} X_ab[m][c]    f32 additions, re and im apart
 * If x_b[n] = x_a[n - d] (capture b lags capture a by d samples), V_ab[c] has the phase +2 pi c d / M, c taken as signed
 * (c - M for c >= M / 2).
 * The order of the additions is rtlws_pfbspec.h's, a function of (M, K) alone: not of j, nspectra, A, the pair, T, the
 * hop or the place of a spectrum in the grid, and no atomics take part.  Every partial sum starts from +0, so a row of
 * zeros is +0 bits.  Two runs give the same bits; S_a equals rtlws_pfbspec_run's RTLWS_OUT_POWER_SUM row of x_a bit for
 * bit; a run over the captures from sample j0 K D on gives rows j0 .. of the whole run bit for bit.
 *
 * Every capture holds rtlws_pfbxc_samples_needed() = (nspectra K - 1) D + T M samples and no byte beyond is read.  Two
 * inputs may be the same pointer.  The outputs are raw f32 (phase is the point: there is no dB or byte form):
 *   d_auto   row j A + a is S_a[j]: M floats at d_auto + (j A + a) auto_stride, auto_stride in floats
 *   d_cross  row j NX + x is V_ab[j]: M (re, im) pairs at d_cross + (j NX + x) cross_stride complex values,
 *            NX = A (A - 1) / 2, x = rtlws_pfbxc_pair_index(A, a, b): the pairs a < b row-major, (0,1), (0,2), .., (1,2), ..
 * shifted = 0: value i of a row is channel i.  shifted = 1: value i is channel (i + M / 2) mod M, DC in the middle.
 *
 * Parallelism is across output spectra, as in rtlws_pfbspec.h: a workgroup owns whole spectra.
 *
 * Refused with -1 (rtlws_pfbxc_last_error() says why): log2_channels outside 4 .. 10, taps_per_branch outside 1 .. 32,
 * a hop that is neither M nor M / 2, k_avg outside 1 .. 65536, ninputs outside 2 .. 4 (a run takes the plan's), shifted
 * other than 0 or 1, nspectra < 0 or more than one grid holds, auto_stride < M or not a multiple of 4, cross_stride < M or
 * not a multiple of 2, a null array or a null pointer in it, a capture or an output that is not 16-byte aligned.
 */
#ifndef RTLWS_PFBXC_H
#define RTLWS_PFBXC_H

#include <stdint.h>

#include "rtlws_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* librtlws_pfbxc.so exports these declarations and nothing else (exports/pfbxc.map) */
#pragma GCC visibility push(default)

#define RTLWS_PFBXC_MAX_K_AVG 65536
#define RTLWS_PFBXC_MIN_INPUTS 2
#define RTLWS_PFBXC_MAX_INPUTS 4

typedef struct rtlws_pfbxc_plan rtlws_pfbxc_plan;

/* 1 when the shape is served, else 0 (rtlws_pfbxc_last_error() says why).  hop: M or M / 2.  Needs no GPU. */
int rtlws_pfbxc_supported(int log2_channels, int taps_per_branch, int hop, int k_avg, int ninputs);

/* Samples of every capture that nspectra spectra read: (nspectra k_avg - 1) hop + T M, 0 for nspectra == 0; -1 when
 * the shape is not served or nspectra < 0.  Needs no GPU. */
long rtlws_pfbxc_samples_needed(int log2_channels, int taps_per_branch, int hop, int k_avg, long nspectra);

/* The number x of the pair (a, b), 0 <= a < b < ninputs, among the rows of a spectrum in d_cross; -1 for anything
 * else.  Host only; needs no GPU. */
int rtlws_pfbxc_pair_index(int ninputs, int a, int b);

/* Launch geometry: workgroups, threads per workgroup, bytes of LDS per workgroup (ninputs tiles of the filter bank),
 * spectra per workgroup (1 where k_avg is at least the 4096 / M frames of a tile, else that many frames / k_avg,
 * rounded down).  Any pointer may be NULL.  0, or -1 when the shape is not served.  Needs no GPU. */
int rtlws_pfbxc_grid(int log2_channels, int taps_per_branch, int hop, int k_avg, int ninputs, long nspectra, int* blocks,
                     int* threads, int* lds_bytes, int* spectra_per_block);

/* The prototype (taps_per_branch * M int16 in host memory, read before the call returns) and the transform's table
 * (the bits of rtlws_pfb_twiddles) on the engine's device and the kernel for ninputs captures loaded, so that
 * rtlws_pfbxc_run makes no runtime call other than its launch and may be captured into a hipGraph.  A new prototype
 * or another ninputs is a new plan.  NULL on failure (a null engine among them: without a device there is no engine,
 * and no CPU path). */
rtlws_pfbxc_plan* rtlws_pfbxc_open(rtlws_engine* e, int log2_channels, int taps_per_branch, const int16_t* taps, int ninputs);

/* d_iq_cu8: a host array of the plan's ninputs device pointers, read before the call returns; each capture is
 * rtlws_pfbxc_samples_needed() cmplx_u8, 16-byte aligned.  d_auto: nspectra * ninputs rows of M f32; d_cross:
 * nspectra * NX rows of M complex f32; both 16-byte aligned; nothing outside the rows is written.  Asynchronous on
 * `stream` (NULL = the engine's own stream, RTLWS_STREAM_DEFAULT = HIP's: "Streams" in rtlws_hip.h); one kernel launch
 * and no other runtime call.  nspectra == 0 does nothing.  Every refusal is made before the device is asked for
 * anything: first what needs no plan (the hop a power of two 8 .. 1024, k_avg, shifted, nspectra, the strides >= 16
 * and their multiples, the output pointers, the array), then a null plan, then what the plan decides (the hop, the
 * grid, the strides >= M, the captures' pointers).  0; -1 bad argument; -3 HIP failure. */
int rtlws_pfbxc_run(rtlws_pfbxc_plan* p, const void* const* d_iq_cu8, long nspectra, int hop, int k_avg, int shifted,
                    float* d_auto, long auto_stride, float* d_cross, long cross_stride, void* stream);

void rtlws_pfbxc_close(rtlws_pfbxc_plan* p);

/* Last error text of the calling thread from this library ("" when none). */
const char* rtlws_pfbxc_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* RTLWS_PFBXC_H */
