/*
 * rtlws_pfbbf.h -- polyphase beamformer: per channel of the filter bank of rtlws_pfb.h, B = 1 .. 4 complex-weighted sums
 * ("beams") of A = 1 .. 8 coherent captures, as voltages or as powers summed over K consecutive frames, in one launch
 * (librtlws_pfbbf.so).
 *
 * rtlws_pfbxc.h measures what lies between receivers that share a clock: delay, bearing, coherence.  This header uses
 * what was measured: a steered beam adds the captures in phase for one direction, a nulled beam cancels one.  With
 * rtlws_pfb_run a beam needs A launches that each write 8 bytes per input sample, and a combine pass of the caller's;
 * here the captures go through one tile of the filter bank one after the other and the beams are summed in registers
 * (tests/pfbbf_ref.py restates it in numpy).
 *
 * M = 2^log2_channels, 16 .. 1024.  T = taps_per_branch, 1 .. 32.  The prototype h and the hop D (M or M / 2) are those
 * of rtlws_pfb.h.  A = ninputs captures x_0 .. x_(A-1) of equal length; Y_a[m][c] is what rtlws_pfb_run delivers for x_a
 * before its sign rule.  B = nbeams.  The weights W[b][a][c] are complex f32 in device memory, contiguous [B][A][M]
 * (re, im) pairs, c the natural channel index in every mode; they are an argument of a run and no state of the plan: a
 * caller re-steers by overwriting the buffer between launches or graph replays.  With w = wr + i wi, y = yr + i yi:
 *   t_a       = (fl(fl(wr yr) - fl(wi yi)), fl(fl(wr yi) + fl(wi yr)))    f32 operations, each rounded once,
 *   Z_b[m][c] = (((+0 + t_0) + t_1) + ..) + t_(A-1)                       no fused multiply-add; a ascending
 * Voltage mode (rtlws_pfbbf_run) delivers Z_b with the sign rule of rtlws_pfb.h applied afterwards as a flip of both
 * sign bits: at D = M / 2 the factor (-1)^(c g), g = first_frame_index + m.  Beam b lies at d_out + b beam_stride
 * complex values, in either layout of rtlws_pfb_run, out_stride as there.  Runs in chunks that pass first_frame_index
 * concatenate bit for bit.
 * Power mode (rtlws_pfbbf_power) delivers
 *   P_b[m][c] = fl(fl(zr zr) + fl(zi zi))
 *   S_b[j][c] = sum_{m = j K .. j K + K - 1} P_b[m][c]                    K = k_avg, 1 .. 65536; nframes = nspectra K
 * summed in exactly the order of rtlws_pfbspec.h, a function of (M, K) alone, every partial sum from +0; the beams'
 * voltages never reach device memory.  Row j B + b is S_b[j]: M floats at d_out + (j B + b) row_stride floats.
 * shifted = 0: value i of a row is channel i.  shifted = 1: value i is channel (i + M / 2) mod M, DC in the middle.
 * There is no dB or byte form.
 *
 * So a beam with W[b][a0][c] = 1 + 0i and every other weight 0 equals rtlws_pfb_run's output of x_a0 by value (the sign
 * of a zero may differ) and rtlws_pfbspec_run's RTLWS_OUT_POWER_SUM row of x_a0 bit for bit; and power mode equals the
 * ordered sums of the f32 products of voltage mode's own output bit for bit.  Beam b does not depend on B or on the
 * other beams' weights.  Two runs give the same bits; no atomics take part.
 *
 * Every capture holds rtlws_pfbbf_samples_needed() samples and no byte beyond is read.  Two inputs may be the same
 * pointer.
 *
 * Refused with -1 (rtlws_pfbbf_last_error() says why): log2_channels outside 4 .. 10, taps_per_branch outside 1 .. 32,
 * a hop that is neither M nor M / 2, ninputs outside 1 .. 8 or nbeams outside 1 .. 4 or either other than the plan's,
 * nframes or nspectra < 0 or more than one grid holds, first_frame_index < 0, an unknown layout, out_stride too small
 * for the layout, beam_stride below the extent of one beam's output, k_avg outside 1 .. 65536, shifted other than 0
 * or 1, row_stride < M or not a multiple of 4, a null array, a null pointer in it or a null output or weight pointer,
 * a capture, the weights or a power output that is not 16-byte aligned, a voltage output that is not 8-byte aligned.
 */
#ifndef RTLWS_PFBBF_H
#define RTLWS_PFBBF_H

#include <stdint.h>

#include "rtlws_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* librtlws_pfbbf.so exports these declarations and nothing else (exports/pfbbf.map) */
#pragma GCC visibility push(default)

#define RTLWS_PFBBF_MAX_K_AVG 65536
#define RTLWS_PFBBF_MIN_INPUTS 1
#define RTLWS_PFBBF_MAX_INPUTS 8
#define RTLWS_PFBBF_MIN_BEAMS 1
#define RTLWS_PFBBF_MAX_BEAMS 4

typedef struct rtlws_pfbbf_plan rtlws_pfbbf_plan;

/* 1 when the shape is served, else 0 (rtlws_pfbbf_last_error() says why).  hop: M or M / 2.  Needs no GPU. */
int rtlws_pfbbf_supported(int log2_channels, int taps_per_branch, int hop, int ninputs, int nbeams);

/* Samples of every capture that a run reads.  k_avg == 0, voltage mode: count is nframes, (count - 1) hop + T M.
 * k_avg >= 1, power mode: count is nspectra, (count k_avg - 1) hop + T M.  0 for count == 0; -1 when the shape is not
 * served, count < 0 or more than one grid holds.  Needs no GPU. */
long rtlws_pfbbf_samples_needed(int log2_channels, int taps_per_branch, int hop, int k_avg, long count);

/* Launch geometry of either mode (k_avg and count as for rtlws_pfbbf_samples_needed): workgroups, threads per
 * workgroup, bytes of LDS per workgroup (one tile of the filter bank, whatever ninputs and nbeams are), and per
 * workgroup the frames (voltage mode: 4096 / M) or the spectra (power mode: 1 where k_avg is at least 4096 / M, else
 * that many frames / k_avg, rounded down).  Any pointer may be NULL.  0, or -1 when the shape is not served.  Needs no
 * GPU. */
int rtlws_pfbbf_grid(int log2_channels, int taps_per_branch, int hop, int k_avg, long count, int* blocks, int* threads,
                     int* lds_bytes, int* per_block);

/* The prototype (taps_per_branch * M int16 in host memory, read before the call returns) and the transform's table
 * (the bits of rtlws_pfb_twiddles) on the engine's device and both kernels for nbeams beams loaded, so that a run makes
 * no runtime call other than its launch and may be captured into a hipGraph.  A new prototype, another ninputs or
 * another nbeams is a new plan.  NULL on failure (a null engine among them: without a device there is no engine, and no
 * CPU path). */
rtlws_pfbbf_plan* rtlws_pfbbf_open(rtlws_engine* e, int log2_channels, int taps_per_branch, const int16_t* taps, int ninputs,
                                   int nbeams);

/* Voltage mode.  d_iq_cu8: a host array of ninputs device pointers, read before the call returns; each capture is
 * rtlws_pfbbf_samples_needed(.., 0, nframes) cmplx_u8, 16-byte aligned.  d_weights: nbeams * ninputs * M complex f32 on
 * the device, 16-byte aligned, read by the kernel when it runs.  layout, out_stride and first_frame_index are
 * rtlws_pfb_run's; beam b lies at d_out_cf32 + b * beam_stride complex values, and beam_stride is at least the extent
 * of one beam: (nframes - 1) out_stride + M (RTLWS_PFB_TIME_MAJOR) or (M - 1) out_stride + nframes
 * (RTLWS_PFB_CHANNEL_MAJOR).  Nothing outside the values is written.  Asynchronous on `stream` (NULL = the engine's own
 * stream, RTLWS_STREAM_DEFAULT = HIP's: "Streams" in rtlws_hip.h); one kernel launch and no other runtime call.
 * nframes == 0 does nothing.  Every refusal is made before the device is asked for anything: first what needs no plan
 * (the hop a power of two 8 .. 1024, ninputs and nbeams in their ranges, nframes, first_frame_index, the layout, the
 * strides for M = 16, the array, the weights, the output), then a null plan, then what the plan decides (the hop, the
 * grid, ninputs and nbeams, the strides for M, the captures' pointers).  0; -1 bad argument; -3 HIP failure. */
int rtlws_pfbbf_run(rtlws_pfbbf_plan* p, const void* const* d_iq_cu8, int ninputs, const float* d_weights, int nbeams,
                    long nframes, int hop, long first_frame_index, int layout, void* d_out_cf32, long out_stride,
                    long beam_stride, void* stream);

/* Power mode.  The captures and the weights as for rtlws_pfbbf_run, each capture
 * rtlws_pfbbf_samples_needed(.., k_avg, nspectra) cmplx_u8.  d_out: nspectra * nbeams rows of M f32, row_stride floats
 * apart (>= M, a multiple of 4), 16-byte aligned; nothing outside the rows is written.  One kernel launch and no other
 * runtime call; nspectra == 0 does nothing.  The refusals in rtlws_pfbbf_run's two steps: first the hop, k_avg,
 * shifted, ninputs, nbeams, nspectra, row_stride >= 16 and its multiple, the pointers; then a null plan; then what the
 * plan decides.  0; -1 bad argument; -3 HIP failure. */
int rtlws_pfbbf_power(rtlws_pfbbf_plan* p, const void* const* d_iq_cu8, int ninputs, const float* d_weights, int nbeams,
                      long nspectra, int hop, int k_avg, int shifted, float* d_out, long row_stride, void* stream);

void rtlws_pfbbf_close(rtlws_pfbbf_plan* p);

/* Last error text of the calling thread from this library ("" when none). */
const char* rtlws_pfbbf_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* RTLWS_PFBBF_H */
