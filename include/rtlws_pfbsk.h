/*
 * rtlws_pfbsk.h -- polyphase spectrometer with spectral-kurtosis excision: the power of all M = 2^k channels of one
 * capture, summed over those of L short sub-integrations of K frames that pass a per-channel test of their
 * kurtosis, with the number kept, in one launch (librtlws_pfbsk.so).
 *
 * rtlws_pfbspec_run (rtlws_pfbspec.h) integrates K frames into a row; interference that is on for a part of a long
 * integration ruins its channel's whole row.  The spectral-kurtosis estimator judges a short sub-integration by two
 * sums, S1 = sum P and S2 = sum P^2: K S2 / S1^2 is 2 for Gaussian noise, 1 for a steady carrier and large for a
 * burst.  rtlws_pfbsk_run forms both where the power is formed, drops the sub-integrations whose ratio leaves a band
 * and adds the rest in a fixed order (tests/pfbsk_ref.py restates it in numpy).  Neither the
 * channelizer's samples nor the short rows reach device memory unless the caller asks for the rows.
 *
 * M, T, the prototype h, the hop D, the capture x and Y[m][c] are rtlws_pfbspec.h's.  K = k_avg, 1 .. 65536, frames
 * per sub-integration; L = nsub, 1 .. 65535, sub-integrations per output row; sub-integration q = j L + l holds the
 * frames q K .. q K + K - 1.  Every operation is f32, rounded once, no fused multiply-add:
 *   P        = fl(fl(re re) + fl(im im))                  rtlws_pfbspec.h's P
 *   S1[q][c] = sum P                                       in the spectrometer's order for (M, K)
 *   p        = fl(P power_scale)
 *   S2[q][c] = sum fl(p p)                                 in that same order
 *   s = fl(S1 power_scale), u = fl(s s), v = fl((float)K S2)
 *   flagged  <=>  v < fl(ratio_lo u)  or  v > fl(ratio_hi u)          both false on NaN
 *   C[j][c]  = ((+0 + S1[j L + l0][c]) + S1[j L + l1][c]) + ..         over the kept l, ascending
 *   N[j][c]  = their number, uint32
 * S1[q] is rtlws_pfbspec_run's row q at the same K bit for bit; with nothing flagged and L = 1, C is that row whatever
 * power_scale is.  All-128 input (u = v = 0) is kept and adds +0.  The order of every addition is a function of
 * (M, K, L) alone and no atomics take part: two runs give the same bits, and a run over the capture from sample
 * j0 L K D on gives rows j0 .. of the whole run bit for bit.
 *
 * power_scale, a finite float > 0, reaches S2 and the decision only.  It is there because P^2 leaves the f32 range for
 * ordinary prototypes at M = 1024; rtlws_pfbsk_power_scale() returns one that keeps p <= 2 for any capture.
 * ratio_lo and ratio_hi bound K S2 / S1^2 itself: 0 <= ratio_lo <= ratio_hi, ratio_lo finite, ratio_hi finite or
 * +inf (no upper test).  rtlws_pfbsk_bounds() forms them from thresholds on the estimator
 * ((K + 1) / (K - 1)) (K S2 / S1^2 - 1), which is 1 for Gaussian noise.
 *
 * The capture holds rtlws_pfbsk_samples_needed() = (nspectra L K - 1) D + T M samples and no byte beyond is read.
 *
 * Outputs, rows of M values, value i channel i (shifted = 0) or channel (i + M / 2) mod M (shifted = 1):
 *   d_clean   row j at d_clean + j * clean_stride, of the kind `output` (the values of enum rtlws_output):
 *               RTLWS_OUT_POWER_SUM   f32 C, raw; scale is ignored
 *               RTLWS_OUT_MEAN_DB     f32 10 log10(C lin), lin = fl(scale / fl((float)K (float)N[j][c])) per channel
 *               RTLWS_OUT_PAYLOAD_U8  one byte per channel: that dB value truncated by (int) and clamped to 0 .. 255
 *             a channel with N = 0 reads exactly -inf and byte 0
 *   d_kept    uint32 N, row j at d_kept + j * kept_stride; NULL: not written
 *   d_s1, d_s2  the raw f32 S1 and S2, row q at d_s1 + q * sub_stride and d_s2 + q * sub_stride, nspectra L rows each;
 *             both NULL (not written) or both given.  The estimator, a waterfall of it or another decision rule are
 *             pointwise functions of these rows.
 * Strides are in elements.  Nothing outside the rows is written.
 *
 * Parallelism is across output rows: a workgroup owns a whole row and walks its L sub-integrations in order.
 *
 * Refused with -1 (rtlws_pfbsk_last_error() says why): log2_channels outside 4 .. 10, taps_per_branch outside
 * 1 .. 32, a hop that is neither M nor M / 2, k_avg outside 1 .. 65536, nsub outside 1 .. 65535, an unknown output,
 * shifted other than 0 or 1, a scale that is not finite or <= 0 (dB and payload), a power_scale that is not finite or
 * <= 0, ratio bounds outside their ranges, nspectra < 0 or more than one grid holds, a stride < M or not a multiple
 * of 4 (f32 and uint32 rows) or 16 (byte rows), one of d_s1 and d_s2 null and the other not, null pointers, a
 * pointer that is not 16-byte aligned.
 */
#ifndef RTLWS_PFBSK_H
#define RTLWS_PFBSK_H

#include <stdint.h>

#include "rtlws_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* librtlws_pfbsk.so exports these declarations and nothing else (exports/pfbsk.map) */
#pragma GCC visibility push(default)

#define RTLWS_PFBSK_MAX_K_AVG 65536
#define RTLWS_PFBSK_MAX_NSUB 65535

typedef struct rtlws_pfbsk_plan rtlws_pfbsk_plan;

/* 1 when the shape is served, else 0 (rtlws_pfbsk_last_error() says why).  hop: M or M / 2; output: a value of enum
 * rtlws_output.  Needs no GPU. */
int rtlws_pfbsk_supported(int log2_channels, int taps_per_branch, int hop, int k_avg, int nsub, int output);

/* Samples of the capture that nspectra rows read: (nspectra nsub k_avg - 1) hop + T M, 0 for nspectra == 0; -1 when
 * the shape is not served or nspectra < 0.  Needs no GPU. */
long rtlws_pfbsk_samples_needed(int log2_channels, int taps_per_branch, int hop, int k_avg, int nsub, long nspectra);

/* Launch geometry: workgroups, threads per workgroup, bytes of LDS per workgroup, output rows per workgroup (1).  Any
 * pointer may be NULL.  0, or -1 when the shape is not served.  Needs no GPU. */
int rtlws_pfbsk_grid(int log2_channels, int taps_per_branch, int hop, int k_avg, int nsub, long nspectra, int* blocks,
                     int* threads, int* lds_bytes, int* rows_per_block);

/* 2^(-2 ceil(log2(128 sum|h|))) of the prototype (taps_per_branch * M int16 in host memory): |re| and |im| of Y stay
 * within 128 sum|h|, so p <= 2 for any capture and S2 and K S2 stay finite for every K.  1.0f for an all-zero
 * prototype.  0 (rtlws_pfbsk_last_error() says why) on a shape that is not served or null taps.  Needs no GPU. */
float rtlws_pfbsk_power_scale(int log2_channels, int taps_per_branch, const int16_t* taps);

/* Thresholds on the estimator to bounds on the ratio: ratio = 1 + sk (K - 1) / (K + 1), formed in double and rounded
 * once.  sk_hi = +INFINITY gives +INFINITY: no upper test.  0; -1 for k_avg outside 2 .. 65536, sk_lo < 0,
 * sk_lo > sk_hi or a NaN.  Either pointer may be NULL.  Needs no GPU. */
int rtlws_pfbsk_bounds(int k_avg, double sk_lo, double sk_hi, float* ratio_lo, float* ratio_hi);

/* The prototype (taps_per_branch * M int16 in host memory, read before the call returns) and the transform's table
 * (the bits of rtlws_pfb_twiddles) on the engine's device and the kernel loaded, so that rtlws_pfbsk_run makes no
 * runtime call other than its launch and may be captured into a hipGraph.  A new prototype is a new plan.  NULL on
 * failure (a null engine among them: without a device there is no engine, and no CPU path). */
rtlws_pfbsk_plan* rtlws_pfbsk_open(rtlws_engine* e, int log2_channels, int taps_per_branch, const int16_t* taps);

/* d_iq_cu8: rtlws_pfbsk_samples_needed() cmplx_u8.  d_clean: nspectra rows of M f32 or M bytes; d_kept: NULL or
 * nspectra rows of M uint32; d_s1, d_s2: both NULL or nspectra nsub rows of M f32 each.  Every pointer 16-byte
 * aligned.  Asynchronous on `stream` (NULL = the engine's own stream, RTLWS_STREAM_DEFAULT = HIP's: "Streams" in
 * rtlws_hip.h); one kernel launch and no other runtime call.  nspectra == 0 does nothing.  Every refusal is made
 * before the device is asked for anything: first what needs no plan (the hop a power of two 8 .. 1024, k_avg, nsub,
 * the output, shifted, scale, power_scale, the ratio bounds, nspectra, then of d_clean, d_kept and the pair d_s1,
 * d_s2 in turn the stride >= 16 and its multiple, then d_s1 and d_s2 both or neither, null pointers, the pointers'
 * alignment), then a null plan, then what the plan's M decides (the hop, the grid, every stride >= M).
 * 0; -1 bad argument; -3 HIP failure. */
int rtlws_pfbsk_run(rtlws_pfbsk_plan* p, const void* d_iq_cu8, long nspectra, int hop, int k_avg, int nsub, float power_scale,
                    float ratio_lo, float ratio_hi, int output, int shifted, float scale, void* d_clean, long clean_stride,
                    uint32_t* d_kept, long kept_stride, float* d_s1, float* d_s2, long sub_stride, void* stream);

void rtlws_pfbsk_close(rtlws_pfbsk_plan* p);

/* Last error text of the calling thread from this library ("" when none). */
const char* rtlws_pfbsk_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* RTLWS_PFBSK_H */
