/*
 * rtlws_cdd.h -- coherent dedispersion of channelizer streams: every channel's complex f32 voltages are convolved with
 * the channel's own filter, a table of N frequency-domain factors (the conjugate of the cold-plasma phase across the
 * channel: rtlws_cdd_chirp), by overlap-save over segments of N points, all segments of all channels in one launch; the
 * voltages come back, or their power summed over ksum samples without the voltages reaching memory (librtlws_cdd.so).
 *
 * rtlws_pfb_run (rtlws_pfb.h) leaves nchan streams on the device in RTLWS_PFB_CHANNEL_MAJOR; this library reads them
 * where they lie.  rtlws_dedisp_run (rtlws_dedisp.h) moves whole rows of detected power, so the sweep inside one
 * channel's bandwidth stays in its series; here it is undone on the voltages at a fiducial DM, and the time-major power
 * rows are the waterfall rtlws_dedisp_run reads for the residual trials (tests/cdd_ref.py restates it in
 * f64 numpy).
 *
 *   N = 2^log2_nfft, log2_nfft 9 .. 14      points of a segment
 *   lead, trail >= 0                        points dropped at the head and at the tail of every segment
 *   hop = N - lead - trail >= 1             outputs of a segment, and the step from a segment to the next
 *   nchan 1 .. 1024
 *   x_c[i]     complex f32 (re, im) on the device, channel c at d_in + c * in_stride (in complex elements; 8-byte aligned)
 *   H_c[k]     complex f32 (re, im), k = 0 .. N - 1 in natural bin order: nchan * N pairs in host memory at open
 *
 *   for segment s = 0 .. nseg - 1 and j = 0 .. hop - 1:
 *   X_s[k]         = sum_{m < N} x_c[s hop + m] e^(-2 pi i m k / N)
 *   y_c[s hop + j] = (1 / N) sum_{k < N} H_c[k] X_s[k] e^(+2 pi i (j + lead) k / N)
 *
 * Output sample j is the circular convolution of the segment with the filter at point j + lead: where the filter's
 * impulse response lies within [-trail, lead], that is the linear convolution, and output i answers input i + lead.
 * Any table is served; what lead and trail a table needs is the caller's to say (rtlws_cdd_overlap for the chirp).
 *
 * The transforms are f32 with once-rounded twiddles (csrc/row_fft.h: forward, and its conjugate transpose back); the
 * product H X is one complex f32 multiplication; 1 / N and the conjugations are exact.  Segments are independent and no
 * atomics take part: two runs give the same bits, and a run whose d_in is advanced by s0 hop elements gives outputs
 * s0 hop .. of the whole run bit for bit.  DESIGN.md 4.26 derives the error bounds tests/cdd_ref.py carries.
 *
 * The run reads elements 0 .. (nseg - 1) hop + N - 1 of every channel (rtlws_cdd_samples_needed) and no byte beyond.
 * What it writes is chosen at open by ksum:
 *   ksum == 0   voltages, complex f32: y_c[i] at d_out + 2 (c out_stride + i) floats, i = 0 .. nseg hop - 1; out_stride
 *               (complex elements) >= nseg hop; the layout must be RTLWS_CDD_CHANNEL_MAJOR; d_out 8-byte aligned
 *   ksum 1 .. hop, dividing hop   power rows, f32, r = 0 .. nseg hop / ksum - 1:
 *               P[r][c] = (((+0 + p(y_c[r ksum])) + p(y_c[r ksum + 1])) + ..) over ksum samples in ascending order,
 *               p(y) = fl(fl(re re) + fl(im im)), one f32 accumulator and one rounding per addition
 *               RTLWS_CDD_TIME_MAJOR:    P[r][c] at d_out + r out_stride + c, out_stride >= nchan: the waterfall
 *               RTLWS_CDD_CHANNEL_MAJOR: P[r][c] at d_out + c out_stride + r, out_stride >= nseg hop / ksum
 * The power rows are, bit for bit, that expression over the voltages a ksum == 0 plan of the same log2_nfft, lead, trail
 * and table writes.  Nothing outside the stated ranges is written; nseg == 0 does nothing.
 *
 * One workgroup of max(64, N / 16) threads per (segment, channel) holds the segment in 8.5 N bytes of LDS (136 KiB at
 * 2^14): rtlws_cdd_geometry says what a run launches.
 *
 * Refused with -1 (rtlws_cdd_last_error() says why): log2_nfft outside 9 .. 14, a negative lead or trail, hop below 1,
 * nchan outside 1 .. 1024, ksum outside 0 .. hop or not dividing hop, a null table, nseg outside 0 .. 1048576, an
 * unknown layout, time-major voltages, a stride too small, null pointers, d_in not 8-byte aligned, d_out not 8-byte
 * (voltages) or 4-byte (power) aligned.
 */
#ifndef RTLWS_CDD_H
#define RTLWS_CDD_H

#include <stddef.h>
#include <stdint.h>

#include "rtlws_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* librtlws_cdd.so exports these declarations and nothing else (exports/cdd.map) */
#pragma GCC visibility push(default)

#define RTLWS_CDD_MIN_LOG2_NFFT 9
#define RTLWS_CDD_MAX_LOG2_NFFT 14
#define RTLWS_CDD_MAX_NCHAN 1024
#define RTLWS_CDD_MAX_NSEG 1048576
/* channel c is the contiguous series at d_out + c * out_stride */
#define RTLWS_CDD_CHANNEL_MAJOR 0
/* power row r is the nchan values at d_out + r * out_stride: the waterfall (power rows only) */
#define RTLWS_CDD_TIME_MAJOR 1

typedef struct rtlws_cdd_plan rtlws_cdd_plan;

/* 1 when the shape is served, else 0 (rtlws_cdd_last_error() says why).  Needs no GPU. */
int rtlws_cdd_supported(int log2_nfft, int lead, int trail, int nchan, int ksum);

/* What a run of nseg segments launches: workgroups (nseg * nchan, a grid of nseg by nchan), threads per workgroup
 * (max(64, N / 16)) and bytes of LDS per workgroup (8 (N + N / 16)).  Any of the pointers may be NULL.  0, or -1 when
 * the shape is not served or nseg is outside 0 .. 1048576.  Needs no GPU. */
int rtlws_cdd_geometry(int log2_nfft, int lead, int trail, int nchan, int ksum, long nseg, int* blocks, int* threads,
                       int* lds_bytes);

/* The tables (nchan * N pairs (re, im) of f32 in host memory, channel c's N entries from tables + 2 c N on, natural bin
 * order, read before the call returns) on the engine's device in the kernel's order, the transform's twiddles beside
 * them and the kernel loaded, so that rtlws_cdd_run makes no runtime call other than its launch and may be captured
 * into a hipGraph.  New tables are a new plan.  NULL on failure (a null engine among them: without a device there is no
 * engine, and no CPU path). */
rtlws_cdd_plan* rtlws_cdd_open(rtlws_engine* e, int log2_nfft, int lead, int trail, int nchan, int ksum, const float* tables);

/* Complex elements of a channel that nseg segments read: (nseg - 1) hop + N, 0 for nseg == 0; -1 for a null plan or
 * nseg < 0. */
long rtlws_cdd_samples_needed(const rtlws_cdd_plan* p, long nseg);

/* d_in: nchan streams of rtlws_cdd_samples_needed() complex f32, in_stride complex elements apart, 8-byte aligned;
 * d_out: what the plan's ksum says above.  Asynchronous on `stream` (NULL = the engine's own stream,
 * RTLWS_STREAM_DEFAULT = HIP's: "Streams" in rtlws_hip.h); one kernel launch and no other runtime call.  nseg == 0 does
 * nothing.  Every refusal is made before the device is asked for anything, in this order: nseg, the layout, null
 * pointers (d_in, d_out), the alignments of d_in (8 bytes) and d_out (4 bytes), then a null plan, then what the plan
 * decides (time-major voltages, d_out 8-byte aligned for voltages, in_stride at least samples_needed, out_stride).
 * 0; -1 bad argument; -3 HIP failure. */
int rtlws_cdd_run(rtlws_cdd_plan* p, const float* d_in, long in_stride, long nseg, float* d_out, long out_stride, int layout,
                  void* stream);

/* The dedispersing table of one channel of N = 2^log2_nfft bins, centred on f_centre_mhz and sampled at rate_mhz complex
 * samples per microsecond (a negative rate: an inverted channel), for the dispersion measure dm (pc cm^-3), in double:
 *   f_k   = (k < N / 2 ? k : k - N) rate / N                                   MHz from the centre
 *   phi_k = 4.148808e3 * 1e6 * dm * f_k^2 / (f0^2 (f0 + f_k))  cycles, less rint of itself
 *   re_im[2 k], re_im[2 k + 1] = cos(2 pi phi_k), -sin(2 pi phi_k), each rounded to f32 once
 * 4.148808e3 is rtlws_dedisp_delays' constant.  Dispersion delays frequency nu by 4.148808e3 dm nu^-2 seconds; less the
 * constant and the delay at f0 that is the phase +2 pi phi_k on bin k of the transform above, and the table is its
 * conjugate.  0; -1 for log2_nfft outside 9 .. 14, a null table, an argument that is not finite, a band edge
 * f0 - |rate| / 2 that is not positive, a zero rate or a negative dm.  Needs no GPU. */
int rtlws_cdd_chirp(int log2_nfft, double f_centre_mhz, double rate_mhz, double dm, float* re_im);

/* The least overlap a plan of that table should be opened with: the delay of the band's edges against its centre in
 * samples,  tau(f) = 4.148808e3 * 1e6 * dm * ((f0 + f)^-2 - f0^-2) |rate|  at f = -|rate| / 2 (positive: the low edge
 * arrives late, the filter looks ahead by it) and at f = +|rate| / 2 (negative):
 *   *trail = ceil(tau(-|rate| / 2)),  *lead = ceil(-tau(+|rate| / 2))
 * 0; -1 for what rtlws_cdd_chirp refuses, null pointers, or a delay above 2^30.  Needs no GPU. */
int rtlws_cdd_overlap(double f_centre_mhz, double rate_mhz, double dm, int* lead, int* trail);

void rtlws_cdd_close(rtlws_cdd_plan* p);

/* Last error text of the calling thread from this library ("" when none). */
const char* rtlws_cdd_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* RTLWS_CDD_H */
