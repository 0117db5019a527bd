/*
 * rtlws_ffa.h -- fast folding search of dedispersed time series: every trial's series is folded at m = 2^L periods
 * between p and p + 1 samples for every base period p of a range, in log2 m rounds of shifted row additions (the Fast
 * Folding Algorithm, Staelin 1969), and for every segment of the m profiles the largest circular boxcar sum of every
 * width of a table and where it lies come back (librtlws_ffa.so).
 *
 * rtlws_dedisp_run (rtlws_dedisp.h) leaves ntrials f32 series on the device; this library reads them where they lie
 * (tests/ffa_ref.py restates it in numpy).  It is the time-domain search for long periods and narrow
 * pulses: N log2 m additions where rtlws_fold_run spends N m.
 *
 *   D[t][n]   f32 on the device, trial t at d_in + t * in_stride (elements; a multiple of 4; d_in 16-byte aligned)
 *   p_i = p0 + i, i = 0 .. nper-1    base periods in samples = phase bins of a profile;  16 <= p0,  p0 + nper - 1 <= 1024
 *   m = 2^L, 1 <= L <= 12            rows;  m * (p0 + nper - 1) <= 2^22;   every trial holds that many samples
 *   w_k, k = 0 .. nwidths-1          int32 table in host memory at open, strictly ascending, 1 .. min(256, p0);  nwidths 1 .. 16
 *   seg                              rows per segment of the peaks: a power of two, 1 .. m;  nseg = m / seg
 *
 *   A_0[r][c] = D[t][r * p + c]                                           r = 0 .. m-1, c = 0 .. p-1   (p = p_i)
 *   stage j = 1 .. L, blocks of 2^j rows from row g (g a multiple of 2^j), s = 0 .. 2^j - 1:
 *   A_j[g + s][c] = fl( A_(j-1)[g + (s >> 1)][c]  +  A_(j-1)[g + 2^(j-1) + (s >> 1)][(c + ((s + 1) >> 1)) mod p] )
 *   prof[t][i][s][c] = A_L[s][c]       -- the series folded at  p + s / (m - 1)  samples (rtlws_ffa_period)
 *
 *   P_0[c] = prof[c];   P_(l+1)[c] = fl(P_l[c] + P_l[(c + 2^l) mod p])
 *   B_w[c] = rtlws_pulse.h's combination for w = 2^a1 + .. + 2^am, a1 > .. > am, every index taken mod p:
 *            fl(..fl(P_a1[c] + P_a2[(c + 2^a1) mod p]) + P_a3[(c + 2^a1 + 2^a2) mod p] ..)
 *   peak, at [t][i][g][k]:  best = -Inf; at = -1;
 *       for s = g*seg .. (g+1)*seg - 1 ascending, c = 0 .. p-1 ascending:
 *           if B_wk(prof[t][i][s])[c] > best:  best = that; at = s * p + c
 *
 * Every addition is one f32 rounding, and the tree of additions depends on (L, s, c, w) alone -- not on the trial, the
 * grid or how the plan splits the stages into passes -- and no atomics take part: two runs give the same bits.  The
 * comparison is strict: NaN never wins, among equal values (+0.0 and -0.0 are equal) the least index wins with its own
 * bits, and a segment with nothing above -Inf gives (-Inf, -1).  A NaN is promised as a NaN at its place, not its
 * payload.  The library only adds floats: subnormal sums are kept, a non-finite sample reaches the sums it enters and
 * no others.
 *
 * The run reads samples 0 .. m * (p0 + nper - 1) - 1 of every trial (rtlws_ffa_samples_needed), nothing in the stride's
 * padding and nothing at or beyond that index.  It writes d_peak[((t * nper + i) * nseg + g) * nwidths + k] (f32), d_at
 * in the same layout (int32) and, only when d_prof is not NULL, d_prof[((t * nper + i) * m + s) * prof_stride + c] for
 * c < p_i (columns p_i .. prof_stride - 1 stay untouched), and nothing else.  Strides are in elements.  The input
 * layout is what rtlws_dedisp_run writes when out_stride is a multiple of 4: the two libraries chain on the device with
 * no copy.
 *
 * The plan splits the L stages into 1 .. 3 passes.  One pass kernel serves every pass: for the stages a + 1 .. b, with
 * the blocks of 2^a rows finished before, a workgroup of 512 threads takes one superblock of 2^b rows from row B0 and
 * one q = 0 .. 2^a - 1, loads the 2^(b-a) rows B0 + i 2^a + q into LDS, runs the stages there as a small transform
 * whose shift at stage j is ((s_j + 1) >> 1), s_j = (q << (j - a)) | u for the row u of a local block, and stores the
 * rows B0 + q 2^(b-a) + u, which are contiguous.  That is the same tree of additions as the definition's (DESIGN.md
 * 4.25).  A wavefront owns a row at a time and its lanes run along c.  Two copies of the tile and a (best, at) pair
 * per width and row have to fit the CU's 160 KiB: a pass has as many stages as fit at p0 + nper - 1 columns, never more
 * than 7, and the stages are dealt evenly over as few passes as that allows.  The first pass reads the series, the
 * others go through the plan's workspace, whose size is capped at RTLWS_FFA_WORKSPACE_CAP: a run of more (trial, base
 * period) pairs than the workspace holds is worked in groups, one after the other.  The last pass also evaluates its
 * rows while they are in LDS and, with a NULL d_prof, stores no profile.  Where seg exceeds the rows of a workgroup of
 * the last pass, the workgroups' partial pairs go through the workspace and one small merge launch; the strict rule
 * makes the order in which partial pairs meet irrelevant.  rtlws_ffa_geometry says what a plan launches.
 *
 * Refused with -1 (rtlws_ffa_last_error() says why): p0 below 16, nper below 1, p0 + nper - 1 above 1024, L outside
 * 1 .. 12, more than 2^22 cells, nwidths outside 1 .. 16, a null table, a width outside 1 .. min(256, p0) or not above
 * the one before, seg not a power of two 1 .. m, max_trials below 1, ntrials outside 1 .. 65536, in_stride not a
 * multiple of 4 or below samples_needed, null pointers, d_in not 16-byte aligned, d_peak, d_at or d_prof not 4-byte
 * aligned, prof_stride below p0 + nper - 1 with a d_prof.  Every grid a run launches holds its workgroups by
 * construction (at most 4096 by at most 65535), so no run is refused for its grid.
 */
#ifndef RTLWS_FFA_H
#define RTLWS_FFA_H

#include <stddef.h>
#include <stdint.h>

#include "rtlws_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
/* librtlws_ffa.so exports these declarations and nothing else (exports/ffa.map) */
#pragma GCC visibility push(default)

#define RTLWS_FFA_MIN_P 16
#define RTLWS_FFA_MAX_P 1024
#define RTLWS_FFA_MAX_L 12
#define RTLWS_FFA_MAX_CELLS 4194304
#define RTLWS_FFA_MAX_WIDTHS 16
#define RTLWS_FFA_MAX_WIDTH 256
#define RTLWS_FFA_MAX_TRIALS 65536
#define RTLWS_FFA_MAX_PASSES 3
#define RTLWS_FFA_WORKSPACE_CAP 1073741824

typedef struct rtlws_ffa_plan rtlws_ffa_plan;

/* 1 when the base periods, L, the table and seg are served, else 0 (rtlws_ffa_last_error() says why).  Needs no GPU. */
int rtlws_ffa_supported(int p0, int nper, int L, int nwidths, const int32_t* widths, int seg);

/* What a plan launches: the number of passes (1 .. 3); per pass (arrays of RTLWS_FFA_MAX_PASSES, 0 behind the last
 * pass) its stages, which add to L, its workgroups per (trial, base period) pair (m / 2^stages) and its bytes of LDS per
 * workgroup (at most 163840); threads per workgroup (512); merge, 1 when seg exceeds the 2^stages rows of a workgroup of
 * the last pass, so that a merge launch follows it, else 0; the bytes of the plan's workspace; and the (trial, base
 * period) pairs in flight, min(max_trials * nper, 65535, what RTLWS_FFA_WORKSPACE_CAP holds), at least 1: a run's
 * launches are ceil(ntrials * nper / pairs) * (passes + merge).  Any of the pointers may be NULL.  0, or -1 when the
 * arguments are not served.  Needs no GPU. */
int rtlws_ffa_geometry(int p0, int nper, int L, int nwidths, const int32_t* widths, int seg, int max_trials, int* passes,
                       int* stages, int* blocks, int* threads, int* lds_bytes, int* merge, size_t* workspace_bytes, int* pairs);

/* The table (nwidths int32 in host memory, read before the call returns) on the engine's device in the kernel's form,
 * the workspace allocated and the kernels loaded, so that rtlws_ffa_run makes no runtime call other than its launches
 * and may be captured into a hipGraph.  max_trials sizes the workspace; a run may bring more trials.  NULL on failure
 * (a null engine among them: without a device there is no engine, and no CPU path). */
rtlws_ffa_plan* rtlws_ffa_open(rtlws_engine* e, int p0, int nper, int L, int nwidths, const int32_t* widths, int seg, int max_trials);

/* Samples of a trial that a run reads: m * (p0 + nper - 1); -1 for a null plan. */
long rtlws_ffa_samples_needed(const rtlws_ffa_plan* p);

/* Bytes of the plan's workspace on the device (0 for a one-pass plan without a merge, and for a null plan). */
size_t rtlws_ffa_workspace_bytes(const rtlws_ffa_plan* p);

/* d_in: ntrials series of rtlws_ffa_samples_needed() f32, in_stride apart, 16-byte aligned; d_peak and d_at:
 * ntrials * nper * nseg * nwidths f32 and int32; d_prof: ntrials * nper * m rows of prof_stride f32, or NULL.
 * Asynchronous on `stream` (NULL = the engine's own stream, RTLWS_STREAM_DEFAULT = HIP's: "Streams" in rtlws_hip.h);
 * kernel launches and no other runtime call.  Every refusal is made before the device is asked for anything, in this
 * order: ntrials, in_stride a multiple of 4, null pointers (d_in, d_peak, d_at), the alignments of d_in, d_peak, d_at
 * and d_prof, then a null plan, then what the plan decides (in_stride at least samples_needed; with a d_prof,
 * prof_stride at least p0 + nper - 1).  Two runs of one plan share its workspace: they must not overlap in time.
 * 0; -1 bad argument; -3 HIP failure. */
int rtlws_ffa_run(rtlws_ffa_plan* p, const float* d_in, long in_stride, int ntrials, float* d_peak, int32_t* d_at, float* d_prof,
                  long prof_stride, void* stream);

/* The period in samples of row s at base period p of a transform of m = 2^L rows: p + s / (m - 1), in double (L = 1:
 * p + s).  NaN where p is below 1, L outside 1 .. 12 or s outside 0 .. m - 1.  Needs no GPU. */
double rtlws_ffa_period(int p, int s, int L);

/* The signal-to-noise ratio of a peak, a boxcar sum of `width` columns of a profile of `rows` rows, over noise whose
 * `count` samples add to sum1 and whose squares add to sum2 (rtlws_pulse_run's moments of the trial), in double on the
 * host:  n = width * rows;  mean = sum1 / count;  var = sum2 / count - mean * mean;  snr = (peak - n * mean) / sqrt(n * var)
 * NaN where count < 2, width < 1, rows < 1 or var is not positive.  Needs no GPU. */
double rtlws_ffa_snr(double peak, int width, int rows, double sum1, double sum2, long count);

void rtlws_ffa_close(rtlws_ffa_plan* p);

/* Last error text of the calling thread from this library ("" when none). */
const char* rtlws_ffa_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* RTLWS_FFA_H */
