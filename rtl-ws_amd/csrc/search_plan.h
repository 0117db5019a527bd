// search_plan.h -- the host side the waterfall-and-series family shares (dedisp_shim.hip, pulse_shim.hip, fold_shim.hip,
// ffa_shim.hip, cdd_shim.hip, cand_shim.hip, clean_shim.hip, subdedisp_shim.hip, sift_shim.hip, cutout_shim.hip): the head every opaque plan type derives
// from with its open, close and the head of a run; the rules more than one library states, each worded once and returning
// its text or nullptr; the band's dispersion formula; the moments of a series.  A shim composes the rules in the order its
// header documents.  Internal linkage, like shim_common.h: a library has one shim.
#ifndef RTLWS_CSRC_SEARCH_PLAN_H
#define RTLWS_CSRC_SEARCH_PLAN_H

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "shim_common.h"

namespace rtlws {
namespace search {
namespace {

// the limits of the rules below; a shim holds its csrc/<name>.h and its public header to them
constexpr int MIN_NCHAN = 4, MAX_NCHAN = 4096, MAX_TRIALS = 65536, MIN_BINS = 2, MAX_BINS = 256, MAX_WIDTHS = 16;
constexpr long MAX_NSAMP = 1L << 30;

// ---- the plan and its life ----
struct Plan {
    rtlws_engine* engine;
    int device;
};

// a table of the host's onto the current device
template <typename T>
[[maybe_unused]] hipError_t upload(T** d, const T* host, size_t count)
{
    const hipError_t err = hipMalloc(reinterpret_cast<void**>(d), count * sizeof(T));
    return err != hipSuccess ? err : hipMemcpy(*d, host, count * sizeof(T), hipMemcpyHostToDevice);
}

// rtlws_*_open of plan type PlanT (derived from Plan): `why` is the verdict of the library's own rules.  fill(plan), on a
// zeroed plan that carries the engine and its device, uploads the tables, allocates the workspace and loads the kernels.
// Where it fails, `what` names what can, the text is recorded and close(plan), the library's own rtlws_*_close, frees what
// there is: a pointer never allocated is null there.  Close is the one place that frees
template <typename PlanT, typename Fill, typename Close>
PlanT* open_plan(const char* fn, const char* why, rtlws_engine* e, Fill&& fill, const char* what, Close&& close)
{
    g_err.clear();
    const int device = open_device(fn, why, e);
    if (device < 0) return nullptr;
    PlanT* p = new PlanT{};
    p->engine = e, p->device = device;
    const hipError_t err = fill(*p);
    if (err != hipSuccess) {
        fail_hip(fn, what, err);
        close(p);
        return nullptr;
    }
    return p;
}

// rtlws_*_close: the plan's device pointers `d` (members of PlanT; null ones are nothing to free), then the plan
template <typename PlanT, typename... Ts>
void close_plan(PlanT* p, Ts* PlanT::*... d)
{
    if (!p) return;
    if (hipSetDevice(p->device) == hipSuccess) ((void)hipFree(p->*d), ...);
    delete p;
}

// the head of a run, behind its refusals: 0, or -3 with the text recorded
[[maybe_unused]] int use_device(const char* fn, const Plan* p)
{
    const hipError_t err = hipSetDevice(p->device);
    return err == hipSuccess ? 0 : fail_hip(fn, "hipSetDevice", err);
}

// ---- the rules more than one library states ----
[[maybe_unused]] const char* why_not_nchan(int nchan)
{
    return nchan < MIN_NCHAN || nchan > MAX_NCHAN || nchan % 4 ? "nchan must be 4 .. 4096 and a multiple of 4" : nullptr;
}
[[maybe_unused]] const char* why_not_ntrials(int ntrials) { return ntrials < 1 || ntrials > MAX_TRIALS ? "ntrials must be 1 .. 65536" : nullptr; }
[[maybe_unused]] const char* why_not_nsamp(long nsamp) { return nsamp < 0 || nsamp > MAX_NSAMP ? "nsamp must be 0 .. 2^30" : nullptr; }
[[maybe_unused]] const char* why_not_nbins(int nbins) { return nbins < MIN_BINS || nbins > MAX_BINS ? "nbins must be 2 .. 256" : nullptr; }

// the stride of series, of rows that may be any length, and of rows against the plan's channels
[[maybe_unused]] const char* why_not_stride(long in_stride) { return in_stride % 4 ? "in_stride must be a multiple of 4" : nullptr; }
[[maybe_unused]] const char* why_not_stride_of_rows(long in_stride)
{
    return in_stride < 4 || in_stride % 4 ? "in_stride must be >= 4 and a multiple of 4" : nullptr;
}
[[maybe_unused]] const char* why_not_row_stride(long in_stride, int nchan) { return in_stride < nchan ? "in_stride must be >= nchan" : nullptr; }

// a grid of a * b workgroups, b >= 1
[[maybe_unused]] const char* why_not_grid(long a, long b) { return a > INT_MAX / b ? "more workgroups than one grid holds" : nullptr; }

// a table of boxcar widths: every entry 1 .. max_width, in the library's words `why_width`
[[maybe_unused]] const char* why_not_widths(int nwidths, const int32_t* widths, int max_width, const char* why_width)
{
    if (nwidths < 1 || nwidths > MAX_WIDTHS) return "nwidths must be 1 .. 16";
    if (!widths) return "null widths";
    for (int k = 0; k < nwidths; ++k) {
        if (widths[k] < 1 || widths[k] > max_width) return why_width;
        if (k && widths[k] <= widths[k - 1]) return "the widths must be strictly ascending";
    }
    return nullptr;
}

[[maybe_unused]] const char* why_not_steps(const uint64_t* steps, const uint64_t* phases)
{
    return !steps ? "null steps" : !phases ? "null phases" : nullptr;
}

[[maybe_unused]] long ceil_div(long a, long b) { return (a + b - 1) / b; }

[[maybe_unused]] int log2_of(int v)
{
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

// p is not aligned to n bytes, n a power of two (null is aligned)
[[maybe_unused]] bool misaligned(const void* p, unsigned n) { return reinterpret_cast<uintptr_t>(p) & (n - 1); }

// ---- the band: M channels of bandwidth_hz / M around f_centre_hz, channel c < M / 2 above the centre ----
constexpr double DISPERSION = 4.148808e3;                     // seconds MHz^2 of delay per unit of dispersion measure

[[maybe_unused]] const char* why_not_band(int M, double f_centre_hz, double bandwidth_hz, double row_seconds)
{
    if (!(std::isfinite(bandwidth_hz) && bandwidth_hz > 0.0)) return "bandwidth_hz must be finite and > 0";
    if (!(std::isfinite(row_seconds) && row_seconds > 0.0)) return "row_seconds must be finite and > 0";
    // the lowest channel is c = M / 2, half the band below the centre
    if (!(std::isfinite(f_centre_hz) && f_centre_hz + (double)(M / 2 - M) * bandwidth_hz / (double)M > 0.0))
        return "every channel's frequency must be finite and > 0";
    return nullptr;
}

// nu_i^-2 - nu_max^-2 of position i, nu in MHz; shifted: position i holds channel (i + M / 2) % M
[[maybe_unused]] std::vector<double> excess(int M, int shifted, double f_centre_hz, double bandwidth_hz)
{
    std::vector<double> x(M);
    const double top = (f_centre_hz + (double)(M / 2 - 1) * bandwidth_hz / (double)M) / 1e6;
    for (int i = 0; i < M; ++i) {
        const int c = shifted ? (i + M / 2) % M : i;
        const double nu = (f_centre_hz + (double)(c < M / 2 ? c : c - M) * bandwidth_hz / (double)M) / 1e6;
        x[i] = 1.0 / (nu * nu) - 1.0 / (top * top);
    }
    return x;
}

// ---- the moments of `count` samples from their sum and their sum of squares; false: no variance to divide by ----
[[maybe_unused]] bool moments(double sum1, double sum2, long count, double* mean, double* var)
{
    if (count < 2) return false;
    *mean = sum1 / (double)count;
    *var = sum2 / (double)count - *mean * *mean;
    return *var > 0.0;
}

}  // namespace
}  // namespace search
}  // namespace rtlws
#endif
