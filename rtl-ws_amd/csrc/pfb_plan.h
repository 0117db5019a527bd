// pfb_plan.h -- the host side the polyphase family shares (pfb_shim.hip, pfbspec_shim.hip, pfbxc_shim.hip,
// pfbbf_shim.hip): the plan every opaque plan type derives from, its open
// and close, the fill of the bank's kernel parameters, and the bank's argument rules, each stated once and returning
// its text or nullptr.  A shim composes the rules in the order its header documents.
#ifndef RTLWS_PFB_PLAN_H
#define RTLWS_PFB_PLAN_H

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

#include "pfb_bank.h"
#include "shim_common.h"

namespace rtlws {
namespace pfb {

// The prototype and the transform's table on the engine's device
struct Plan {
    rtlws_engine* engine;
    int device;
    int log2_m, taps_per_branch;
    int16_t* d_taps;
    float2* d_tw;
};

// e^(-2 pi i j / M) in f64, rounded once; the quadrant points exactly
inline void build_twiddles(int k, float* re_im)
{
    const int M = 1 << k;
    for (int j = 0; j < M; ++j) {
        const double a = -2.0 * M_PI * (double)j / (double)M;
        double c = std::cos(a), s = std::sin(a);
        if ((4 * j) % M == 0) {
            c = std::rint(c);
            s = std::rint(s);
        }
        re_im[2 * j] = (float)c;
        re_im[2 * j + 1] = (float)s;
    }
}

inline void free_plan_arrays(int16_t* d_taps, float2* d_tw)
{
    if (d_taps) (void)hipFree(d_taps);
    if (d_tw) (void)hipFree(d_tw);
}

// The prototype (taps_per_branch * M int16 in host memory) and the table of build_twiddles on the current device.
// On failure nothing stays allocated and both pointers are null.
inline hipError_t upload_plan_arrays(int k, int taps_per_branch, const int16_t* taps, int16_t** d_taps, float2** d_tw)
{
    const size_t M = (size_t)1 << k, ntaps = M * (size_t)taps_per_branch;
    std::vector<float> tw(2 * M);
    build_twiddles(k, tw.data());
    *d_taps = nullptr;
    *d_tw = nullptr;
    hipError_t err = hipMalloc(reinterpret_cast<void**>(d_taps), ntaps * sizeof(int16_t));
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(d_tw), tw.size() * sizeof(float));
    if (err == hipSuccess) err = hipMemcpy(*d_taps, taps, ntaps * sizeof(int16_t), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(*d_tw, tw.data(), tw.size() * sizeof(float), hipMemcpyHostToDevice);
    if (err != hipSuccess) {
        free_plan_arrays(*d_taps, *d_tw);
        *d_taps = nullptr;
        *d_tw = nullptr;
    }
    return err;
}

// ---- the bank's rules ----
inline const char* why_not_bank(int k, int taps)
{
    if (k < MIN_LOG2_M || k > MAX_LOG2_M) return "log2_channels must be 4 .. 10";
    if (taps < 1 || taps > MAX_TAPS) return "taps_per_branch must be 1 .. 32";
    return nullptr;
}

inline const char* why_not_hop(int k, int hop) { return hop != 1 << k && hop != 1 << (k - 1) ? "hop must be M or M / 2" : nullptr; }

// what a run can say of the hop before it looks at its plan: a power of two 8 .. 1024
inline const char* why_not_any_hop(int hop)
{
    return hop < 8 || hop > 1 << MAX_LOG2_M || (hop & (hop - 1)) ? "hop must be M or M / 2" : nullptr;
}

inline const char* why_not_k_avg(int k_avg) { return k_avg < 1 || k_avg > MAX_K_AVG ? "k_avg must be 1 .. 65536" : nullptr; }

// count frames (spectra false) or spectra, per_workgroup of them a workgroup
inline const char* why_not_count(long count, int per_workgroup, bool spectra)
{
    if (count < 0) return spectra ? "nspectra must be >= 0" : "nframes must be >= 0";
    if (count > (long)INT_MAX * per_workgroup) return spectra ? "more spectra than one grid holds" : "more frames than one grid holds";
    return nullptr;
}

// a run of K-frame sums over a bank of 2^k channels: the hop, K, the spectra
inline const char* why_not_sums(int k, int hop, int k_avg, long nspectra)
{
    if (const char* why = why_not_hop(k, hop)) return why;
    if (const char* why = why_not_k_avg(k_avg)) return why;
    return why_not_count(nspectra, spectra_per_block(k, k_avg), true);
}

// the captures' pointers, the last of the refusals
inline const char* why_not_captures(const void* const* d_iq_cu8, int ninputs)
{
    for (int a = 0; a < ninputs; ++a) {
        if (!d_iq_cu8[a]) return "null pointer among the captures";
        if (reinterpret_cast<uintptr_t>(d_iq_cu8[a]) & 15u) return "every capture must be 16-byte aligned";
    }
    return nullptr;
}

namespace {

// rtlws_*_open of plan type P (derived from Plan; what it adds is the caller's to fill): `why` is the verdict of the
// library's shape rules, prepare(k) loads its kernels on the current device, `what` names what can fail there.
// Null with the text recorded, nothing left allocated
template <typename P, typename Prepare>
P* open_plan(const char* fn, const char* why, rtlws_engine* e, int k, int taps_per_branch, const int16_t* taps, Prepare&& prepare,
             const char* what = "the taps, the table or the kernel")
{
    if (!why && !taps) why = "null taps";
    const int device = open_device(fn, why, e);
    if (device < 0) return nullptr;
    int16_t* d_taps = nullptr;
    float2* d_tw = nullptr;
    hipError_t err = upload_plan_arrays(k, taps_per_branch, taps, &d_taps, &d_tw);
    if (err == hipSuccess) {
        err = prepare(k);
        if (err != hipSuccess) free_plan_arrays(d_taps, d_tw);
    }
    if (err != hipSuccess) {
        fail_hip(fn, what, err);
        return nullptr;
    }
    P* p = new P{};
    static_cast<Plan&>(*p) = Plan{e, device, k, taps_per_branch, d_taps, d_tw};
    return p;
}

template <typename P>
void close_plan(P* p)
{
    if (!p) return;
    if (hipSetDevice(p->device) == hipSuccess) free_plan_arrays(p->d_taps, p->d_tw);
    delete p;
}

}  // namespace

// the bank's kernel parameters of a run over nframes frames; src, out, first, out_stride and layout are the caller's
inline PfbParams bank_params(const Plan& p, int hop, long nframes)
{
    PfbParams b;
    b.src = nullptr;
    b.out = nullptr;
    b.taps = p.d_taps;
    b.tw = p.d_tw;
    b.nframes = nframes;
    b.first = 0;
    b.out_stride = 0;
    b.taps_per_branch = p.taps_per_branch;
    b.half_hop = hop != 1 << p.log2_m;
    b.layout = 0;
    return b;
}

}  // namespace pfb
}  // namespace rtlws
#endif
