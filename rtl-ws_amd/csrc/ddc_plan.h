// ddc_plan.h -- the host side the tuned-channel family shares (ddc_shim.hip, fmbank_shim.hip, ddcfir_shim.hip;
// DESIGN.md 4.13b): the plan every opaque plan type derives from, its open and close, and the family's argument rules,
// each stated once and returning its text or nullptr.  A shim composes the rules in the order its header documents.
#ifndef RTLWS_DDC_PLAN_H
#define RTLWS_DDC_PLAN_H

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <vector>

#include "ddc_bank.h"
#include "ddc_table.h"
#include "shim_common.h"

namespace rtlws {
namespace ddc {

// The phasor table on the engine's device
struct Plan {
    rtlws_engine* engine;
    int device;
    uint32_t* d_table;
};

// workgroups of a bank that stores dec_len decimated samples a channel
inline long tiles_of(long dec_len) { return (dec_len + TILE_DEC - 1) / TILE_DEC; }

// ---- the family's rules ----
inline const char* why_not_cic_r(int cic_r) { return cic_r < 1 || cic_r > MAX_R ? "cic_r must be 1 .. 128" : nullptr; }

inline const char* why_not_channels(int nchannels) { return nchannels < 1 || nchannels > MAX_CH ? "nchannels must be 1 .. 32" : nullptr; }

inline const char* why_not_dec_len(long dec_len)
{
    if (dec_len < 0) return "dec_len must be >= 0";
    if (dec_len > (long)INT_MAX * TILE_DEC) return "more decimated samples than one grid holds";
    return nullptr;
}

inline const char* why_not_first(long first_dec_index) { return first_dec_index < 0 ? "first_dec_index must be >= 0" : nullptr; }

inline const char* why_not_out_stride(long out_stride, long dec_len) { return out_stride < dec_len ? "out_stride must be >= dec_len" : nullptr; }

// The caller's words into the kernel parameters, zero behind nchannels (nothing there is read)
inline const char* fill_words(int16_t (&words)[MAX_CH], const int* tuning_words, int nchannels)
{
    if (!tuning_words) return "null tuning_words";
    for (int c = 0; c < MAX_CH; ++c) {
        const int k = c < nchannels ? tuning_words[c] : 0;
        if (k < -P / 2 || k >= P / 2) return "a tuning word lies outside [-32768, 32768)";
        words[c] = (int16_t)k;
    }
    return nullptr;
}

// the capture and what the run writes, both needed where there is work; then the capture's alignment
inline const char* why_not_capture(bool work, const void* d_iq_cu8, const void* d_out)
{
    if (work && (!d_iq_cu8 || !d_out)) return "null pointer";
    return reinterpret_cast<uintptr_t>(d_iq_cu8) & 15u ? "d_iq_cu8 must be 16-byte aligned" : nullptr;
}

inline const char* why_not_cs32(const void* d_out_cs32)
{
    return reinterpret_cast<uintptr_t>(d_out_cs32) & 7u ? "d_out_cs32 must be 8-byte aligned" : nullptr;
}

// the last of a run's refusals
inline const char* why_not_plan(const Plan* p) { return p ? nullptr : "null plan (no usable HIP device: there is no CPU path)"; }

namespace {

template <typename PlanT>
void close_plan(PlanT* p)
{
    if (!p) return;
    if (hipSetDevice(p->device) == hipSuccess) (void)hipFree(p->d_table);
    delete p;
}

// rtlws_*_open of plan type PlanT (derived from Plan): `why` is the verdict of the library's own rules.  With the
// table on the engine's device, prepare(plan) uploads what the library adds to the plan and loads its kernels there;
// where it fails it leaves nothing of its own allocated.  `what` names what can fail.  Null with the text recorded,
// nothing left allocated
template <typename PlanT, typename Prepare>
PlanT* open_plan(const char* fn, const char* why, rtlws_engine* e, Prepare&& prepare, const char* what = "the table or the kernels")
{
    const int device = open_device(fn, why, e);
    if (device < 0) return nullptr;
    std::vector<int16_t> host(2 * (size_t)P);
    build_table(host.data(), P);
    PlanT* p = new PlanT{};
    static_cast<Plan&>(*p) = Plan{e, device, nullptr};
    hipError_t err = hipMalloc(reinterpret_cast<void**>(&p->d_table), host.size() * sizeof(int16_t));
    if (err == hipSuccess) err = hipMemcpy(p->d_table, host.data(), host.size() * sizeof(int16_t), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = prepare(*p);
    if (err != hipSuccess) {
        fail_hip(fn, what, err);
        close_plan(p);
        return nullptr;
    }
    return p;
}

}  // namespace

}  // namespace ddc
}  // namespace rtlws
#endif
