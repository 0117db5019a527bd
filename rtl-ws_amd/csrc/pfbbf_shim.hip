// pfbbf_shim.hip -- extern "C" glue of include/rtlws_pfbbf.h (librtlws_pfbbf.so): argument rules, geometry, the plan
// (pfb_plan.h's text, as the other polyphase libraries' plans), the launches.  The engine (device, stream) is
// librtlws_hip.so's; nothing here reads the environment, and nothing of a run is computed on the host: without a
// device there is no plan.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pfb_plan.h"
#include "pfbbf.h"
#include "rtlws_pfb.h"
#include "rtlws_pfbbf.h"

struct rtlws_pfbbf_plan : rtlws::pfb::Plan {
    int ninputs, nbeams;
};

namespace {

using namespace rtlws::pfb;
using namespace rtlws::pfbbf;

static_assert(MIN_LOG2_M == RTLWS_PFB_MIN_LOG2_CHANNELS && MAX_LOG2_M == RTLWS_PFB_MAX_LOG2_CHANNELS &&
                  MAX_TAPS == RTLWS_PFB_MAX_TAPS && LAYOUT_CHANNEL == RTLWS_PFB_CHANNEL_MAJOR && LAYOUT_TIME == RTLWS_PFB_TIME_MAJOR &&
                  MAX_K_AVG == RTLWS_PFBBF_MAX_K_AVG && MIN_INPUTS == RTLWS_PFBBF_MIN_INPUTS && MAX_INPUTS == RTLWS_PFBBF_MAX_INPUTS &&
                  MIN_BEAMS == RTLWS_PFBBF_MIN_BEAMS && MAX_BEAMS == RTLWS_PFBBF_MAX_BEAMS,
              "rtlws_pfbbf.h, rtlws_pfb.h and pfbbf.h disagree");

const char* why_not_counts(int ninputs, int nbeams)
{
    if (ninputs < MIN_INPUTS || ninputs > MAX_INPUTS) return "ninputs must be 1 .. 8";
    if (nbeams < MIN_BEAMS || nbeams > MAX_BEAMS) return "nbeams must be 1 .. 4";
    return nullptr;
}

// why a plan's shape is not served, or nullptr
const char* why_not_plan(int k, int taps, int ninputs, int nbeams)
{
    if (const char* why = why_not_bank(k, taps)) return why;
    return why_not_counts(ninputs, nbeams);
}

// why a run's shape is not served, or nullptr.  k_avg == 0: voltage mode, count frames; else power mode, count spectra
const char* why_not(int k, int taps, int hop, int k_avg, int ninputs, int nbeams, long count)
{
    if (const char* why = why_not_plan(k, taps, ninputs, nbeams)) return why;
    if (const char* why = why_not_hop(k, hop)) return why;
    if (k_avg < 0 || k_avg > MAX_K_AVG) return "k_avg must be 1 .. 65536 (0: voltage mode)";
    return k_avg == 0 ? why_not_count(count, tile_frames(k), false) : why_not_count(count, spectra_per_block(k, k_avg), true);
}

// the extent of one beam's voltages in complex values; nframes > 0
__int128 beam_extent(int layout, long nframes, long out_stride, int log2_m)
{
    const long M = 1L << log2_m;
    return layout == LAYOUT_TIME ? (__int128)(nframes - 1) * out_stride + M : (__int128)(M - 1) * out_stride + nframes;
}

BfParams params_of(const rtlws_pfbbf_plan* p, const void* const* d_iq_cu8, const float* d_weights, int hop, long nframes)
{
    BfParams bp;
    bp.bank = bank_params(*p, hop, nframes);
    for (int a = 0; a < MAX_INPUTS; ++a) bp.src[a] = a < p->ninputs ? d_iq_cu8[a] : nullptr;
    bp.w = reinterpret_cast<const float2*>(d_weights);
    bp.rows = nullptr;
    bp.beam_stride = 0;
    bp.nspectra = 0;
    bp.row_stride = 0;
    bp.ninputs = p->ninputs;
    bp.k_avg = 0;
    bp.shift = 0;
    return bp;
}

}  // namespace

extern "C" {

const char* rtlws_pfbbf_last_error(void) { return g_err.c_str(); }

int rtlws_pfbbf_supported(int log2_channels, int taps_per_branch, int hop, int ninputs, int nbeams)
{
    return supported("rtlws_pfbbf", why_not(log2_channels, taps_per_branch, hop, 0, ninputs, nbeams, 0));
}

long rtlws_pfbbf_samples_needed(int log2_channels, int taps_per_branch, int hop, int k_avg, long count)
{
    g_err.clear();
    if (const char* why = why_not(log2_channels, taps_per_branch, hop, k_avg, MIN_INPUTS, MIN_BEAMS, count))
        return fail("rtlws_pfbbf_samples_needed", why, -1);
    if (count == 0) return 0;
    const long nframes = k_avg == 0 ? count : count * k_avg;
    return (nframes - 1) * hop + (long)taps_per_branch * (1L << log2_channels);
}

int rtlws_pfbbf_grid(int log2_channels, int taps_per_branch, int hop, int k_avg, long count, int* blocks, int* threads,
                     int* lds_bytes, int* per_block)
{
    g_err.clear();
    if (const char* why = why_not(log2_channels, taps_per_branch, hop, k_avg, MIN_INPUTS, MIN_BEAMS, count))
        return fail("rtlws_pfbbf_grid", why, -1);
    const int g = k_avg == 0 ? tile_frames(log2_channels) : spectra_per_block(log2_channels, k_avg);
    if (blocks) *blocks = (int)((count + g - 1) / g);
    if (threads) *threads = THREADS;
    if (lds_bytes) *lds_bytes = rtlws::pfbbf::lds_bytes(log2_channels);
    if (per_block) *per_block = g;
    return 0;
}

rtlws_pfbbf_plan* rtlws_pfbbf_open(rtlws_engine* e, int log2_channels, int taps_per_branch, const int16_t* taps, int ninputs,
                                   int nbeams)
{
    g_err.clear();
    rtlws_pfbbf_plan* p = open_plan<rtlws_pfbbf_plan>(
        "rtlws_pfbbf_open", why_not_plan(log2_channels, taps_per_branch, ninputs, nbeams), e, log2_channels, taps_per_branch, taps,
        [nbeams](int k) { return prepare_pfbbf(k, nbeams); }, "the taps, the table or the kernels");
    if (p) {
        p->ninputs = ninputs;
        p->nbeams = nbeams;
    }
    return p;
}

void rtlws_pfbbf_close(rtlws_pfbbf_plan* p) { close_plan(p); }

int rtlws_pfbbf_run(rtlws_pfbbf_plan* p, const void* const* d_iq_cu8, int ninputs, const float* d_weights, int nbeams,
                    long nframes, int hop, long first_frame_index, int layout, void* d_out_cf32, long out_stride,
                    long beam_stride, void* stream)
{
    const char* fn = "rtlws_pfbbf_run";
    g_err.clear();
    // what needs no plan: the hop is a power of two 8 .. 1024, a frame holds at least 16 values
    if (const char* why = why_not_any_hop(hop)) return fail(fn, why, -1);
    if (const char* why = why_not_counts(ninputs, nbeams)) return fail(fn, why, -1);
    if (const char* why = why_not_count(nframes, tile_frames(MIN_LOG2_M), false)) return fail(fn, why, -1);
    if (first_frame_index < 0) return fail(fn, "first_frame_index must be >= 0", -1);
    if (layout != LAYOUT_CHANNEL && layout != LAYOUT_TIME) return fail(fn, "unknown layout", -1);
    if (out_stride < (layout == LAYOUT_CHANNEL ? nframes : 1L << MIN_LOG2_M)) return fail(fn, "out_stride too small for the layout", -1);
    if (nframes > 0 && beam_stride < beam_extent(layout, nframes, out_stride, MIN_LOG2_M))
        return fail(fn, "beam_stride smaller than one beam's output", -1);
    if (nframes > 0 && (!d_iq_cu8 || !d_weights || !d_out_cf32)) return fail(fn, "null pointer", -1);
    if (reinterpret_cast<uintptr_t>(d_weights) & 15u) return fail(fn, "d_weights must be 16-byte aligned", -1);
    if (reinterpret_cast<uintptr_t>(d_out_cf32) & 7u) return fail(fn, "d_out_cf32 must be 8-byte aligned", -1);
    if (!p) return fail(fn, "null plan (no usable HIP device: there is no CPU path)", -1);
    // what the plan decides; still before anything is asked of the device
    if (const char* why = why_not(p->log2_m, p->taps_per_branch, hop, 0, ninputs, nbeams, nframes)) return fail(fn, why, -1);
    if (ninputs != p->ninputs) return fail(fn, "ninputs is not the plan's", -1);
    if (nbeams != p->nbeams) return fail(fn, "nbeams is not the plan's", -1);
    if (layout == LAYOUT_TIME && out_stride < 1L << p->log2_m) return fail(fn, "out_stride too small for the layout", -1);
    if (nframes == 0) return 0;
    if (beam_stride < beam_extent(layout, nframes, out_stride, p->log2_m)) return fail(fn, "beam_stride smaller than one beam's output", -1);
    if (const char* why = why_not_captures(d_iq_cu8, p->ninputs)) return fail(fn, why, -1);

    hipError_t err = hipSetDevice(p->device);
    if (err != hipSuccess) return fail_hip(fn, "hipSetDevice", err);
    BfParams bp = params_of(p, d_iq_cu8, d_weights, hop, nframes);
    bp.bank.out = static_cast<float2*>(d_out_cf32);
    bp.bank.first = first_frame_index;
    bp.bank.out_stride = out_stride;
    bp.bank.layout = layout;
    bp.beam_stride = beam_stride;
    err = launch_pfbbf(p->log2_m, p->nbeams, bp, stream_of(p->engine, stream));
    if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
    return 0;
}

int rtlws_pfbbf_power(rtlws_pfbbf_plan* p, const void* const* d_iq_cu8, int ninputs, const float* d_weights, int nbeams,
                      long nspectra, int hop, int k_avg, int shifted, float* d_out, long row_stride, void* stream)
{
    const char* fn = "rtlws_pfbbf_power";
    g_err.clear();
    // what needs no plan: the hop is a power of two 8 .. 1024, a row holds at least 16 values, a workgroup at most
    // 256 / k_avg spectra
    if (const char* why = why_not_any_hop(hop)) return fail(fn, why, -1);
    if (const char* why = why_not_k_avg(k_avg)) return fail(fn, why, -1);
    if (shifted != 0 && shifted != 1) return fail(fn, "shifted must be 0 or 1", -1);
    if (const char* why = why_not_counts(ninputs, nbeams)) return fail(fn, why, -1);
    if (const char* why = why_not_count(nspectra, spectra_per_block(MIN_LOG2_M, k_avg), true)) return fail(fn, why, -1);
    if (row_stride < 1L << MIN_LOG2_M) return fail(fn, "row_stride must be >= M", -1);
    if (row_stride % 4) return fail(fn, "row_stride must be a multiple of 4", -1);
    if (nspectra > 0 && (!d_iq_cu8 || !d_weights || !d_out)) return fail(fn, "null pointer", -1);
    if (reinterpret_cast<uintptr_t>(d_weights) & 15u) return fail(fn, "d_weights must be 16-byte aligned", -1);
    if (reinterpret_cast<uintptr_t>(d_out) & 15u) return fail(fn, "d_out must be 16-byte aligned", -1);
    if (!p) return fail(fn, "null plan (no usable HIP device: there is no CPU path)", -1);
    // what the plan decides; still before anything is asked of the device
    if (const char* why = why_not(p->log2_m, p->taps_per_branch, hop, k_avg, ninputs, nbeams, nspectra)) return fail(fn, why, -1);
    if (ninputs != p->ninputs) return fail(fn, "ninputs is not the plan's", -1);
    if (nbeams != p->nbeams) return fail(fn, "nbeams is not the plan's", -1);
    if (row_stride < 1L << p->log2_m) return fail(fn, "row_stride must be >= M", -1);
    if (nspectra == 0) return 0;
    if (const char* why = why_not_captures(d_iq_cu8, p->ninputs)) return fail(fn, why, -1);

    hipError_t err = hipSetDevice(p->device);
    if (err != hipSuccess) return fail_hip(fn, "hipSetDevice", err);
    BfParams bp = params_of(p, d_iq_cu8, d_weights, hop, nspectra * k_avg);
    bp.rows = d_out;
    bp.nspectra = nspectra;
    bp.row_stride = row_stride;
    bp.k_avg = k_avg;
    bp.shift = shifted ? 1 << (p->log2_m - 1) : 0;
    err = launch_pfbbf_power(p->log2_m, p->nbeams, bp, stream_of(p->engine, stream));
    if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
    return 0;
}

}  // extern "C"
