// fm_shim.hip -- extern "C" glue of include/rtlws_fm.h (librtlws_fm.so): argument rules, geometry, launches.
// The engine (device, stream) is librtlws_hip.so's; nothing here reads the environment, and nothing computes on
// the host: without a device every launching entry point fails.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "fm_chain.h"
#include "rtlws_fm.h"
#include "shim_common.h"

namespace {

long tiles_of(int block_len, long nblocks)
{
    const long total_audio = nblocks * (long)(block_len / 4);
    return (total_audio + rtlws::fm::TILE - 1) / rtlws::fm::TILE;
}

// why a shape is not served, or nullptr (cic_r = 0: the cmplx_s32 form)
const char* why_not(int block_len, long nblocks, int cic_r, bool cu8)
{
    if (block_len < RTLWS_FM_MIN_BLOCK_LEN) return "block_len must be >= 20 (the reference's half-band keeps ten samples of a block)";
    if (nblocks < 0) return "nblocks must be >= 0";
    if (cu8 ? (cic_r < 1 || cic_r > 128) : cic_r != 0) return "cic_r must be 1 .. 128";
    if (nblocks > LONG_MAX / ((long)block_len * 2 * (cu8 ? cic_r : 4))) return "nblocks * block_len too large";
    if (tiles_of(block_len, nblocks) > (long)INT_MAX - 1) return "more audio than one grid holds";
    return nullptr;
}

int run(const char* fn, rtlws_engine* e, int cic_r, bool cu8, const void* d_src, int block_len, long nblocks,
        const float* d_state_in, float* d_state_out, int run_stage2, float* d_audio, void* d_dec, void* stream)
{
    using namespace rtlws::fm;
    g_err.clear();
    if (const char* why = why_not(block_len, nblocks, cic_r, cu8)) return fail(fn, why, -1);
    if (!d_state_in || !d_state_out) return fail(fn, "null state pointer", -1);
    if (d_state_in == d_state_out) return fail(fn, "d_state_in and d_state_out must differ", -1);
    if (nblocks > 0 && (!d_src || (run_stage2 && !d_audio))) return fail(fn, "null pointer", -1);
    if (reinterpret_cast<uintptr_t>(d_src) & (cu8 ? 15u : 7u))
        return fail(fn, cu8 ? "d_iq_cu8 must be 16-byte aligned" : "d_iq_cs32 must be 8-byte aligned", -1);
    if (reinterpret_cast<uintptr_t>(d_dec) & 7u) return fail(fn, "d_dec must be 8-byte aligned", -1);
    if ((reinterpret_cast<uintptr_t>(d_state_in) | reinterpret_cast<uintptr_t>(d_state_out) |
         reinterpret_cast<uintptr_t>(d_audio)) & 3u)
        return fail(fn, "d_state_in, d_state_out and d_audio must be 4-byte aligned", -1);
    if (!e) return fail(fn, "null engine (no usable HIP device: there is no CPU path)", -1);

    hipError_t err = hipSetDevice(rtlws_engine_device(e));
    if (err != hipSuccess) return fail_hip(fn, "hipSetDevice", err);
    hipStream_t st = stream_of(e, stream);
    if (nblocks == 0) {
        err = launch_state_copy(d_state_in, d_state_out, st);
    } else {
        ChainParams p;
        p.src = d_src;
        p.dec = d_dec;
        p.state_in = d_state_in;
        p.state_out = d_state_out;
        p.audio = d_audio;
        p.nblocks = nblocks;
        p.ntiles = tiles_of(block_len, nblocks);
        p.block_len = block_len;
        p.cic_r = cic_r;
        err = launch_chain(p, run_stage2 != 0, st);
    }
    if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
    return 0;
}

}  // namespace

extern "C" {

const char* rtlws_fm_last_error(void) { return g_err.c_str(); }

int rtlws_fm_supported(int block_len, long nblocks, int cic_r)
{
    return supported("rtlws_fm", why_not(block_len, nblocks, cic_r, cic_r != 0));
}

int rtlws_fm_grid(int block_len, long nblocks, int cic_r, int* blocks, int* threads, int* lds_bytes, int* tile_audio)
{
    using namespace rtlws::fm;
    g_err.clear();
    if (const char* why = why_not(block_len, nblocks, cic_r, cic_r != 0)) return fail("rtlws_fm_grid", why, -1);
    const bool copy = nblocks == 0;                      // the state copy: one small workgroup, no LDS
    if (blocks) *blocks = copy ? 1 : (int)(tiles_of(block_len, nblocks) + 1);
    if (threads) *threads = copy ? 64 : THREADS;
    if (lds_bytes) *lds_bytes = copy ? 0 : LDS_FLOATS * (int)sizeof(float);
    if (tile_audio) *tile_audio = TILE;
    return 0;
}

int rtlws_fm_prepare(rtlws_engine* e)
{
    g_err.clear();
    if (!e) return fail("rtlws_fm_prepare", "null engine (no usable HIP device: there is no CPU path)", -1);
    hipError_t err = hipSetDevice(rtlws_engine_device(e));
    if (err == hipSuccess) err = rtlws::fm::prepare_chain();
    if (err != hipSuccess) return fail_hip("rtlws_fm_prepare", "loading the kernels", err);
    return 0;
}

int rtlws_fm_audio_blocks(rtlws_engine* e, const void* d_iq_cs32, int block_len, long nblocks,
                          const float* d_state_in, float* d_state_out, int run_stage2, float* d_audio, void* stream)
{
    return run("rtlws_fm_audio_blocks", e, 0, false, d_iq_cs32, block_len, nblocks, d_state_in, d_state_out,
               run_stage2, d_audio, nullptr, stream);
}

int rtlws_fm_audio_blocks_cu8(rtlws_engine* e, int cic_r, const void* d_iq_cu8, int block_len, long nblocks,
                              const float* d_state_in, float* d_state_out, int run_stage2, float* d_audio,
                              void* d_dec_or_null, void* stream)
{
    return run("rtlws_fm_audio_blocks_cu8", e, cic_r, true, d_iq_cu8, block_len, nblocks, d_state_in, d_state_out,
               run_stage2, d_audio, d_dec_or_null, stream);
}

}  // extern "C"
