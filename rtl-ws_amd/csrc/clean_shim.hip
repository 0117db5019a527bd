// clean_shim.hip -- extern "C" glue of include/rtlws_clean.h (librtlws_clean.so): argument rules, the plan with its mask
// and its workspace, the three launches of a run, and the host's helper (the one mask of a run's flags).  The engine
// (device, stream) is librtlws_hip.so's; nothing here reads the environment, and nothing of a run is computed on the
// host: without a device there is no plan.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "clean.h"
#include "rtlws_clean.h"
#include "search_plan.h"

struct rtlws_clean_plan : rtlws::search::Plan {
    int nchan, block_rows, zerodm;
    double t_mean, t_sigma;
    long max_blocks;
    void* d_work;              // the cells [max_blocks][nchan], nkept [max_blocks], then the mask [nchan]
};

namespace {

using namespace rtlws::clean;
namespace sp = rtlws::search;
using sp::why_not_nchan;

static_assert(MIN_NCHAN == RTLWS_CLEAN_MIN_NCHAN && MAX_NCHAN == RTLWS_CLEAN_MAX_NCHAN && MIN_BLOCK == RTLWS_CLEAN_MIN_BLOCK &&
                  MAX_BLOCK == RTLWS_CLEAN_MAX_BLOCK && MAX_NROWS == RTLWS_CLEAN_MAX_NROWS && MAX_CELLS == RTLWS_CLEAN_MAX_CELLS &&
                  FLAG_ZERODM == RTLWS_CLEAN_ZERODM && MIN_NCHAN == sp::MIN_NCHAN && MAX_NCHAN == sp::MAX_NCHAN,
              "rtlws_clean.h, clean.h and search_plan.h disagree");

// ---- the rules, each worded once ----
const char* why_not_block(long block_rows) { return block_rows < MIN_BLOCK || block_rows > MAX_BLOCK ? "block_rows must be 32 .. 16384" : nullptr; }
const char* why_not_nrows(long nrows) { return nrows < 0 || nrows > MAX_NROWS ? "nrows must be 0 .. 2^24" : nullptr; }

const char* why_not_shape(int nchan, long block_rows)
{
    if (const char* why = why_not_nchan(nchan)) return why;
    return why_not_block(block_rows);
}

const char* why_not_plan(int nchan, long block_rows, double t_mean, double t_sigma, int flags)
{
    if (const char* why = why_not_shape(nchan, block_rows)) return why;
    if (!(t_mean >= 0.0)) return "t_mean must be >= 0 or +Inf";
    if (!(t_sigma >= 0.0)) return "t_sigma must be >= 0 or +Inf";
    if (flags & ~FLAG_ZERODM) return "unknown flag bits";
    return nullptr;
}

// what a shape decides about nrows (within 0 .. 2^24): the least run, the workspace, the three grids
const char* why_not_run(int nchan, long block_rows, long nrows)
{
    if (nrows == 0) return nullptr;
    if (nrows < block_rows) return "nrows must be 0 or at least block_rows";
    const long nblocks = sp::ceil_div(nrows, block_rows);
    if (nblocks > max_blocks(nchan, (int)block_rows)) return "more blocks than the plan's workspace holds (clean the rows in pieces of whole blocks)";
    const long most = chan_groups(nchan) > apply_groups(nchan, (int)block_rows) ? chan_groups(nchan) : apply_groups(nchan, (int)block_rows);
    return sp::why_not_grid(nblocks, most);
}

// [a, a + na) and [b, b + nb) in bytes share a byte
bool overlap(uintptr_t a, uintptr_t na, uintptr_t b, uintptr_t nb) { return a < b + nb && b < a + na; }

}  // namespace

extern "C" {

const char* rtlws_clean_last_error(void) { return g_err.c_str(); }

int rtlws_clean_supported(int nchan, long block_rows) { return supported("rtlws_clean", why_not_shape(nchan, block_rows)); }

int rtlws_clean_geometry(int nchan, long block_rows, long nrows, int* blocks, int* threads, int* lds, long* nblocks, long* workspace, long* most)
{
    const char* fn = "rtlws_clean_geometry";
    g_err.clear();
    if (const char* why = why_not_shape(nchan, block_rows)) return fail(fn, why, -1);
    if (const char* why = why_not_nrows(nrows)) return fail(fn, why, -1);
    if (const char* why = why_not_run(nchan, block_rows, nrows)) return fail(fn, why, -1);
    const long nb = sp::ceil_div(nrows, block_rows);
    if (blocks) blocks[0] = (int)(nb * chan_groups(nchan)), blocks[1] = (int)nb, blocks[2] = (int)(nb * apply_groups(nchan, (int)block_rows));
    if (threads) threads[0] = STATS_THREADS, threads[1] = flag_threads(nchan), threads[2] = apply_threads(nchan);
    if (lds) lds[0] = STATS_LDS, lds[1] = flag_lds(nchan), lds[2] = apply_lds(nchan);
    if (nblocks) *nblocks = nb;
    if (workspace) *workspace = workspace_bytes(nchan, nb);
    if (most) *most = max_blocks(nchan, (int)block_rows);
    return 0;
}

rtlws_clean_plan* rtlws_clean_open(rtlws_engine* e, int nchan, long block_rows, const uint8_t* mask, double t_mean, double t_sigma, int flags)
{
    const auto fill = [&](rtlws_clean_plan& p) {
        p.nchan = nchan, p.block_rows = (int)block_rows, p.zerodm = (flags & FLAG_ZERODM) ? 1 : 0;
        p.t_mean = t_mean, p.t_sigma = t_sigma, p.max_blocks = max_blocks(nchan, (int)block_rows);
        const size_t work = (size_t)workspace_bytes(nchan, p.max_blocks);
        std::vector<uint8_t> host(nchan, 1);
        if (mask)
            for (int i = 0; i < nchan; ++i) host[i] = mask[i] ? 1 : 0;
        hipError_t err = hipMalloc(&p.d_work, work + (size_t)nchan);
        if (err == hipSuccess) err = hipMemcpy(static_cast<char*>(p.d_work) + work, host.data(), (size_t)nchan, hipMemcpyHostToDevice);
        return err == hipSuccess ? prepare(nchan, p.device) : err;
    };
    return sp::open_plan<rtlws_clean_plan>("rtlws_clean_open", why_not_plan(nchan, block_rows, t_mean, t_sigma, flags), e, fill,
                                           "the mask, the workspace or the kernels", rtlws_clean_close);
}

void rtlws_clean_close(rtlws_clean_plan* p) { sp::close_plan(p, &rtlws_clean_plan::d_work); }

long rtlws_clean_blocks(const rtlws_clean_plan* p, long nrows)
{
    const char* fn = "rtlws_clean_blocks";
    g_err.clear();
    if (const char* why = why_not_nrows(nrows)) return fail(fn, why, -1);
    if (!p) return fail(fn, NULL_PLAN, -1);
    return sp::ceil_div(nrows, p->block_rows);
}

int rtlws_clean_run(rtlws_clean_plan* p, const float* d_rows, long in_stride, long nrows, float* d_out, long out_stride, uint8_t* d_keep,
                    float* d_stats, int32_t* d_nkept, void* stream)
{
    const char* fn = "rtlws_clean_run";
    g_err.clear();
    // what needs no plan
    if (const char* why = why_not_nrows(nrows)) return fail(fn, why, -1);
    if (const char* why = sp::why_not_stride_of_rows(in_stride)) return fail(fn, why, -1);
    if (out_stride < 4 || out_stride % 4) return fail(fn, "out_stride must be >= 4 and a multiple of 4", -1);
    if (!d_rows || !d_out) return fail(fn, "null pointer", -1);
    if (sp::misaligned(d_rows, 16)) return fail(fn, "d_rows must be 16-byte aligned", -1);
    if (sp::misaligned(d_out, 16)) return fail(fn, "d_out must be 16-byte aligned", -1);
    if (sp::misaligned(d_stats, 4)) return fail(fn, "d_stats must be 4-byte aligned", -1);
    if (sp::misaligned(d_nkept, 4)) return fail(fn, "d_nkept must be 4-byte aligned", -1);
    if (!p) return fail(fn, NULL_PLAN, -1);
    // what the plan decides; still before anything is asked of the device
    if (const char* why = sp::why_not_row_stride(in_stride, p->nchan)) return fail(fn, why, -1);
    if (out_stride < p->nchan) return fail(fn, "out_stride must be >= nchan", -1);
    if (nrows == 0) return 0;
    if (nrows < p->block_rows) return fail(fn, "nrows must be 0 or at least block_rows", -1);
    const uintptr_t in0 = reinterpret_cast<uintptr_t>(d_rows), out0 = reinterpret_cast<uintptr_t>(d_out);
    const uintptr_t in_bytes = ((uintptr_t)(nrows - 1) * (uintptr_t)in_stride + (uintptr_t)p->nchan) * sizeof(float);
    const uintptr_t out_bytes = ((uintptr_t)(nrows - 1) * (uintptr_t)out_stride + (uintptr_t)p->nchan) * sizeof(float);
    if (!(in0 == out0 && in_stride == out_stride) && overlap(in0, in_bytes, out0, out_bytes))
        return fail(fn, "d_out overlaps d_rows (in place: d_out == d_rows with equal strides)", -1);
    if (const char* why = why_not_run(p->nchan, p->block_rows, nrows)) return fail(fn, why, -1);

    if (sp::use_device(fn, p)) return -3;
    const hipStream_t st = stream_of(p->engine, stream);
    const long nblocks = sp::ceil_div(nrows, p->block_rows);
    Cell* const cells = static_cast<Cell*>(p->d_work);
    int32_t* const ws_nkept = reinterpret_cast<int32_t*>(cells + p->max_blocks * p->nchan);
    const uint8_t* const mask = reinterpret_cast<const uint8_t*>(ws_nkept + p->max_blocks);

    StatsParams s1{};
    s1.rows = d_rows;
    s1.cells = cells;
    s1.in_stride = in_stride, s1.nrows = nrows;
    s1.nchan = p->nchan, s1.block_rows = p->block_rows, s1.groups = chan_groups(p->nchan);
    hipError_t err = launch_stats(s1, nblocks, st);
    if (err != hipSuccess) return fail_hip(fn, "kernel launch (stage 1)", err);
    FlagParams s2{};
    s2.cells = cells;
    s2.ws_nkept = ws_nkept;
    s2.mask = mask;
    s2.keep = d_keep, s2.stats = d_stats, s2.nkept = d_nkept;
    s2.t_mean = p->t_mean, s2.t_sigma = p->t_sigma;
    s2.nchan = p->nchan;
    err = launch_flags(s2, nblocks, st);
    if (err != hipSuccess) return fail_hip(fn, "kernel launch (stage 2)", err);
    ApplyParams s3{};
    s3.rows = d_rows;
    s3.out = d_out;
    s3.cells = reinterpret_cast<const Flagged*>(cells);
    s3.ws_nkept = ws_nkept;
    s3.in_stride = in_stride, s3.out_stride = out_stride, s3.nrows = nrows;
    s3.nchan = p->nchan, s3.block_rows = p->block_rows, s3.groups = apply_groups(p->nchan, p->block_rows);
    s3.zerodm = p->zerodm;
    err = launch_apply(s3, nblocks, st);
    if (err != hipSuccess) return fail_hip(fn, "kernel launch (stage 3)", err);
    return 0;
}

int rtlws_clean_union_mask(const uint8_t* keep, long nblocks, int nchan, double min_share, uint8_t* mask_out)
{
    const char* fn = "rtlws_clean_union_mask";
    g_err.clear();
    if (!keep || !mask_out) return fail(fn, "null pointer", -1);
    if (nblocks < 1) return fail(fn, "nblocks must be >= 1", -1);
    if (const char* why = why_not_nchan(nchan)) return fail(fn, why, -1);
    if (!(min_share >= 0.0 && min_share <= 1.0)) return fail(fn, "min_share must be 0 .. 1", -1);
    const double least = min_share * (double)nblocks;
    for (int i = 0; i < nchan; ++i) {
        long count = 0;
        for (long b = 0; b < nblocks; ++b) count += keep[b * nchan + i] ? 1 : 0;
        mask_out[i] = (double)count >= least ? 1 : 0;
    }
    return 0;
}

}  // extern "C"
