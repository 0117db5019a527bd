// accel.hip -- the kernels of include/rtlws_accel.h (librtlws_accel.so): the long-frame search of
// rtlws_periodlong.h over series read through a quadratic index map, one virtual trial per (trial, acceleration), with
// no resampled copy in memory; and the kernel that writes such a copy for the few candidates that go on to folding.
//
//   mapped_mean    periodlong_front.h's mean, its quads four indexed 4-byte loads
//   mapped_cols    periodlong_front.h's columns, a point's two samples two indexed 4-byte loads
//   (rows, untangle, whiten, peaks: periodlong.hip's kernels, linked as they are)
//   resample       R[n] = D[f(n)], a thread four consecutive n and one 16-byte store
//
// A virtual trial v = trial0 + blockIdx.y lies in workspace slot blockIdx.y; its source trial v / naccel and its
// coefficient coefs[v mod naccel] are uniform over the workgroup: one scalar division and one scalar load.  f(n) = n +
// shift(c, n, nsamp - 1) stays in 0 .. nsamp - 1 for every |c| <= 2^40 (DESIGN.md 4.24 proves it): no clamp.
#include <hip/hip_runtime.h>

#include "accel.h"
#include "periodlong_front.h"
#include "rtlws_internal.h"

namespace rtlws {
namespace accel {

namespace {

namespace front = periodlong::front;

// a trial read through the map: every sample an indexed load of its own
struct Mapped {
    const float* x;
    int64_t c;
    int last;              // nsamp - 1
    __device__ __forceinline__ float one(int n) const { return x[n + shift(c, n, last)]; }
    __device__ __forceinline__ float2 pair(int n) const { return make_float2(one(n), one(n + 1)); }
    __device__ __forceinline__ float4 quad(int n) const { return make_float4(one(n), one(n + 1), one(n + 2), one(n + 3)); }
};

__device__ __forceinline__ Mapped series_of(const Params& q)
{
    const int v = q.s.trial0 + (int)blockIdx.y, t = v / q.naccel, a = v - t * q.naccel;
    return Mapped{q.s.in + (long)t * q.s.in_stride, q.coefs[a], q.s.nsamp - 1};
}

}  // namespace

__global__ __launch_bounds__(periodlong::MEAN_THREADS) void mapped_mean_kernel(const Params q) { front::mean(q.s, series_of(q)); }

__global__ __launch_bounds__(periodlong::COLS_THREADS) void mapped_cols16_kernel(const Params q) { front::cols16(q.s, series_of(q)); }

__global__ __launch_bounds__(periodlong::COLS_THREADS) void mapped_cols256_kernel(const Params q) { front::cols256(q.s, series_of(q)); }

// ---- resample: workgroup (i, row) writes elements 1024 i .. 1024 i + 1023 below nsamp of rows row, row + gridDim.y, .. ----
__global__ __launch_bounds__(RESAMPLE_THREADS) void resample_kernel(const ResampleParams p)
{
    const int nsamp = p.nsamp, n0 = RESAMPLE_QUAD * ((int)blockIdx.x * RESAMPLE_THREADS + (int)threadIdx.x);
    if (n0 >= nsamp) return;
    for (int row = blockIdx.y; row < p.rows; row += (int)gridDim.y) {
        const int t = row / p.a_count, a = p.a_first + (row - t * p.a_count);
        const Mapped x{p.in + (long)t * p.in_stride, p.coefs[a], nsamp - 1};
        float* const out = p.out + (long)row * p.out_stride + n0;
        if (n0 + RESAMPLE_QUAD <= nsamp) {
            *reinterpret_cast<float4*>(out) = x.quad(n0);
        } else {                                             // the last, partial quad: nothing at or behind nsamp is written
            out[0] = x.one(n0);
            if (n0 + 1 < nsamp) out[1] = x.one(n0 + 1);
            if (n0 + 2 < nsamp) out[2] = x.one(n0 + 2);
        }
    }
}

hipError_t launch_group(const Params& q, int group, hipStream_t st)
{
    using namespace periodlong;
    const int n = q.s.log2n, l1 = log2m1_of(n);
    hipError_t e = launch(&mapped_mean_kernel, dim3((unsigned)stage_blocks(STAGE_MEAN, n), (unsigned)group), dim3((unsigned)stage_threads(STAGE_MEAN, n)), 0, st, q);
    if (e != hipSuccess) return e;
    e = launch(l1 == 4 ? &mapped_cols16_kernel : &mapped_cols256_kernel, dim3((unsigned)stage_blocks(STAGE_COLS, n), (unsigned)group),
               dim3((unsigned)stage_threads(STAGE_COLS, n)), (size_t)cols_lds(l1), st, q);
    if (e != hipSuccess) return e;
    return launch_tail(q.s, group, st);
}

hipError_t launch_resample(const ResampleParams& p, hipStream_t st)
{
    return launch(&resample_kernel, dim3((unsigned)resample_blocks_x(p.nsamp), (unsigned)resample_blocks_y(p.rows)), dim3(RESAMPLE_THREADS), 0, st, p);
}

hipError_t prepare(int log2n, int device)
{
    hipError_t e = load_kernel(&mapped_mean_kernel);
    if (e == hipSuccess) e = load_kernel(&mapped_cols16_kernel);
    if (e == hipSuccess) e = load_kernel(&mapped_cols256_kernel);
    if (e == hipSuccess) e = load_kernel(&resample_kernel);
    return e == hipSuccess ? periodlong::prepare(log2n, device) : e;
}

}  // namespace accel
}  // namespace rtlws
