// pulse_direct.hip -- the comparison form of tools/pulse_rates.py, not product: include/rtlws_pulse.h's boxcar sums with
// one thread per (trial, width, n) that reads its w samples from device memory and adds them in the header's balanced
// order with a carry stack (a binary counter of partial sums), no LDS and no plan; the sums go to device memory, and a
// second kernel takes every segment's peak from there.  The additions are the product's, in its order, and the peak
// rule is the header's: peaks and places agree bit for bit.  No moments.
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -shared -o pulse_direct.so pulse_direct.hip
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int LEVELS = 11;

__global__ __launch_bounds__(256) void pulse_direct_sums(const float* in, long in_stride, const int* widths, int nwidths, long nout, float* sums)
{
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y, t = blockIdx.z;
    if (n >= nout) return;
    const int w = widths[k];
    const float* x = in + t * in_stride + n;
    float part[LEVELS];                                       // part[l]: a finished sum of 2^l samples waiting for its partner
    for (int j = 0; j < w; ++j) {
        float v = x[j];
        bool carry = true;
#pragma unroll
        for (int l = 0; l < LEVELS; ++l)
            if (carry) {
                if (j >> l & 1) v = part[l] + v;              // the earlier half first
                else {
                    part[l] = v;
                    carry = false;
                }
            }
    }
    float b = 0.0f;
    bool have = false;
#pragma unroll
    for (int l = LEVELS - 1; l >= 0; --l)
        if (w >> l & 1) {
            b = have ? b + part[l] : part[l];
            have = true;
        }
    sums[((long)t * nwidths + k) * nout + n] = b;
}

__global__ __launch_bounds__(256) void pulse_direct_peaks(const float* sums, int nwidths, long nout, long seg, long nseg, float* peak, int* at)
{
    __shared__ float best_of[256];
    __shared__ int at_of[256];
    const long s = blockIdx.x;
    const int k = blockIdx.y, t = blockIdx.z, tid = threadIdx.x;
    const float* b = sums + ((long)t * nwidths + k) * nout;
    const long end = (s + 1) * seg < nout ? (s + 1) * seg : nout;
    float best = -__builtin_inff();
    int where = -1;
    for (long n = s * seg + tid; n < end; n += 256)
        if (b[n] > best) {
            best = b[n];
            where = (int)n;
        }
    best_of[tid] = best;
    at_of[tid] = where;
    for (int h = 128; h >= 1; h >>= 1) {
        __syncthreads();
        if (tid < h && (best_of[tid + h] > best_of[tid] || (best_of[tid + h] == best_of[tid] && at_of[tid + h] < at_of[tid]))) {
            best_of[tid] = best_of[tid + h];
            at_of[tid] = at_of[tid + h];
        }
    }
    if (tid == 0) {
        peak[((long)t * nwidths + k) * nseg + s] = best_of[0];
        at[((long)t * nwidths + k) * nseg + s] = at_of[0];
    }
}

// widths int32 [nwidths] and the workspace d_sums (ntrials * nwidths * nout f32) in device memory; 0, or the HIP error
extern "C" __attribute__((visibility("default"))) int pulse_direct(const float* d_in, long in_stride, int ntrials, long nout, const int* d_widths,
                                                                   int nwidths, long seg, float* d_sums, float* d_peak, int* d_at, void* stream)
{
    if (nout <= 0) return 0;
    const long nseg = (nout + seg - 1) / seg;
    pulse_direct_sums<<<dim3((unsigned)((nout + 255) / 256), (unsigned)nwidths, (unsigned)ntrials), dim3(256), 0, (hipStream_t)stream>>>(
        d_in, in_stride, d_widths, nwidths, nout, d_sums);
    pulse_direct_peaks<<<dim3((unsigned)nseg, (unsigned)nwidths, (unsigned)ntrials), dim3(256), 0, (hipStream_t)stream>>>(
        d_sums, nwidths, nout, seg, nseg, d_peak, d_at);
    return (int)hipGetLastError();
}
