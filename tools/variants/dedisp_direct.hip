// dedisp_direct.hip -- the comparison form of tools/dedisp_rates.py, not product: include/rtlws_dedisp.h's sum with one
// thread per output that reads every term from device memory, no LDS and no plan.  Lanes run along n, so a wavefront's
// load of one position touches 64 rows.  The additions are the product's, in its order: the outputs agree bit for bit.
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -shared -o dedisp_direct.so dedisp_direct.hip
#include <hip/hip_runtime.h>
#include <stdint.h>

__global__ __launch_bounds__(256) void dedisp_direct_kernel(const float* rows, long in_stride, const int* delays, const uint8_t* mask,
                                                            int nchan, long nout, float* out, long out_stride)
{
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    const int t = blockIdx.y;
    if (n >= nout) return;
    const int* d = delays + (long)t * nchan;
    float acc = 0.0f;
    for (int i = 0; i < nchan; ++i)
        if (!mask || mask[i]) acc = acc + rows[(n + d[i]) * in_stride + i];
    out[t * out_stride + n] = acc;
}

// delays int32 [ntrials][nchan] and mask (or null) in device memory; 0, or the HIP error
extern "C" __attribute__((visibility("default"))) int dedisp_direct(const float* d_rows, long in_stride, const int* d_delays,
                                                                    const uint8_t* d_mask, int nchan, int ntrials, long nout,
                                                                    float* d_out, long out_stride, void* stream)
{
    if (nout <= 0) return 0;
    dedisp_direct_kernel<<<dim3((unsigned)((nout + 255) / 256), (unsigned)ntrials), dim3(256), 0, (hipStream_t)stream>>>(
        d_rows, in_stride, d_delays, d_mask, nchan, nout, d_out, out_stride);
    return (int)hipGetLastError();
}
