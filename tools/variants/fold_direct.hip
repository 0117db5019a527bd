// fold_direct.hip -- the comparison form of tools/fold_rates.py, not product: include/rtlws_fold.h's profiles with one
// thread per (trial, period, sub-integration) that keeps its profile in device memory: it clears its nbins words, then
// walks the sub-integration's samples in ascending n and adds each to the word of its bin (load, add, store), no LDS and
// no plan.  Threads run along periods, so a wavefront's threads read the same sample.  The additions are the product's,
// in its order: the profiles agree bit for bit.  No hits.
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -shared -o fold_direct.so fold_direct.hip
#include <hip/hip_runtime.h>
#include <stdint.h>

__global__ __launch_bounds__(64) void fold_direct_kernel(const float* in, long in_stride, long nsamp, const uint64_t* steps, const uint64_t* phases,
                                                         int nperiods, int nbins, long sub, long nsub, float* prof)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    const long s = blockIdx.y, t = blockIdx.z;
    if (p >= nperiods) return;
    const long n0 = s * sub, n1 = n0 + sub < nsamp ? n0 + sub : nsamp;
    const uint64_t step = steps[p];
    uint64_t phase = phases[p] + (uint64_t)n0 * step;
    float* mine = prof + ((t * nperiods + p) * nsub + s) * nbins;
    const float* x = in + t * in_stride;
    for (int b = 0; b < nbins; ++b) mine[b] = 0.0f;
    for (long n = n0; n < n1; ++n) {
        const unsigned b = __umulhi((unsigned)(phase >> 32), (unsigned)nbins);
        mine[b] = mine[b] + x[n];
        phase += step;
    }
}

// steps and phases uint64 [nperiods] in device memory; 0, or the HIP error
extern "C" __attribute__((visibility("default"))) int fold_direct(const float* d_in, long in_stride, int ntrials, long nsamp, const uint64_t* d_steps,
                                                                  const uint64_t* d_phases, int nperiods, int nbins, long sub, float* d_prof, void* stream)
{
    if (nsamp <= 0) return 0;
    const long nsub = (nsamp + sub - 1) / sub;
    fold_direct_kernel<<<dim3((unsigned)((nperiods + 63) / 64), (unsigned)nsub, (unsigned)ntrials), dim3(64), 0, (hipStream_t)stream>>>(
        d_in, in_stride, nsamp, d_steps, d_phases, nperiods, nbins, sub, nsub, d_prof);
    return (int)hipGetLastError();
}
