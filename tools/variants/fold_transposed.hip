// fold_transposed.hip -- the other epilogue of tools/fold_rates.py, not product: csrc/fold_kernel.h's kernel, the same hot
// loop and the same bits, with the histogram read transposed: for each of the wavefront's periods in turn the 64 lanes
// read 64 consecutive bins of that period's column (one bank: the reads take the conflicts) and store them as 256
// consecutive bytes.  The product reads rows without conflicts and stores a lane a period (RowReads).
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -shared -I rtl-ws_amd/csrc -I include -o fold_transposed.so fold_transposed.hip
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fold_kernel.h"

namespace {

using namespace rtlws::fold;

struct Transposed {
    template <typename T>
    static __device__ __forceinline__ void store(const float* hist, int lane, int valid, T* rows, long pitch, int nbins)
    {
        const T* const h = reinterpret_cast<const T*>(hist);
        __builtin_amdgcn_wave_barrier();
        for (int q = 0; q < valid; ++q)
            for (int b = lane; b < nbins; b += LANES) rows[q * pitch + b] = h[b * LANES + q];
        __builtin_amdgcn_wave_barrier();
    }
};

}  // namespace

// steps and phases uint64 [nperiods] in device memory, d_hits may be null; 0, or the HIP error
extern "C" __attribute__((visibility("default"))) int fold_transposed(const float* d_in, long in_stride, int ntrials, long nsamp, const uint64_t* d_steps,
                                                                      const uint64_t* d_phases, int nperiods, int nbins, long sub, float* d_prof,
                                                                      uint32_t* d_hits, void* stream)
{
    if (nsamp <= 0) return 0;
    const int wpb = waves_per_block(nbins);
    Params p;
    p.in = d_in;
    p.prof = d_prof;
    p.hits = d_hits;
    p.steps = d_steps;
    p.phases = d_phases;
    p.in_stride = in_stride;
    p.nsamp = nsamp;
    p.sub = sub;
    p.nsub = (nsamp + sub - 1) / sub;
    p.nperiods = nperiods;
    p.nbins = nbins;
    p.groups = (nperiods + LANES * wpb - 1) / (LANES * wpb);
    const dim3 grid((unsigned)(ntrials * p.nsub * p.groups)), block(wpb * LANES);
    const size_t lds = (size_t)lds_bytes(nbins);
    if (wpb == 4) fold_kernel<4, Transposed><<<grid, block, lds, (hipStream_t)stream>>>(p);
    else if (wpb == 2) fold_kernel<2, Transposed><<<grid, block, lds, (hipStream_t)stream>>>(p);
    else fold_kernel<1, Transposed><<<grid, block, lds, (hipStream_t)stream>>>(p);
    return (int)hipGetLastError();
}
