// fold.hip -- the kernels of include/rtlws_fold.h (librtlws_fold.so): csrc/fold_kernel.h's kernel with the
// epilogue of conflict-free row reads, one instantiation per block shape, and their launch table.
#include <hip/hip_runtime.h>

#include "fold_kernel.h"
#include "rtlws_internal.h"

namespace rtlws {
namespace fold {

// The launch table: f is handed the instantiation of the bin count's block shape
template <typename F>
static hipError_t with_kernel(int nbins, F&& f)
{
    switch (waves_per_block(nbins)) {
    case 4: return f(&fold_kernel<4, RowReads>);
    case 2: return f(&fold_kernel<2, RowReads>);
    default: return f(&fold_kernel<1, RowReads>);
    }
}

hipError_t launch_fold(const Params& p, int ntrials, hipStream_t st)
{
    const long blocks = (long)ntrials * p.nsub * p.groups;
    const int wpb = waves_per_block(p.nbins);
    return with_kernel(p.nbins, [&](auto kernel) {
        return launch(kernel, dim3((unsigned)blocks), dim3(wpb * LANES), (size_t)lds_bytes(p.nbins), st, p);
    });
}

// load_kernel (rtlws_internal.h) for the kernel of a bin count
hipError_t prepare_fold(int nbins)
{
    return with_kernel(nbins, [](auto kernel) { return load_kernel(kernel); });
}

}  // namespace fold
}  // namespace rtlws
