// subdedisp.h -- shared between subdedisp.hip (the kernels) and subdedisp_shim.hip (rtlws_subdedisp.h's host glue): the
// two stages' forms and the tables they upload.  The tile, its constants and Layout are dedisp.h's.
#ifndef RTLWS_CSRC_SUBDEDISP_H
#define RTLWS_CSRC_SUBDEDISP_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dedisp.h"

namespace rtlws {
namespace subdedisp {

using dedisp::BIG_WORDS;
using dedisp::Layout;
using dedisp::MAX_CHUNK;
using dedisp::MAX_TRIALS_PER_BLOCK;
using dedisp::SMALL_WORDS;
using dedisp::THREADS;
using dedisp::TILE_OUT;

constexpr int MIN_NCHAN = dedisp::MIN_NCHAN, MAX_NCHAN = dedisp::MAX_NCHAN, MAX_TRIALS = dedisp::MAX_TRIALS, MAX_DELAY = dedisp::MAX_DELAY;
constexpr int MIN_PER_SUB = 4, MAX_NOMINALS = 4096;

// Stage 1 is dedisp.h's tile over d1 as a table of nnominal trials: its Layout and Params (out: the workspace,
// out_stride: mid_stride, nout: nmid, ntrials: nnominal, rows_needed: nmid + max_d1), with the sums stored and begun
// again at every subband's last position.
//
// Stage 2: a workgroup owns TILE_OUT consecutive outputs of up to `trials` consecutive trials of one nominal (a group)
// and walks the subbands in chunks of MAX_CHUNK.  A unit is one subband: its column is the part of its series between
// the group's least and largest d2, staged by consecutive lanes along time, no transposition; Layout's lone = 1,
// chunk = MAX_CHUNK, stride = TILE_OUT + the widest spread of d2 inside a subband and a group (any stride: the lanes of a
// store and of a read are along a column), and behind the chunk's columns the TILE_OUT zeros a subband reads that keeps
// no position: MAX_CHUNK * stride + TILE_OUT <= the LDS.
struct Params2 {
    const float* mid;      // P: series (nominal * nsub + subband) at mid + .. * mid_stride, nmid values
    float* out;
    const int4* groups;    // [group] {first trial, trials (1 .. the form's), nominal, 0}
    const int2* units;     // [group][subband] {base, span}: the window is values n0 + base .. n0 + base + TILE_OUT - 1 + span; base < 0: nothing kept
    const int* rel;        // [group][subband][trial of the group]: (subband in its chunk) * stride + d2 - base; MAX_CHUNK * stride (the zeros) where nothing is kept
    long mid_stride, nmid, nout, out_stride;
    int nsub, ngroups, stride;
};

// ceil(nmid / TILE_OUT) * ceil(nnominal / l.trials) workgroups; per: positions of a subband
hipError_t launch_stage1(const Layout& l, const dedisp::Params& p, int per, int nsub, hipStream_t st);
// ceil(nout / TILE_OUT) * ngroups workgroups; nout > 0
hipError_t launch_stage2(const Layout& l, const Params2& p, hipStream_t st);
hipError_t prepare_stage1(const Layout& l);
hipError_t prepare_stage2(const Layout& l);

}  // namespace subdedisp
}  // namespace rtlws
#endif
