"""librtlws_ffa.so (include/rtlws_ffa.h): the fast folding search of dedispersed series, bound as a submodule with its own
prototype table (the package's public names, Engine's methods and _Plan's subclasses are pinned, so a
library after the pin lives in a module of its own).  It needs librtlws_hip.so's engine.

  import rtlws, rtlws.ffa
  peak, at, prof = rtlws.ffa.search(engine, series, p0=250, nper=4, L=7, widths=(1, 2, 4), seg=1)
"""
import ctypes as C
import os

import numpy as np

from . import LIB_DIR, _PlanBase, _load, _outs, _p, _satellite           # noqa: F401  (_load: what _satellite loads through)

FFA_LIB = os.path.join(LIB_DIR, "librtlws_ffa.so")       # include/rtlws_ffa.h
MIN_P, MAX_P, MAX_L, MAX_CELLS, MAX_WIDTHS, MAX_WIDTH, MAX_TRIALS, MAX_PASSES = 16, 1024, 12, 1 << 22, 16, 256, 65536, 3
WORKSPACE_CAP = 1 << 30
GUARD = 8                  # search(fill=...): preset elements behind every output array

_i, _l, _vp, _ip, _d = C.c_int, C.c_long, C.c_void_p, C.POINTER(C.c_int), C.c_double
_PASSES = C.c_int * MAX_PASSES
_PROTOTYPES = {
    "rtlws_ffa_supported": [_i, _i, _i, _i, _vp, _i],
    "rtlws_ffa_geometry": [_i, _i, _i, _i, _vp, _i, _i, _ip, _PASSES, _PASSES, _ip, _PASSES, _ip, C.POINTER(C.c_size_t), _ip],
    "rtlws_ffa_open": ([_vp, _i, _i, _i, _i, _vp, _i, _i], _vp), "rtlws_ffa_samples_needed": ([_vp], _l),
    "rtlws_ffa_workspace_bytes": ([_vp], C.c_size_t), "rtlws_ffa_run": [_vp, _vp, _l, _i, _vp, _vp, _vp, _l, _vp],
    "rtlws_ffa_period": ([_i, _i, _i], _d), "rtlws_ffa_snr": ([_d, _i, _i, _d, _d, _l], _d),
    "rtlws_ffa_close": ([_vp], None), "rtlws_ffa_last_error": ([], C.c_char_p)}
SYMBOLS = list(_PROTOTYPES)


def lib():
    """librtlws_ffa.so (include/rtlws_ffa.h); it needs librtlws_hip.so's engine."""
    return _satellite(FFA_LIB, _PROTOTYPES)


def last_error():
    return lib().rtlws_ffa_last_error().decode()


def _widths(widths):
    """The table as the library reads it: int32 [nwidths], or None (a NULL table)."""
    return None if widths is None else np.ascontiguousarray(widths, dtype=np.int32).reshape(-1)


def _table(widths):
    widths = _widths(widths)
    return (0, None) if widths is None else (widths.size, _p(widths) if widths.size else None)


def supported(p0, nper, L, widths, seg):
    """rtlws_ffa_supported.  No GPU needed."""
    return lib().rtlws_ffa_supported(int(p0), int(nper), int(L), *_table(widths), int(seg))


def geometry(p0, nper, L, widths, seg, max_trials=1):
    """rtlws_ffa_geometry: (rc, passes, stages [3], workgroups per pair [3], threads, LDS bytes [3], merge, workspace
    bytes, pairs in flight).  No GPU needed."""
    return _outs(lib().rtlws_ffa_geometry, (int(p0), int(nper), int(L), *_table(widths), int(seg), int(max_trials)),
                 (C.c_int, _PASSES, _PASSES, C.c_int, _PASSES, C.c_int, C.c_size_t, C.c_int))


def period(p, s, L):
    """rtlws_ffa_period: p + s / (2^L - 1) in double, NaN where it is not defined.  No GPU needed."""
    return lib().rtlws_ffa_period(int(p), int(s), int(L))


def snr(peak, width, rows, sum1, sum2, count):
    """rtlws_ffa_snr: (peak - width rows mean) / sqrt(width rows var) in double, NaN where it is not defined.  No GPU
    needed."""
    return lib().rtlws_ffa_snr(float(peak), int(width), int(rows), float(sum1), float(sum2), int(count))


class FfaPlan(_PlanBase):
    """rtlws_ffa_plan* of include/rtlws_ffa.h: the table of widths (int32 [nwidths]) on the engine's device in the
    kernel's form, the workspace of max_trials trials (or what the cap holds) allocated, the kernels loaded.  eng may be
    None (as a C caller's NULL engine): open then fails with the library's text."""
    _name, _lib = "ffa", staticmethod(lib)

    def __init__(self, eng, p0, nper, L, widths, seg, max_trials=1):
        widths = _widths(widths)
        self.p0, self.nper, self.L, self.nwidths, self.seg = int(p0), int(nper), int(L), widths.size, int(seg)
        self.m, self.p_max = 1 << self.L, self.p0 + self.nper - 1
        self._open(eng, self.p0, self.nper, self.L, self.nwidths, _p(widths), self.seg, int(max_trials))
        self.nseg = self.m // self.seg

    def samples_needed(self):
        return self._fn("samples_needed")(self.h)

    def workspace_bytes(self):
        return self._fn("workspace_bytes")(self.h)

    def run(self, d_in, in_stride, ntrials, d_peak, d_at, d_prof=None, prof_stride=0, stream=None, check=True):
        """The passes of every group of pairs: trial t at d_in + t * in_stride elements; d_peak and d_at [ntrials, nper,
        nseg, nwidths] (f32, int32), d_prof [ntrials, nper, m, prof_stride] (f32) or None."""
        return self._call("run", check, self._ptr(d_in), int(in_stride), int(ntrials), self._ptr(d_peak), self._ptr(d_at),
                          self._ptr(d_prof), int(prof_stride), stream)


def search(engine, series, p0, nper, L, widths, seg, in_stride=None, want_prof=False, fill=None):
    """rtlws_ffa_run: series float32 [ntrials, nsamples] (with in_stride: [ntrials, in_stride], the padding as the caller
    left it), widths int32 [nwidths] -> (float32 [ntrials, nper, nseg, nwidths] the peaks, int32 of that shape their
    places s * p + c, float32 [ntrials, nper, m, p0 + nper - 1] the profiles, base period i in columns 0 .. p0 + i - 1
    and zeros behind them, or None without want_prof).  With `fill` (a float32) the three come back as the whole flat
    buffers, GUARD elements longer than the outputs, every element preset to fill (to fill's bits: the places), so that a
    caller sees what the run left untouched; without want_prof the run gets a NULL d_prof and the preset profiles come
    back as they were."""
    series, samples = engine._series(series, in_stride, "nsamples")
    ntrials, width = series.shape
    plan = FfaPlan(engine, p0, nper, L, widths, seg, max_trials=ntrials)
    try:
        assert samples >= plan.samples_needed(), "fewer samples than rtlws_ffa_samples_needed"
    except AssertionError:
        plan.close()
        raise
    npeaks, nprof = ntrials * plan.nper * plan.nseg * plan.nwidths, ntrials * plan.nper * plan.m * plan.p_max
    hosts = [engine._preset(npeaks, fill, GUARD), engine._preset(npeaks, fill, GUARD, np.int32),
             engine._preset(nprof if want_prof or fill is not None else 0, fill, GUARD)]
    got = engine._drive(plan, [series], [h if h.size else None for h in hosts], lambda i, o: plan.run(
        i[0], width, ntrials, o[0], o[1], o[2] if want_prof else None, plan.p_max))
    peak, at, prof = [h if g is None else g for g, h in zip(got, hosts)]
    if fill is not None:
        return peak, at, prof
    shape = (ntrials, plan.nper, plan.nseg, plan.nwidths)
    return peak.reshape(shape), at.reshape(shape), prof.reshape(ntrials, plan.nper, plan.m, plan.p_max) if want_prof else None
