"""librtlws_sift.so (include/rtlws_sift.h): the sift of single-pulse peaks -- the best width of every (trial, segment),
the local maxima at or above a threshold over a box of trials and segments, those as a list of 32-byte candidates in
(segment, trial) order, three launches -- bound as a submodule with its own prototype table (the
package's public names, Engine's methods and _Plan's subclasses are pinned, so a library after the pin lives in a module
of its own).  It needs librtlws_hip.so's engine.

  import rtlws, rtlws.sift
  peak, at, mom = engine.pulse(series, widths, seg)
  cand, count = rtlws.sift.sift(engine, peak, at, mom, widths, seg, nout, 7.0, rt=16, rs=2, max_cand=4096)
"""
import ctypes as C
import os

import numpy as np

from . import LIB_DIR, _PlanBase, _load, _outs, _p, _satellite           # noqa: F401  (_load: what _satellite loads through)

SIFT_LIB = os.path.join(LIB_DIR, "librtlws_sift.so")   # include/rtlws_sift.h
MAX_WIDTHS, MAX_WIDTH, MIN_SEG, MAX_SEG, MAX_TRIALS, MAX_NOUT, MAX_RT, MAX_RS, MAX_CAND = 16, 1024, 64, 1048576, 65536, 1 << 30, 32, 8, 1 << 24
CAND_WORDS = 8             # {t, s, k, at, bits of score, bits of peak_k, members, (t_hi << 16) | t_lo}
GUARD = 8                  # sift(fill=...): preset elements behind every output and behind the workspace

_i, _l, _vp, _ip, _f = C.c_int, C.c_long, C.c_void_p, C.POINTER(C.c_int), C.c_float
_PROTOTYPES = {
    "rtlws_sift_supported": [_i, _vp, _l, _i, _i],
    "rtlws_sift_geometry": [_i, _vp, _l, _i, _i, _i, _l, _ip, _ip, _ip, _ip, _ip, C.POINTER(_l)],
    "rtlws_sift_open": ([_vp, _i, _vp, _l, _i, _i], _vp),
    "rtlws_sift_work_bytes": ([_vp, _i, _l], _l),
    "rtlws_sift_run": [_vp, _vp, _vp, _vp, _i, _l, _f, _i, _vp, _vp, _vp, _vp, _vp, _vp],
    "rtlws_sift_close": ([_vp], None),
    "rtlws_sift_last_error": ([], C.c_char_p)}
SYMBOLS = list(_PROTOTYPES)


def lib():
    """librtlws_sift.so (include/rtlws_sift.h); it needs librtlws_hip.so's engine."""
    return _satellite(SIFT_LIB, _PROTOTYPES)


def last_error():
    return lib().rtlws_sift_last_error().decode()


def _widths(widths):
    return np.ascontiguousarray(widths, dtype=np.int32).reshape(-1)


def supported(widths, seg, rt, rs):
    """rtlws_sift_supported.  No GPU needed."""
    w = _widths(widths)
    return lib().rtlws_sift_supported(w.size, _p(w), int(seg), int(rt), int(rs))


def geometry(widths, seg, rt, rs, ntrials=1, nout=1):
    """rtlws_sift_geometry: (rc, workgroups, threads, LDS bytes -- a tuple of three each: scoring, the box, the list --,
    the tile's trials, its segments, nseg).  No GPU needed."""
    w = _widths(widths)
    return _outs(lib().rtlws_sift_geometry, (w.size, _p(w), int(seg), int(rt), int(rs), int(ntrials), int(nout)), (C.c_int * 3,) * 3 + (C.c_int, C.c_int, C.c_long))


class SiftPlan(_PlanBase):
    """rtlws_sift_plan* of include/rtlws_sift.h: the widths on the engine's device, the three kernels loaded.  eng may be
    None (as a C caller's NULL engine): open then fails with the library's text."""
    _name = "sift"
    _lib = staticmethod(lib)

    def __init__(self, eng, widths, seg, rt, rs):
        w = _widths(widths)
        self.nwidths, self.seg, self.rt, self.rs = w.size, int(seg), int(rt), int(rs)
        self._open(eng, w.size, _p(w), self.seg, self.rt, self.rs)

    def work_bytes(self, ntrials, nout):
        return self._fn("work_bytes")(self.h, int(ntrials), int(nout))

    def run(self, d_peak, d_at, d_mom, ntrials, nout, threshold, max_cand, d_work, d_cand, d_count, d_score=None, d_k=None, stream=None, check=True):
        """Three launches over the buffers rtlws_pulse_run wrote: the candidates into d_cand (max_cand * 8 words), their
        number and that of the events at or above threshold into d_count, the plane into d_score and d_k where given."""
        return self._call("run", check, self._ptr(d_peak), self._ptr(d_at), self._ptr(d_mom), int(ntrials), int(nout), float(threshold), int(max_cand),
                          self._ptr(d_work), self._ptr(d_cand), self._ptr(d_count), self._ptr(d_score), self._ptr(d_k), stream)


def sift(engine, peak, at, mom, widths, seg, nout, threshold, rt, rs, max_cand, want_plane=False, fill=None):
    """rtlws_sift_run: peak float32 and at int32 [ntrials, nwidths, nseg], mom float64 [ntrials, nseg, 2] as Engine.pulse
    gives them for nout outputs -> (uint32 [n, 8] the candidates, n = min(found, max_cand), int32 [2] the counts); with
    want_plane also (float32 [ntrials, nseg] the scores, int32 of that shape the widths' indices).  With `fill` (a float32)
    every output and the workspace are preset to its bits and come back as the whole flat buffers, GUARD elements longer:
    (cand uint32, count int32, score float32, k int32, work uint32), so that a caller sees what the run left untouched."""
    plan = SiftPlan(engine, widths, seg, rt, rs)
    peak, at = np.ascontiguousarray(peak, dtype=np.float32), np.ascontiguousarray(at, dtype=np.int32)
    mom = np.ascontiguousarray(mom, dtype=np.float64)
    assert peak.ndim == 3 and peak.shape == at.shape and mom.shape == (peak.shape[0], peak.shape[2], 2), "peak and at are [ntrials, nwidths, nseg], mom [ntrials, nseg, 2]"
    ntrials, nseg = peak.shape[0], peak.shape[2]
    nout, max_cand = int(nout), int(max_cand)
    assert peak.shape[1] == plan.nwidths and nseg == max(-(-nout // plan.seg), 0), "the arrays are not those of nout outputs"
    plane = ntrials * nseg if want_plane or fill is not None else 0
    words = max(plan.work_bytes(ntrials, nout), 0) // 4
    if fill is None:
        hosts = [(np.uint32, (max(max_cand, 0) * CAND_WORDS,)), (np.int32, (2,)), (np.float32, (plane,)) if plane else None,
                 (np.int32, (plane,)) if plane else None, (np.uint32, (words,))]
    else:
        hosts = [engine._preset(max(max_cand, 0) * CAND_WORDS, fill, GUARD, np.uint32), engine._preset(2, fill, GUARD, np.int32),
                 engine._preset(plane, fill, GUARD), engine._preset(plane, fill, GUARD, np.int32), engine._preset(words, fill, GUARD, np.uint32)]
    cand, count, score, k, work = engine._drive(plan, [peak, at, mom], hosts, lambda i, o: plan.run(
        i[0], i[1], i[2], ntrials, nout, threshold, max_cand, o[4], o[0], o[1], o[2], o[3]))
    if fill is not None:
        return cand, count, score, k, work
    cand = cand.reshape(-1, CAND_WORDS)[:min(int(count[0]), max_cand)]
    return (cand, count, score.reshape(ntrials, nseg), k.reshape(ntrials, nseg)) if want_plane else (cand, count)
