"""librtlws_subdedisp.so (include/rtlws_subdedisp.h): two-stage (subband) incoherent dedispersion -- the subbands' sums
of every nominal trial, then every trial over the subband series of its nominal, two launches -- bound as a submodule with
its own prototype table (the package's public names, Engine's methods and _Plan's subclasses are pinned,
so a library after the pin lives in a module of its own).  It needs librtlws_hip.so's engine.

  import rtlws, rtlws.subdedisp
  first, d1, d2, smear = rtlws.subdedisp.delays(1024, 64, 1, 408e6, 2.4e6, 2048 / 2.4e6, 256, 0.0, 0.5, per_nominal=16)
  series = rtlws.subdedisp.dedisperse(engine, rows, first, d1, d2)        # float32 [256, nout], as engine.dedisp gives them
"""
import ctypes as C
import os

import numpy as np

from . import LIB_DIR, _PlanBase, _load, _outs, _p, _satellite           # noqa: F401  (_load: what _satellite loads through)

SUBDEDISP_LIB = os.path.join(LIB_DIR, "librtlws_subdedisp.so")   # include/rtlws_subdedisp.h
MIN_NCHAN, MAX_NCHAN, MIN_PER_SUB, MAX_NOMINALS, MAX_TRIALS, MAX_DELAY = 4, 4096, 4, 4096, 4096, 65535
GUARD = 8                  # dedisperse(fill=...): preset elements behind the outputs and behind the workspace

_i, _l, _vp, _ip, _d = C.c_int, C.c_long, C.c_void_p, C.POINTER(C.c_int), C.c_double
_PROTOTYPES = {
    "rtlws_subdedisp_supported": [_i, _i, _i, _i],
    "rtlws_subdedisp_delays": [_i, _i, _i, _d, _d, _d, _i, _d, _d, _i, _vp, _vp, _vp, C.POINTER(_d)],
    "rtlws_subdedisp_geometry": [_i, _i, _i, _i, _vp, _vp, _vp, _vp, _l, _ip, _ip, _ip, _ip, _ip, _ip, _ip, _ip],
    "rtlws_subdedisp_open": ([_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp], _vp),
    "rtlws_subdedisp_rows_needed": ([_vp, _l], _l),
    "rtlws_subdedisp_mid_stride": ([_vp, _l], _l),
    "rtlws_subdedisp_work_floats": ([_vp, _l], _l),
    "rtlws_subdedisp_run": [_vp, _vp, _l, _l, _vp, _vp, _l, _vp],
    "rtlws_subdedisp_close": ([_vp], None),
    "rtlws_subdedisp_last_error": ([], C.c_char_p)}
SYMBOLS = list(_PROTOTYPES)


def lib():
    """librtlws_subdedisp.so (include/rtlws_subdedisp.h); it needs librtlws_hip.so's engine."""
    return _satellite(SUBDEDISP_LIB, _PROTOTYPES)


def last_error():
    return lib().rtlws_subdedisp_last_error().decode()


def supported(nchan, nsub, nnominal, ntrials):
    """rtlws_subdedisp_supported.  No GPU needed."""
    return lib().rtlws_subdedisp_supported(int(nchan), int(nsub), int(nnominal), int(ntrials))


def delays(nchan, nsub, shifted, f_centre_hz, bandwidth_hz, row_seconds, ntrials, dm0, dm_step, per_nominal):
    """rtlws_subdedisp_delays: the tables of ntrials dispersion measures dm0 + t dm_step, per_nominal trials a nominal ->
    (first int32 [A + 1], d1 int32 [A, nchan], d2 int32 [ntrials, nsub], smear_rows), A = ceil(ntrials / per_nominal).
    No GPU needed."""
    nchan, nsub, ntrials, per = int(nchan), int(nsub), int(ntrials), int(per_nominal)
    A = -(-max(ntrials, 0) // per) if per >= 1 else 0
    first, d1, d2 = np.zeros(A + 1, np.int32), np.zeros((A, max(nchan, 0)), np.int32), np.zeros((max(ntrials, 0), max(nsub, 0)), np.int32)
    smear = C.c_double(0.0)
    rc = lib().rtlws_subdedisp_delays(nchan, nsub, int(shifted), float(f_centre_hz), float(bandwidth_hz), float(row_seconds), ntrials,
                                      float(dm0), float(dm_step), per, _p(first), _p(d1), _p(d2), C.byref(smear))
    if rc != 0:
        raise RuntimeError("rtlws_subdedisp_delays failed (rc=%d): %s" % (rc, last_error()))
    return first, d1, d2, smear.value


def _tables(first, d1, d2, mask):
    """first int32 [A + 1], d1 int32 [A, nchan], d2 int32 [ntrials, nsub] and the mask (uint8 [nchan] or None) as the
    library reads them"""
    first = np.ascontiguousarray(first, dtype=np.int32).reshape(-1)
    d1, d2 = np.ascontiguousarray(d1, dtype=np.int32), np.ascontiguousarray(d2, dtype=np.int32)
    if d1.ndim != 2 or d2.ndim != 2 or first.size != d1.shape[0] + 1:
        raise RuntimeError("rtlws_subdedisp: the tables are first [nnominal + 1], d1 [nnominal, nchan] and d2 [ntrials, nsub]")
    if mask is not None:
        mask = np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
        if mask.size != d1.shape[1]:
            raise RuntimeError("rtlws_subdedisp: the mask holds nchan bytes")
    return first, d1, d2, mask


def geometry(first, d1, d2, mask=None, nout=0):
    """rtlws_subdedisp_geometry of the tables: (rc, workgroups, threads, LDS bytes -- a tuple of two each, stage 1 then stage
    2 --, outputs per workgroup, nominals per workgroup of stage 1, trials per workgroup of stage 2, max_d1, max_d2).  No
    GPU needed."""
    first, d1, d2, mask = _tables(first, d1, d2, mask)
    return _outs(lib().rtlws_subdedisp_geometry, (d1.shape[1], d2.shape[1], d1.shape[0], d2.shape[0], _p(first), _p(d1), _p(d2),
                                                  None if mask is None else _p(mask), int(nout)), (C.c_int * 2,) * 3 + (C.c_int,) * 5)


class SubdedispPlan(_PlanBase):
    """rtlws_subdedisp_plan* of include/rtlws_subdedisp.h: the tables and the mask on the engine's device in the kernels'
    forms, both kernels loaded.  eng may be None (as a C caller's NULL engine): open then fails with the library's text."""
    _name = "subdedisp"
    _lib = staticmethod(lib)

    def __init__(self, eng, first, d1, d2, mask=None):
        first, d1, d2, mask = _tables(first, d1, d2, mask)
        (self.nnominal, self.nchan), (self.ntrials, self.nsub) = d1.shape, d2.shape
        self._open(eng, self.nchan, self.nsub, self.nnominal, self.ntrials, _p(first), _p(d1), _p(d2), None if mask is None else _p(mask))

    def rows_needed(self, nout):
        return self._fn("rows_needed")(self.h, int(nout))

    def mid_stride(self, nout):
        return self._fn("mid_stride")(self.h, int(nout))

    def work_floats(self, nout):
        return self._fn("work_floats")(self.h, int(nout))

    def run(self, d_rows, nout, d_work, d_out, in_stride=None, out_stride=None, stream=None, check=True):
        """Two launches: row j of the input at d_rows + j * in_stride elements, the subband series into d_work
        (work_floats(nout) f32), trial t at d_out + t * out_stride."""
        return self._call("run", check, self._ptr(d_rows), int(self.nchan if in_stride is None else in_stride), int(nout), self._ptr(d_work),
                          self._ptr(d_out), int(nout if out_stride is None else out_stride), stream)


def dedisperse(engine, rows, first, d1, d2, mask=None, nout=None, in_stride=None, out_stride=None, fill=None, want_subbands=False):
    """rtlws_subdedisp_run: rows float32 [nrows, nchan] (with in_stride: [nrows, in_stride], the padding as the caller left
    it) and the tables of _tables -> float32 [ntrials, nout]; nout None: as many as the rows hold.  want_subbands: (that,
    P float32 [nnominal, nsub, mid_stride], the words at and behind nmid = nout + max_d2 as they were preset).  With
    out_stride the whole buffer [ntrials, out_stride] comes back.  With `fill` (a float32) every element of the outputs
    and of the workspace is preset to it and both come back as the whole flat buffers, GUARD elements longer, so that a
    caller sees what the run left untouched (P then comes back whether wanted or not: (out, P))."""
    plan = SubdedispPlan(engine, first, d1, d2, mask)
    width = plan.nchan if in_stride is None else int(in_stride)
    rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, width)
    if nout is None:
        nout = max(rows.shape[0] - (plan.rows_needed(1) - 1), 0)
    nout = int(nout)
    assert rows.shape[0] >= plan.rows_needed(nout), "fewer rows than rtlws_subdedisp_rows_needed"
    stride = nout if out_stride is None else int(out_stride)
    mid, floats = max(plan.mid_stride(nout), 0), max(plan.work_floats(nout), 0)
    nnominal, nsub, ntrials = plan.nnominal, plan.nsub, plan.ntrials
    hosts = [engine._preset(ntrials * max(stride, 0), fill, GUARD), engine._preset(floats, fill, GUARD)]
    out, work = engine._drive(plan, [rows], hosts, lambda i, o: plan.run(i[0], nout, o[1], o[0], width, stride))
    if fill is not None:
        return out, work
    out = out.reshape(ntrials, max(stride, 0))
    out = out if out_stride is not None else out[:, :nout]
    return (out, work.reshape(nnominal, nsub, mid)) if want_subbands else out
