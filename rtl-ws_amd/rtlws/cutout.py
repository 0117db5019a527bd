"""librtlws_cutout.so (include/rtlws_cutout.h): cutouts of single-pulse candidates -- for every candidate of the list
rtlws_sift_run leaves on the device, the waterfall dedispersed at the candidate's trial in time bins and subbands, and
the series of the neighbouring trials in the same bins, two launches -- bound as a submodule with its own prototype
table (the package's public names, Engine's methods and _Plan's subclasses are pinned, so a library
after the pin lives in a module of its own).  It needs librtlws_hip.so's engine.

  import rtlws, rtlws.sift, rtlws.cutout
  series = engine.dedisp(rows, delays, mask, nout=nsamp)
  cand, count = rtlws.sift.sift(engine, peak, at, mom, widths, seg, nout, 7.0, rt=16, rs=2, max_cand=64)
  ft, dmt, info = rtlws.cutout.cutout(engine, rows, series, cand, count, delays, mask, widths, bins, nx=64, nf=32, rq=8, dq=1)
"""
import ctypes as C
import os

import numpy as np

from . import LIB_DIR, _PlanBase, _load, _outs, _p, _satellite           # noqa: F401  (_load: what _satellite loads through)

CUTOUT_LIB = os.path.join(LIB_DIR, "librtlws_cutout.so")   # include/rtlws_cutout.h
MIN_NCHAN, MAX_NCHAN, MAX_TRIALS, MAX_DELAY, MAX_WIDTHS, MAX_WIDTH, MAX_BIN = 4, 4096, 4096, 65535, 16, 1024, 1024
MIN_NX, MAX_NX, MAX_NF, MAX_RQ, MAX_DQ, MAX_NSAMP, MAX_CAND = 4, 256, 4096, 64, 64, 1 << 30, 4096
CAND_WORDS = 8             # the sift's candidate; words 0 (t), 2 (k) and 3 (at) are read
INFO_WORDS = 4             # {n0, b, valid, the rows of the window inside 0 .. nsamp - 1}
GUARD = 8                  # cutout(fill=...): preset elements behind every output

_i, _l, _vp, _ip, _lp = C.c_int, C.c_long, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_long)
_PROTOTYPES = {
    "rtlws_cutout_supported": [_i, _i, _i, _vp, _vp, _i, _i, _i, _i],
    "rtlws_cutout_geometry": [_i, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _ip, _ip, _ip, _ip, _ip],
    "rtlws_cutout_open": ([_vp, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i], _vp),
    "rtlws_cutout_rows_needed": ([_vp, _l], _l),
    "rtlws_cutout_window": [_l, _i, _i, _i, _l, _lp, _lp],
    "rtlws_cutout_run": [_vp, _vp, _l, _vp, _l, _l, _vp, _vp, _i, _vp, _vp, _vp, _vp],
    "rtlws_cutout_close": ([_vp], None),
    "rtlws_cutout_last_error": ([], C.c_char_p)}
SYMBOLS = list(_PROTOTYPES)


def lib():
    """librtlws_cutout.so (include/rtlws_cutout.h); it needs librtlws_hip.so's engine."""
    return _satellite(CUTOUT_LIB, _PROTOTYPES)


def last_error():
    return lib().rtlws_cutout_last_error().decode()


def _table(a):
    return np.ascontiguousarray(a, dtype=np.int32).reshape(-1)


def _tables(delays, mask, widths, bins):
    """(nchan, ntrials, delays, mask or None, nwidths, widths, bins) as the library takes them; delays is [ntrials, nchan]"""
    delays = np.ascontiguousarray(delays, dtype=np.int32)
    assert delays.ndim == 2, "delays are [ntrials, nchan]"
    mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
    assert mask is None or mask.size == delays.shape[1], "mask is [nchan]"
    widths, bins = _table(widths), _table(bins)
    assert bins.size == widths.size, "a bin for every width"
    return delays.shape[1], delays.shape[0], delays, mask, widths.size, widths, bins


def supported(nchan, ntrials, widths, bins, nx, nf, rq, dq):
    """rtlws_cutout_supported.  No GPU needed."""
    w, b = _table(widths), _table(bins)
    return lib().rtlws_cutout_supported(int(nchan), int(ntrials), w.size, _p(w), _p(b), int(nx), int(nf), int(rq), int(dq))


def geometry(delays, mask, widths, bins, nx, nf, rq, dq, max_cand=1):
    """rtlws_cutout_geometry: (rc, workgroups, threads, LDS bytes -- a tuple of two each: band-time, DM-time --, ndm,
    max_delay).  No GPU needed."""
    nchan, ntrials, d, m, K, w, b = _tables(delays, mask, widths, bins)
    return _outs(lib().rtlws_cutout_geometry, (nchan, ntrials, _p(d), None if m is None else _p(m), K, _p(w), _p(b), int(nx), int(nf), int(rq), int(dq),
                                               int(max_cand)), (C.c_int * 2,) * 3 + (C.c_int, C.c_int))


def window(at, width, bin, nx, nsamp):
    """rtlws_cutout_window: (rc, n0, the rows of the window inside 0 .. nsamp - 1).  No GPU needed."""
    return _outs(lib().rtlws_cutout_window, (int(at), int(width), int(bin), int(nx), int(nsamp)), (C.c_long, C.c_long))


class CutoutPlan(_PlanBase):
    """rtlws_cutout_plan* of include/rtlws_cutout.h: the tables on the engine's device, the kernels loaded.  eng may be
    None (as a C caller's NULL engine): open then fails with the library's text."""
    _name = "cutout"
    _lib = staticmethod(lib)

    def __init__(self, eng, delays, mask, widths, bins, nx, nf, rq, dq):
        self.nchan, self.ntrials, d, m, self.nwidths, w, b = _tables(delays, mask, widths, bins)
        self.nx, self.nf, self.rq, self.dq, self.ndm = int(nx), int(nf), int(rq), int(dq), 2 * int(rq) + 1
        self._open(eng, self.nchan, self.ntrials, _p(d), None if m is None else _p(m), self.nwidths, _p(w), _p(b), self.nx, self.nf, self.rq, self.dq)

    def rows_needed(self, nsamp):
        return self._fn("rows_needed")(self.h, int(nsamp))

    def run(self, d_rows, in_stride, d_series, series_stride, nsamp, d_cand, d_count, max_cand, d_ft, d_dmt, d_info, stream=None, check=True):
        """Up to two launches over the waterfall, the series and the sift's list: the band-time planes into d_ft
        (max_cand * nf * nx f32), the DM-time planes into d_dmt (max_cand * ndm * nx f32), either of which may be None, and
        d_info (max_cand * 4 int32)."""
        return self._call("run", check, self._ptr(d_rows), int(in_stride), self._ptr(d_series), int(series_stride), int(nsamp), self._ptr(d_cand),
                          self._ptr(d_count), int(max_cand), self._ptr(d_ft), self._ptr(d_dmt), self._ptr(d_info), stream)


def cutout(engine, rows, series, cand, count, delays, mask, widths, bins, nx, nf, rq, dq, nsamp=None, max_cand=None, want_ft=True, want_dmt=True,
           fill=None):
    """rtlws_cutout_run: rows float32 [nrows, nchan] and series float32 [ntrials, nsamp] as Engine.dedisp takes and gives
    them (series may be None without want_dmt, rows without want_ft), cand uint32 [n, 8] and count int32 [2] as
    rtlws.sift.sift gives them (or a list of the caller's in that form) -> (float32 [m, nf, nx] the band-time planes,
    float32 [m, ndm, nx] the DM-time planes, int32 [m, 4] the info), m = min(count[0], max_cand); a plane not wanted is
    None.  max_cand None: the candidates given.  With `fill` (a float32) the three come back as the whole flat buffers
    of max_cand candidates, GUARD elements longer, every element preset to fill (its bits in the info), so that a caller
    sees what the run left untouched; a plane not wanted comes back as it was preset."""
    plan = CutoutPlan(engine, delays, mask, widths, bins, nx, nf, rq, dq)
    cand = np.ascontiguousarray(cand, dtype=np.uint32).reshape(-1, CAND_WORDS)
    count = np.ascontiguousarray(count, dtype=np.int32).reshape(-1)
    max_cand = max(len(cand), 1) if max_cand is None else int(max_cand)
    if len(cand) == 0:
        cand = np.zeros((1, CAND_WORDS), np.uint32)
    rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, plan.nchan)
    series = None if series is None else np.ascontiguousarray(series, dtype=np.float32).reshape(plan.ntrials, -1)
    if nsamp is None:
        nsamp = series.shape[1] if series is not None else rows.shape[0] - (plan.rows_needed(1) - 1)
    nsamp = int(nsamp)
    assert rows is None or rows.shape[0] >= plan.rows_needed(nsamp), "fewer rows than rtlws_cutout_rows_needed"
    assert series is None or series.shape[1] >= nsamp, "series shorter than nsamp"
    assert len(cand) >= min(max(int(count[0]), 0), max(max_cand, 0)), "fewer candidates than the count serves"
    room = max(max_cand, 0)
    sizes = (room * plan.nf * plan.nx, room * plan.ndm * plan.nx, room * INFO_WORDS)
    hosts = [engine._preset(sizes[0], fill, GUARD), engine._preset(sizes[1], fill, GUARD), engine._preset(sizes[2], fill, GUARD, np.int32)]
    stride = series.shape[1] if series is not None else nsamp
    got = engine._drive(plan, [rows, series, cand, count], hosts, lambda i, o: plan.run(
        i[0], plan.nchan, i[1], stride, nsamp, i[2], i[3], max_cand, o[0] if want_ft else None, o[1] if want_dmt else None, o[2]))
    if fill is not None:
        return tuple(got)
    m = min(max(int(count[0]), 0), room)
    ft, dmt, info = got
    return (ft.reshape(room, plan.nf, plan.nx)[:m] if want_ft else None, dmt.reshape(room, plan.ndm, plan.nx)[:m] if want_dmt else None,
            info.reshape(room, INFO_WORDS)[:m])
