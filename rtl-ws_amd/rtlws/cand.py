"""librtlws_cand.so (include/rtlws_cand.h): candidate folding of the waterfall into (sub-integration, channel, phase) cubes
and the refinement of a cube over DM and period / period-derivative offsets, bound as a submodule with its own prototype
table (the package's public names, Engine's methods and _Plan's subclasses are pinned, so a library after
the pin lives in a module of its own).  It needs librtlws_hip.so's engine.

  import rtlws, rtlws.cand
  cube, hits = rtlws.cand.fold(engine, rows, [rtlws.fold_step(period)], [0], nbins=64, sub=4096, delays=delays)
  a = rtlws.cand.dm_shifts(nchan, 1, f_centre, bandwidth, row_seconds, period, 64, 33, -4.0, 0.25)
  g = rtlws.cand.drift_shifts(64, 4096, cube.shape[1], 65, -df, df / 32)
  stat, total, prof, tphase = rtlws.cand.search(engine, cube, a[None], g[None])
"""
import ctypes as C
import os

import numpy as np

from . import LIB_DIR, _PlanBase, _load, _outs, _p, _satellite           # noqa: F401  (_load: what _satellite loads through)

CAND_LIB = os.path.join(LIB_DIR, "librtlws_cand.so")     # include/rtlws_cand.h
MAX_CANDS, MIN_NCHAN, MAX_NCHAN, MAX_DELAY, MIN_BINS, MAX_BINS = 64, 4, 4096, 65535, 2, 256
MIN_SUB, MAX_SUB, MAX_NSAMP, MAX_NSUB, MAX_NDM, MAX_NTR, MAX_WORKSPACE = 16, 1 << 24, 1 << 30, 1024, 256, 4096, 1 << 30
GUARD = 8                  # fold(fill=...), search(fill=...): preset elements behind every output array

_i, _l, _vp, _ip, _lp, _d = C.c_int, C.c_long, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_long), C.c_double
_PROTOTYPES = {
    "rtlws_cand_fold_supported": [_i, _i, _i, _l],
    "rtlws_cand_fold_geometry": [_i, _i, _i, _l, _l, _ip, _ip, _ip, _ip, _lp],
    "rtlws_cand_fold_open": ([_vp, _i, _vp, _vp, _i, _vp, _vp, _i, _l], _vp),
    "rtlws_cand_fold_rows_needed": ([_vp, _l], _l),
    "rtlws_cand_fold_run": [_vp, _vp, _l, _l, _vp, _vp, _vp],
    "rtlws_cand_fold_close": ([_vp], None),
    "rtlws_cand_search_supported": [_i, _i, _i, _i, _i, _i],
    "rtlws_cand_search_geometry": [_i, _i, _i, _i, _i, _i, _ip, _ip, _ip, _ip, _ip, _lp],
    "rtlws_cand_search_open": ([_vp, _i, _i, _i, _i, _i, _vp, _i, _vp], _vp),
    "rtlws_cand_search_run": [_vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "rtlws_cand_search_close": ([_vp], None),
    "rtlws_cand_dm_shifts": [_i, _i, _d, _d, _d, _d, _i, _i, _d, _d, _vp],
    "rtlws_cand_drift_shifts": [_i, _l, _i, _i, _d, _d, _i, _d, _d, _vp],
    "rtlws_cand_chi2": ([_d, _d, _i, _d], _d),
    "rtlws_cand_last_error": ([], C.c_char_p)}
SYMBOLS = list(_PROTOTYPES)


def lib():
    """librtlws_cand.so (include/rtlws_cand.h); it needs librtlws_hip.so's engine."""
    return _satellite(CAND_LIB, _PROTOTYPES)


def last_error():
    return lib().rtlws_cand_last_error().decode()


def _table(values, dtype):
    """A table as the library reads it: contiguous, of the header's type; None stays None (a NULL table)."""
    return None if values is None else np.ascontiguousarray(values, dtype=dtype)


def _ptr_of(table):
    return None if table is None else _p(table)


def fold_supported(ncand, nchan, nbins, sub):
    """rtlws_cand_fold_supported.  No GPU needed."""
    return lib().rtlws_cand_fold_supported(int(ncand), int(nchan), int(nbins), int(sub))


def fold_geometry(ncand, nchan, nbins, sub, nsamp=0):
    """rtlws_cand_fold_geometry: (rc, workgroups, threads, LDS bytes, waves_per_block, nsub).  No GPU needed."""
    return _outs(lib().rtlws_cand_fold_geometry, (int(ncand), int(nchan), int(nbins), int(sub), int(nsamp)), (C.c_int,) * 4 + (C.c_long,))


def search_supported(ncand, nsub, nchan, nbins, ndm, ntr):
    """rtlws_cand_search_supported.  No GPU needed."""
    return lib().rtlws_cand_search_supported(int(ncand), int(nsub), int(nchan), int(nbins), int(ndm), int(ntr))


def search_geometry(ncand, nsub, nchan, nbins, ndm, ntr):
    """rtlws_cand_search_geometry: (rc, workgroups of stage 1, of stage 2, threads, LDS bytes of stage 1, of stage 2,
    workspace bytes).  No GPU needed."""
    return _outs(lib().rtlws_cand_search_geometry, (int(ncand), int(nsub), int(nchan), int(nbins), int(ndm), int(ntr)),
                 (C.c_int,) * 5 + (C.c_long,))


def dm_shifts(nchan, shifted, f_centre_hz, bandwidth_hz, row_seconds, period_rows, nbins, ndm, ddm0, ddm_step):
    """rtlws_cand_dm_shifts: int32 [ndm, nchan], the phase shift of every channel under every DM offset.  No GPU needed."""
    a = np.zeros((max(int(ndm), 0), max(int(nchan), 0)), np.int32)
    if lib().rtlws_cand_dm_shifts(int(nchan), int(shifted), float(f_centre_hz), float(bandwidth_hz), float(row_seconds), float(period_rows),
                                  int(nbins), int(ndm), float(ddm0), float(ddm_step), _p(a)) != 0:
        raise ValueError(last_error())
    return a


def drift_shifts(nbins, sub, nsub, nf, df0, df_step, nfd=1, dfd0=0.0, dfd_step=0.0):
    """rtlws_cand_drift_shifts: int32 [nfd * nf, nsub], the phase shift of every sub-integration under every (frequency,
    derivative) offset, the frequency index fastest; an offset is the folding frequency less the trial's.  No GPU needed."""
    g = np.zeros((max(int(nf), 0) * max(int(nfd), 0), max(int(nsub), 0)), np.int32)
    if lib().rtlws_cand_drift_shifts(int(nbins), int(sub), int(nsub), int(nf), float(df0), float(df_step), int(nfd), float(dfd0),
                                     float(dfd_step), _p(g)) != 0:
        raise ValueError(last_error())
    return g


def chi2(stat, total, nbins, bin_variance):
    """rtlws_cand_chi2.  No GPU needed."""
    return lib().rtlws_cand_chi2(float(stat), float(total), int(nbins), float(bin_variance))


class _CandPlan(_PlanBase):
    """The library's two plans: rtlws_cand_<part>_open, _run and _close, one error slot for both."""
    _lib = staticmethod(lib)

    @classmethod
    def _fn(cls, what):
        return getattr(lib(), "rtlws_cand_last_error" if what == "last_error" else "rtlws_%s_%s" % (cls._name, what))


class CandFoldPlan(_CandPlan):
    """rtlws_cand_fold_plan* of include/rtlws_cand.h: the candidates' steps and phases (uint64 [ncand]), the delays (int32
    [ncand, nchan] or None: zeros) and the mask (uint8 [nchan] or None) on the engine's device, the kernel loaded.  eng
    may be None (as a C caller's NULL engine): open then fails with the library's text."""
    _name = "cand_fold"

    def __init__(self, eng, steps, phases, nchan, nbins, sub, delays=None, mask=None, ncand=None):
        steps, phases = _table(steps, np.uint64), _table(phases, np.uint64)
        delays, mask = _table(delays, np.int32), _table(mask, np.uint8)
        self.ncand = int(ncand) if ncand is not None else 0 if steps is None else steps.size
        self.nchan, self.nbins, self.sub = int(nchan), int(nbins), int(sub)
        assert phases is None or steps is None or steps.size == phases.size, "a phase for every step"
        assert delays is None or delays.size >= self.ncand * self.nchan, "fewer delays than ncand * nchan"
        assert mask is None or mask.size >= self.nchan, "fewer mask bytes than nchan"
        self._open(eng, self.ncand, _ptr_of(steps), _ptr_of(phases), self.nchan, _ptr_of(delays), _ptr_of(mask), self.nbins, self.sub)

    def rows_needed(self, nsamp):
        return self._fn("rows_needed")(self.h, int(nsamp))

    def subints(self, nsamp):
        return -(-int(nsamp) // self.sub)

    def run(self, d_rows, in_stride, nsamp, d_cube, d_hits=None, stream=None, check=True):
        """One launch: row j at d_rows + j * in_stride elements; d_cube [ncand, nsub, nchan, nbins] f32, d_hits
        [ncand, nsub, nbins] uint32 or None."""
        return self._call("run", check, self._ptr(d_rows), int(in_stride), int(nsamp), self._ptr(d_cube), self._ptr(d_hits), stream)


class CandSearchPlan(_CandPlan):
    """rtlws_cand_search_plan* of include/rtlws_cand.h: the shift tables a (int32 [ncand, ndm, nchan]) and g (int32
    [ncand, ntr, nsub]) and the workspace of T on the engine's device, both kernels loaded."""
    _name = "cand_search"

    def __init__(self, eng, ncand, nsub, nchan, nbins, a, g, ndm=None, ntr=None):
        a, g = _table(a, np.int32), _table(g, np.int32)
        self.ncand, self.nsub, self.nchan, self.nbins = int(ncand), int(nsub), int(nchan), int(nbins)
        per_a, per_g = max(self.ncand * self.nchan, 1), max(self.ncand * self.nsub, 1)
        self.ndm = int(ndm) if ndm is not None else 0 if a is None else a.size // per_a
        self.ntr = int(ntr) if ntr is not None else 0 if g is None else g.size // per_g
        assert a is None or a.size >= self.ncand * self.ndm * self.nchan, "fewer entries of a than ncand * ndm * nchan"
        assert g is None or g.size >= self.ncand * self.ntr * self.nsub, "fewer entries of g than ncand * ntr * nsub"
        self._open(eng, self.ncand, self.nsub, self.nchan, self.nbins, self.ndm, _ptr_of(a), self.ntr, _ptr_of(g))

    def run(self, d_cube, d_stat, d_total, d_prof=None, d_tphase=None, stream=None, check=True):
        """Two launches: d_cube as CandFoldPlan.run wrote it; d_stat and d_total [ncand, ndm, ntr] f64; d_prof [ncand,
        ndm, ntr, nbins] and d_tphase [ncand, ndm, nsub, nbins] f32, or None."""
        return self._call("run", check, self._ptr(d_cube), self._ptr(d_stat), self._ptr(d_total), self._ptr(d_prof), self._ptr(d_tphase), stream)


def fold(engine, rows, steps, phases, nbins, sub, delays=None, mask=None, nsamp=None, in_stride=None, nchan=None, want_hits=True, fill=None):
    """rtlws_cand_fold_run: rows float32 [nrows, nchan] (with in_stride and nchan: [nrows, in_stride], the first nchan
    values of a row its channels, the padding as the caller left it), steps and phases uint64 [ncand], delays int32 [ncand, nchan]
    or None, mask uint8 [nchan] or None -> (float32 [ncand, nsub, nchan, nbins] the cube, uint32 [ncand, nsub, nbins] the
    hits, or None without want_hits).  nsamp None: as many as the rows hold behind the largest delay.  With `fill` (a
    float32) the two come back as the whole flat buffers, GUARD elements longer than the outputs, every element preset to
    fill (the cube) and to fill's bits (the hits), so that a caller sees what the run left untouched; without want_hits
    the run gets a NULL d_hits and the preset hits buffer comes back as it was."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    if in_stride is not None:
        rows = rows.reshape(-1, int(in_stride))
    assert rows.ndim == 2, "the rows are [nrows, nchan]"
    width = rows.shape[1]
    nchan = width if nchan is None else int(nchan)
    plan = CandFoldPlan(engine, steps, phases, nchan, nbins, sub, delays, mask)
    try:
        if nsamp is None:
            nsamp = max(rows.shape[0] - (plan.rows_needed(1) - 1), 0)
        nsamp = int(nsamp)
        assert rows.shape[0] >= plan.rows_needed(nsamp), "fewer rows than rtlws_cand_fold_rows_needed"
    except AssertionError:
        plan.close()
        raise
    ncand, nsub = plan.ncand, plan.subints(nsamp)
    hosts = [engine._preset(ncand * nsub * nchan * plan.nbins, fill, GUARD), engine._preset(ncand * nsub * plan.nbins, fill, GUARD, np.uint32)]
    cube, hits = engine._drive(plan, [rows], hosts, lambda i, o: plan.run(i[0], width, nsamp, o[0], o[1] if want_hits else None))
    if fill is not None:
        return cube, hits
    return cube.reshape(ncand, nsub, nchan, plan.nbins), hits.reshape(ncand, nsub, plan.nbins) if want_hits else None


def search(engine, cube, a, g, want_prof=True, want_tphase=True, fill=None):
    """rtlws_cand_search_run: cube float32 [ncand, nsub, nchan, nbins], a int32 [ncand, ndm, nchan], g int32 [ncand, ntr,
    nsub] -> (float64 [ncand, ndm, ntr] stat and total, float32 [ncand, ndm, ntr, nbins] the profiles P and [ncand, ndm,
    nsub, nbins] the time-phase rows T, each None where it is not wanted).  With `fill` (a float32) the four come back as
    the whole flat buffers, GUARD elements longer than the outputs, every element preset to fill (float64(fill) for the
    sums); an output that is not wanted gets a NULL pointer and its preset buffer comes back as it was."""
    cube = np.ascontiguousarray(cube, dtype=np.float32)
    assert cube.ndim == 4, "the cube is [ncand, nsub, nchan, nbins]"
    ncand, nsub, nchan, nbins = cube.shape
    a, g = np.ascontiguousarray(a, dtype=np.int32), np.ascontiguousarray(g, dtype=np.int32)
    assert a.ndim == 3 and a.shape[0] == ncand and a.shape[2] == nchan, "a is [ncand, ndm, nchan]"
    assert g.ndim == 3 and g.shape[0] == ncand and g.shape[2] == nsub, "g is [ncand, ntr, nsub]"
    ndm, ntr = a.shape[1], g.shape[1]
    plan = CandSearchPlan(engine, ncand, nsub, nchan, nbins, a, g)
    hosts = [engine._preset(ncand * ndm * ntr, fill, GUARD, np.float64), engine._preset(ncand * ndm * ntr, fill, GUARD, np.float64),
             engine._preset(ncand * ndm * ntr * nbins if want_prof or fill is not None else 0, fill, GUARD),
             engine._preset(ncand * ndm * nsub * nbins if want_tphase or fill is not None else 0, fill, GUARD)]
    got = engine._drive(plan, [cube], [h if h.size else None for h in hosts], lambda i, o: plan.run(
        i[0], o[0], o[1], o[2] if want_prof else None, o[3] if want_tphase else None))
    stat, total, prof, tphase = [h if v is None else v for v, h in zip(got, hosts)]
    if fill is not None:
        return stat, total, prof, tphase
    return (stat.reshape(ncand, ndm, ntr), total.reshape(ncand, ndm, ntr), prof.reshape(ncand, ndm, ntr, nbins) if want_prof else None,
            tphase.reshape(ncand, ndm, nsub, nbins) if want_tphase else None)
