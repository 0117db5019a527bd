"""librtlws_cdd.so (include/rtlws_cdd.h): coherent dedispersion of channelizer streams, bound as a submodule with its own
prototype table (the package's public names, Engine's methods and _Plan's subclasses are pinned, so a
library after the pin lives in a module of its own).  It needs librtlws_hip.so's engine.

  import rtlws, rtlws.cdd
  lead, trail = rtlws.cdd.overlap(1400.0, 1.0, 50.0)
  tables = np.stack([rtlws.cdd.chirp(12, f, 1.0, 50.0) for f in centres_mhz])
  rows = rtlws.cdd.dedisperse(engine, streams, tables, lead, trail, ksum=16, layout="time")
"""
import ctypes as C
import os

import numpy as np

from . import LIB_DIR, _PlanBase, _load, _outs, _p, _satellite           # noqa: F401  (_load: what _satellite loads through)

CDD_LIB = os.path.join(LIB_DIR, "librtlws_cdd.so")       # include/rtlws_cdd.h
MIN_LOG2_NFFT, MAX_LOG2_NFFT, MAX_NCHAN, MAX_NSEG = 9, 14, 1024, 1 << 20
CHANNEL_MAJOR, TIME_MAJOR = 0, 1
GUARD = 8                  # dedisperse(fill=...): preset elements behind the output array

_LAYOUTS = {"channel": CHANNEL_MAJOR, "time": TIME_MAJOR}
_i, _l, _vp, _ip, _d = C.c_int, C.c_long, C.c_void_p, C.POINTER(C.c_int), C.c_double
_PROTOTYPES = {
    "rtlws_cdd_supported": [_i, _i, _i, _i, _i],
    "rtlws_cdd_geometry": [_i, _i, _i, _i, _i, _l, _ip, _ip, _ip],
    "rtlws_cdd_open": ([_vp, _i, _i, _i, _i, _i, _vp], _vp), "rtlws_cdd_samples_needed": ([_vp, _l], _l),
    "rtlws_cdd_run": [_vp, _vp, _l, _l, _vp, _l, _i, _vp],
    "rtlws_cdd_chirp": [_i, _d, _d, _d, _vp], "rtlws_cdd_overlap": [_d, _d, _d, _ip, _ip],
    "rtlws_cdd_close": ([_vp], None), "rtlws_cdd_last_error": ([], C.c_char_p)}
SYMBOLS = list(_PROTOTYPES)


def lib():
    """librtlws_cdd.so (include/rtlws_cdd.h); it needs librtlws_hip.so's engine."""
    return _satellite(CDD_LIB, _PROTOTYPES)


def last_error():
    return lib().rtlws_cdd_last_error().decode()


def _layout(layout):
    return _LAYOUTS.get(layout, layout)


def _tables(tables):
    """The tables as the library reads them: complex64 [nchan, N] (pairs of f32), or None (a NULL table)."""
    return None if tables is None else np.ascontiguousarray(np.atleast_2d(np.asarray(tables)), dtype=np.complex64)


def supported(log2_nfft, lead, trail, nchan, ksum=0):
    """rtlws_cdd_supported.  No GPU needed."""
    return lib().rtlws_cdd_supported(int(log2_nfft), int(lead), int(trail), int(nchan), int(ksum))


def geometry(log2_nfft, lead, trail, nchan, ksum=0, nseg=1):
    """rtlws_cdd_geometry: (rc, workgroups, threads, LDS bytes).  No GPU needed."""
    return _outs(lib().rtlws_cdd_geometry, (int(log2_nfft), int(lead), int(trail), int(nchan), int(ksum), int(nseg)), (C.c_int,) * 3)


def chirp(log2_nfft, f_centre_mhz, rate_mhz, dm):
    """rtlws_cdd_chirp: the dedispersing table of one channel, complex64 [N] in natural bin order.  No GPU needed."""
    n = 1 << int(log2_nfft) if MIN_LOG2_NFFT <= int(log2_nfft) <= MAX_LOG2_NFFT else 1
    table = np.zeros(n, np.complex64)
    if lib().rtlws_cdd_chirp(int(log2_nfft), float(f_centre_mhz), float(rate_mhz), float(dm), _p(table)) != 0:
        raise ValueError(last_error())
    return table


def overlap(f_centre_mhz, rate_mhz, dm):
    """rtlws_cdd_overlap: (lead, trail), the least overlap a plan of chirp()'s table should be opened with.  No GPU
    needed."""
    rc, lead, trail = _outs(lib().rtlws_cdd_overlap, (float(f_centre_mhz), float(rate_mhz), float(dm)), (C.c_int,) * 2)
    if rc != 0:
        raise ValueError(last_error())
    return lead, trail


class CddPlan(_PlanBase):
    """rtlws_cdd_plan* of include/rtlws_cdd.h: the channels' tables (complex64 [nchan, N], natural bin order) on the
    engine's device in the kernel's order, the twiddles beside them, the kernel loaded.  ksum 0: voltages; else power
    rows of ksum samples.  eng may be None (as a C caller's NULL engine): open then fails with the library's text."""
    _name, _lib = "cdd", staticmethod(lib)

    def __init__(self, eng, log2_nfft, lead, trail, nchan, ksum, tables):
        tables = _tables(tables)
        self.log2_nfft, self.lead, self.trail, self.nchan, self.ksum = int(log2_nfft), int(lead), int(trail), int(nchan), int(ksum)
        self.n = 1 << self.log2_nfft if 0 <= self.log2_nfft < 31 else 0
        self.hop = self.n - self.lead - self.trail
        assert tables is None or tables.size >= self.nchan * self.n, "fewer table entries than nchan * N"
        self._open(eng, self.log2_nfft, self.lead, self.trail, self.nchan, self.ksum, None if tables is None else _p(tables))

    def samples_needed(self, nseg):
        return self._fn("samples_needed")(self.h, int(nseg))

    def outputs(self, nseg):
        """values of a channel that nseg segments write: nseg * hop voltages, or nseg * hop / ksum power rows"""
        return int(nseg) * (self.hop // self.ksum if self.ksum else self.hop)

    def run(self, d_in, in_stride, nseg, d_out, out_stride, layout="channel", stream=None, check=True):
        """One launch: channel c at d_in + c * in_stride complex elements; d_out what rtlws_cdd.h says for the plan's ksum
        and the layout ("channel" or "time")."""
        return self._call("run", check, self._ptr(d_in), int(in_stride), int(nseg), self._ptr(d_out), int(out_stride), _layout(layout), stream)


def dedisperse(engine, streams, tables, lead, trail, ksum=0, layout="channel", nseg=None, in_stride=None, out_stride=None, fill=None):
    """rtlws_cdd_run: streams complex64 [nchan, nsamples] (with in_stride: [nchan, in_stride], the padding as the caller
    left it), tables complex64 [nchan, N] -> complex64 [nchan, nseg * hop] (ksum 0), or float32 power rows
    [nseg * hop / ksum, nchan] (layout "time") or [nchan, nseg * hop / ksum] ("channel").  nseg None: as many segments as
    the streams hold.  With out_stride the rows are that many elements apart.  With `fill` (a float32) the whole flat
    buffer comes back, GUARD elements (complex ones for voltages) longer than [rows, out_stride], every float of it
    preset to fill, so that a caller sees what the run left untouched."""
    tables = _tables(tables)
    nchan, n = tables.shape
    log2_nfft = max(n.bit_length() - 1, 0)
    assert n == 1 << log2_nfft, "the tables are [nchan, 2^log2_nfft]"
    streams = np.ascontiguousarray(streams, dtype=np.complex64)
    if in_stride is not None:
        streams = streams.reshape(-1, int(in_stride))
    assert streams.ndim == 2 and streams.shape[0] == nchan, "the streams are [nchan, nsamples]"
    width = streams.shape[1]
    plan = CddPlan(engine, log2_nfft, lead, trail, nchan, ksum, tables)
    try:
        if nseg is None:
            nseg = max((width - n) // plan.hop + 1, 0) if width >= n else 0
        nseg = int(nseg)
        assert width >= plan.samples_needed(nseg), "fewer samples than rtlws_cdd_samples_needed"
    except AssertionError:
        plan.close()
        raise
    per, time_major = plan.outputs(nseg), _layout(layout) == TIME_MAJOR
    rows, least = (per, nchan) if time_major else (nchan, per)
    stride = least if out_stride is None else int(out_stride)
    floats = 1 if plan.ksum else 2
    host = engine._preset((rows * max(stride, 0)) * floats, fill, GUARD * floats)
    out, = engine._drive(plan, [streams], [host], lambda i, o: plan.run(i[0], width, nseg, o[0], stride, layout))
    if not plan.ksum:
        out = out.view(np.complex64)
    if fill is not None:
        return out
    return out.reshape(rows, stride)[:, :least]
