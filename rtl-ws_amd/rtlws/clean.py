"""librtlws_clean.so (include/rtlws_clean.h): cleaning of a waterfall per block of rows -- the channels' statistics, the
channels off the block's medians flagged, the kept ones normalised, the zero-DM filter -- bound as a submodule with its own
prototype table (the package's public names, Engine's methods and _Plan's subclasses are pinned, so a
library after the pin lives in a module of its own).  It needs librtlws_hip.so's engine.

  import rtlws, rtlws.clean
  out, keep, stats, nkept = rtlws.clean.clean(engine, rows, 1024, t_mean=6.0, t_sigma=6.0)
  series = engine.dedisp(out, delays)                       # flagged channels are +0.0: no mask needed
  mask = rtlws.clean.union_mask(keep, 0.5)                  # or the one mask rtlws_dedisp_open and rtlws_cand_fold_open take
"""
import ctypes as C
import os

import numpy as np

from . import LIB_DIR, _PlanBase, _load, _outs, _p, _satellite           # noqa: F401  (_load: what _satellite loads through)

CLEAN_LIB = os.path.join(LIB_DIR, "librtlws_clean.so")   # include/rtlws_clean.h
MIN_NCHAN, MAX_NCHAN, MIN_BLOCK, MAX_BLOCK, MAX_NROWS, MAX_CELLS, ZERODM = 4, 4096, 32, 16384, 1 << 24, 1 << 22, 1
GUARD = 8                  # clean(fill=...): preset elements behind every output array
KEEP_FILL = 0xA5           # ... and what the bytes of keep are preset to
WANT = ("keep", "stats", "nkept")

_i, _l, _vp, _ip, _lp, _d = C.c_int, C.c_long, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_long), C.c_double
_PROTOTYPES = {
    "rtlws_clean_supported": [_i, _l],
    "rtlws_clean_geometry": [_i, _l, _l, _ip, _ip, _ip, _lp, _lp, _lp],
    "rtlws_clean_open": ([_vp, _i, _l, _vp, _d, _d, _i], _vp),
    "rtlws_clean_blocks": ([_vp, _l], _l),
    "rtlws_clean_run": [_vp, _vp, _l, _l, _vp, _l, _vp, _vp, _vp, _vp],
    "rtlws_clean_union_mask": [_vp, _l, _i, _d, _vp],
    "rtlws_clean_close": ([_vp], None),
    "rtlws_clean_last_error": ([], C.c_char_p)}
SYMBOLS = list(_PROTOTYPES)


def lib():
    """librtlws_clean.so (include/rtlws_clean.h); it needs librtlws_hip.so's engine."""
    return _satellite(CLEAN_LIB, _PROTOTYPES)


def last_error():
    return lib().rtlws_clean_last_error().decode()


def supported(nchan, block_rows):
    """rtlws_clean_supported.  No GPU needed."""
    return lib().rtlws_clean_supported(int(nchan), int(block_rows))


def geometry(nchan, block_rows, nrows=0):
    """rtlws_clean_geometry: (rc, the three launches' workgroups, threads, LDS bytes -- a tuple of three each --, nblocks,
    the workspace bytes of this run, the blocks a plan's workspace holds).  No GPU needed."""
    return _outs(lib().rtlws_clean_geometry, (int(nchan), int(block_rows), int(nrows)), (C.c_int * 3,) * 3 + (C.c_long,) * 3)


def union_mask(keep, min_share=1.0):
    """rtlws_clean_union_mask: keep uint8 [nblocks, nchan] -> uint8 [nchan], 1 where at least min_share of the blocks keep
    the channel.  No GPU needed."""
    keep = np.ascontiguousarray(keep, dtype=np.uint8)
    assert keep.ndim == 2, "keep is [nblocks, nchan]"
    mask = np.zeros(keep.shape[1], np.uint8)
    if lib().rtlws_clean_union_mask(_p(keep), keep.shape[0], keep.shape[1], float(min_share), _p(mask)) != 0:
        raise ValueError(last_error())
    return mask


class CleanPlan(_PlanBase):
    """rtlws_clean_plan* of include/rtlws_clean.h: the mask (uint8 [nchan] or None) on the engine's device, the workspace
    and the three kernels loaded.  eng may be None (as a C caller's NULL engine): open then fails with the library's text."""
    _name = "clean"
    _lib = staticmethod(lib)

    def __init__(self, eng, nchan, block_rows, mask=None, t_mean=float("inf"), t_sigma=float("inf"), zerodm=True, flags=None):
        mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        self.nchan, self.block_rows = int(nchan), int(block_rows)
        assert mask is None or mask.size >= self.nchan, "fewer mask bytes than nchan"
        self.flags = (ZERODM if zerodm else 0) if flags is None else int(flags)
        self._open(eng, self.nchan, self.block_rows, None if mask is None else _p(mask), float(t_mean), float(t_sigma), self.flags)

    def blocks(self, nrows):
        return self._fn("blocks")(self.h, int(nrows))

    def run(self, d_rows, in_stride, nrows, d_out, out_stride, d_keep=None, d_stats=None, d_nkept=None, stream=None, check=True):
        """Three launches: row j at d_rows + j * in_stride elements, cleaned to d_out + j * out_stride (d_out may be d_rows
        with equal strides); d_keep uint8 [nblocks, nchan], d_stats float32 [nblocks, nchan, 2], d_nkept int32 [nblocks],
        or None."""
        return self._call("run", check, self._ptr(d_rows), int(in_stride), int(nrows), self._ptr(d_out), int(out_stride), self._ptr(d_keep),
                          self._ptr(d_stats), self._ptr(d_nkept), stream)


def clean(engine, rows, block_rows, mask=None, t_mean=float("inf"), t_sigma=float("inf"), zerodm=True, want=WANT, in_stride=None,
          nchan=None, out_stride=None, in_place=False, fill=None):
    """rtlws_clean_run: rows float32 [nrows, nchan] (with in_stride and nchan: [nrows, in_stride], the first nchan values of
    a row its channels, the padding as the caller left it) -> (out float32 [nrows, nchan], keep uint8 [nblocks, nchan],
    stats float32 [nblocks, nchan, 2], nkept int32 [nblocks]); an output that `want` does not name gets a NULL pointer
    and comes back None.  in_place: d_out is d_rows (and out_stride in_stride), and `out` is the rows' buffer as the run
    left it, [nrows, in_stride].  With `fill` (a float32) the four come back as the whole flat buffers, GUARD elements
    longer than the outputs ([nrows, out_stride] for out), every element preset to fill or to its bits (keep: to KEEP_FILL), so that a caller
    sees what the run left untouched; an output that is not wanted comes back as it was preset."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    if in_stride is not None:
        rows = rows.reshape(-1, int(in_stride))
    assert rows.ndim == 2, "the rows are [nrows, nchan]"
    nrows, width = rows.shape
    nchan = width if nchan is None else int(nchan)
    stride = width if in_place else nchan if out_stride is None else int(out_stride)
    plan = CleanPlan(engine, nchan, block_rows, mask, t_mean, t_sigma, zerodm)
    nblocks = max(plan.blocks(nrows), 0)
    hosts = [None if in_place else engine._preset(nrows * stride, fill, GUARD), np.full(nblocks * nchan + (0 if fill is None else GUARD), 0 if fill is None else KEEP_FILL, np.uint8),
             engine._preset(nblocks * nchan * 2, fill, GUARD), engine._preset(nblocks, fill, GUARD, np.int32)]
    wanted = [True] + [name in want for name in WANT]
    if in_place:
        hosts[0] = rows.reshape(-1).copy()
        got = engine._drive(plan, [], hosts, lambda i, o: plan.run(o[0], width, nrows, o[0], width, *[b if w else None for b, w in zip(o[1:], wanted[1:])]))
    else:
        got = engine._drive(plan, [rows], hosts, lambda i, o: plan.run(i[0], width, nrows, o[0], stride, *[b if w else None for b, w in zip(o[1:], wanted[1:])]))
    out, keep, stats, nkept = got
    if fill is not None:
        return out, keep, stats, nkept
    out = out.reshape(nrows, stride)
    return (out if in_place or out_stride is not None else out[:, :nchan], keep.reshape(nblocks, nchan) if wanted[1] else None,
            stats.reshape(nblocks, nchan, 2) if wanted[2] else None, nkept if wanted[3] else None)
