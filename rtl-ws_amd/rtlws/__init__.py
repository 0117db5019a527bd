"""ctypes front end of the product libraries (rtl-ws_amd/lib/*.so).

This is plumbing for tests/, bench.py and __graft_entry__: it loads the C-ABI
declared in include/*.h and nothing else.  There is no CPU implementation
behind it -- if the libraries are missing or no HIP device is usable, calls
fail loudly.

  Engine ............ include/rtlws_hip.h (batch API on device buffers)
  LongPlan .......... include/rtlws_long.h (f64 spectra of 2^14 .. 2^20-point frames)
  AnyLenPlan ........ include/rtlws_anylen.h (f64 spectra of any frame length 2 .. 2^19)
  Engine.fm_audio_blocks[_cu8]  include/rtlws_fm.h (the FM receive chain in one launch)
  DdcPlan, Engine.ddc  include/rtlws_ddc.h (tuned channels from one capture: integer mixer + CIC in one launch)
  DdcFirPlan, Engine.ddcfir  include/rtlws_ddcfir.h (tuned channels with an int16 FIR of up to 256 taps as the channel filter, one launch)
  FmBankPlan, Engine.fm_bank  include/rtlws_fmbank.h (up to 32 FM stations from one capture in one launch)
  FmFirPlan, Engine.fm_fir_bank  include/rtlws_fmfir.h (those stations behind an int16 FIR of up to 256 taps, one launch)
  PfbPlan, Engine.pfb  include/rtlws_pfb.h (polyphase channelizer: all 2^k channels of one capture in one launch)
  PfbSpecPlan, Engine.pfbspec  include/rtlws_pfbspec.h (polyphase spectrometer: K-frame power of all 2^k channels in one launch)
  PfbXcPlan, Engine.pfbxc  include/rtlws_pfbxc.h (polyphase cross-correlator: K-frame powers and cross-spectra of 2-4 captures in one launch)
  PfbBfPlan, Engine.pfbbf, Engine.pfbbf_power  include/rtlws_pfbbf.h (polyphase beamformer: 1-4 weighted beams of 1-8 captures in one launch)
  PfbSkPlan, Engine.pfbsk  include/rtlws_pfbsk.h (polyphase spectrometer with spectral-kurtosis excision: the power over the kept ones of L sub-integrations, one launch)
  DedispPlan, Engine.dedisp  include/rtlws_dedisp.h (incoherent dedispersion of f32 rows: every trial of a delay table in one launch)
  PulsePlan, Engine.pulse  include/rtlws_pulse.h (single-pulse search: boxcar peaks of a table of widths and the moments per segment, one launch)
  FoldPlan, Engine.fold  include/rtlws_fold.h (epoch folding: the profiles of every trial at a table of periods, per sub-integration, one launch)
  PeriodPlan, Engine.period  include/rtlws_period.h (periodicity search: whitened power spectra, harmonic sums and their peaks per segment, every trial in one launch)
  PeriodLongPlan, Engine.periodlong  include/rtlws_periodlong.h (that search for frames of 2^16 .. 2^22 samples: a four-step transform through device memory)
  AccelPlan, Engine.accel_search, Engine.accel_resample  include/rtlws_accel.h (acceleration search: that long-frame search of every series read through a table of quadratic index maps, no resampled copy in memory)
  Spectrum .......... include/spectrum.h      (reference src/spectrum.h:7-17)
  cic_decimate ...... include/resample.h      (reference src/resample.h:14)
  halfband_decimate . include/resample.h      (reference src/resample.h:17)
  RfDecimator ....... include/rf_decimator.h  (reference src/rf_decimator.h:6-21)
"""
import ctypes as C
import os
import subprocess

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_PKG)                       # rtl-ws_amd/
LIB_DIR = os.path.join(ROOT, "lib")
# RTLWS_HIP_LIB selects an experiment build (make variant ...); default: the product library
HIP_LIB = os.environ.get("RTLWS_HIP_LIB") or os.path.join(LIB_DIR, "librtlws_hip.so")
# RTLWS_AMD_LIB: an instrumented build of the C host layer (tests/tools/asan_host_cpu.sh)
AMD_LIB = os.environ.get("RTLWS_AMD_LIB") or os.path.join(LIB_DIR, "librtlws_amd.so")
LONG_LIB = os.path.join(LIB_DIR, "librtlws_long.so")     # include/rtlws_long.h
ANYLEN_LIB = os.path.join(LIB_DIR, "librtlws_anylen.so") # include/rtlws_anylen.h
FM_LIB = os.path.join(LIB_DIR, "librtlws_fm.so")         # include/rtlws_fm.h
DDC_LIB = os.path.join(LIB_DIR, "librtlws_ddc.so")       # include/rtlws_ddc.h
FMBANK_LIB = os.path.join(LIB_DIR, "librtlws_fmbank.so") # include/rtlws_fmbank.h
DDCFIR_LIB = os.path.join(LIB_DIR, "librtlws_ddcfir.so") # include/rtlws_ddcfir.h
FMFIR_LIB = os.path.join(LIB_DIR, "librtlws_fmfir.so")   # include/rtlws_fmfir.h
PFB_LIB = os.path.join(LIB_DIR, "librtlws_pfb.so")       # include/rtlws_pfb.h
PFBSPEC_LIB = os.path.join(LIB_DIR, "librtlws_pfbspec.so")   # include/rtlws_pfbspec.h
PFBXC_LIB = os.path.join(LIB_DIR, "librtlws_pfbxc.so")   # include/rtlws_pfbxc.h
PFBBF_LIB = os.path.join(LIB_DIR, "librtlws_pfbbf.so")   # include/rtlws_pfbbf.h
PFBSK_LIB = os.path.join(LIB_DIR, "librtlws_pfbsk.so")   # include/rtlws_pfbsk.h
DEDISP_LIB = os.path.join(LIB_DIR, "librtlws_dedisp.so") # include/rtlws_dedisp.h
PULSE_LIB = os.path.join(LIB_DIR, "librtlws_pulse.so")   # include/rtlws_pulse.h
FOLD_LIB = os.path.join(LIB_DIR, "librtlws_fold.so")     # include/rtlws_fold.h
PERIOD_LIB = os.path.join(LIB_DIR, "librtlws_period.so") # include/rtlws_period.h
PERIODLONG_LIB = os.path.join(LIB_DIR, "librtlws_periodlong.so")  # include/rtlws_periodlong.h
ACCEL_LIB = os.path.join(LIB_DIR, "librtlws_accel.so")   # include/rtlws_accel.h
CBB_LIB = os.path.join(LIB_DIR, "librtlws_cbb.so")       # include/cbb_main.h
SYNTH_LIB = os.path.join(LIB_DIR, "librtlws_synth.so")   # synthetic rtl_sensor.h + signal_source.h

IN_CU8, IN_CS32, IN_RF32 = 0, 1, 2
WIN_RECT, WIN_HANN = 0, 1
OUT_POWER_SUM, OUT_MEAN_DB, OUT_PAYLOAD_U8 = 0, 1, 2
FLAG_ROWS_F32 = 1          # rtlws_spectra_batch_f64: f64 arithmetic, f32 rows
FLAG_F64 = 2               # rtlws_stream.h: this stream computes in f64

_INPUTS = {"cu8": IN_CU8, "cs32": IN_CS32, "rf32": IN_RF32}
_SAMPLE_BYTES = {"cu8": 2, "cs32": 8, "rf32": 4}
_WINDOWS = {"rect": WIN_RECT, "hann": WIN_HANN, None: WIN_RECT}
_OUTPUTS = {"power_sum": OUT_POWER_SUM, "mean_db": OUT_MEAN_DB, "payload_u8": OUT_PAYLOAD_U8}


def build(jobs=8):
    """Compile every HIP/C source for gfx950 (hipcc cross-compiles without a GPU)."""
    out = subprocess.run(["make", "-C", ROOT, "-j%d" % jobs], capture_output=True, text=True)
    if out.returncode != 0:
        raise RuntimeError("rtl-ws_amd build failed:\n" + out.stdout[-4000:] + out.stderr[-4000:])


class SpectraDesc(C.Structure):
    _fields_ = [("n_fft", C.c_int), ("k_avg", C.c_int), ("input", C.c_int), ("window", C.c_int),
                ("output", C.c_int), ("cic_r", C.c_int), ("gain_db", C.c_int), ("flags", C.c_int)]


class CmplxS32(C.Structure):
    _fields_ = [("re", C.c_int32), ("im", C.c_int32)]


class TopoInfo(C.Structure):
    """rtlws_topo_info (include/rtlws_topo.h)"""
    _fields_ = [("device", C.c_int), ("bus_id", C.c_char * 32), ("numa_node", C.c_int), ("ncpus", C.c_int),
                ("cpulist", C.c_char * 512)]


class CicDelayLine(C.Structure):
    _fields_ = [("integrator_prev_out", CmplxS32), ("comb_prev_in", CmplxS32)]


# every symbol include/*.h declares, by library (tests check the exports).  A library with a prototype table below lists
# its table's functions: X_SYMBOLS = list(_X_PROTOTYPES).
AUDIO_SYMBOLS = ["audio_init", "audio_new_audio_available", "audio_get_audio_payload",
                 "audio_fm_demodulator", "audio_close"]
STREAM_SYMBOLS = ["rtlws_stream_open", "rtlws_stream_open_q", "rtlws_stream_push", "rtlws_stream_flush",
                  "rtlws_stream_get_stats", "rtlws_stream_close", "rtlws_stream_device_for", "rtlws_stream_topology"]
AMD_SYMBOLS = [
    "spectrum_alloc", "spectrum_add_cmplx_u8", "spectrum_add_cmplx_s32", "spectrum_add_real_f32",
    "spectrum_free", "cic_decimate", "halfband_decimate", "rf_decimator_alloc",
    "rf_decimator_add_callback", "rf_decimator_set_parameters", "rf_decimator_decimate_cmplx_u8",
    "rf_decimator_remove_callbacks", "rf_decimator_free",
]

# include/rtlws_multi.h: one device-resident batch sharded over the devices of a node (librtlws_amd.so)
MULTI_SYMBOLS = ["rtlws_multi_partition", "rtlws_multi_open", "rtlws_multi_shards", "rtlws_multi_frames",
                 "rtlws_multi_frame_bytes", "rtlws_multi_row_bytes", "rtlws_multi_upload", "rtlws_multi_run",
                 "rtlws_multi_download", "rtlws_multi_close", "rtlws_multi_error", "rtlws_multi_shard_topology"]
# include/rtlws_topo.h (librtlws_amd.so)
TOPO_SYMBOLS = ["rtlws_topo_describe", "rtlws_topo_parse_cpulist", "rtlws_topo_pin_thread"]

# include/rtlws_host.h: sticky failure record of the void entry points (librtlws_amd.so)
HOST_SYMBOLS = ["rtlws_host_error", "rtlws_host_error_count", "rtlws_host_error_clear", "rtlws_host_fail",
                "rtlws_host_device"]

CBB_SYMBOLS = ["cbb_init", "cbb_rf_decimator", "cbb_get_rtl_dev", "cbb_new_spectrum_available",
               "cbb_get_spectrum_payload", "cbb_close",
               "rtlws_cbb_published_frames", "rtlws_cbb_samples_seen"]      # include/rtlws_cbb.h
SYNTH_SYMBOLS = ["rtl_init", "rtl_set_frequency", "rtl_set_sample_rate", "rtl_set_gain", "rtl_freq",
                 "rtl_sample_rate", "rtl_gain", "rtl_read_async", "rtl_cancel", "rtl_close",
                 "signal_source_start", "signal_source_add_callback",
                 "signal_source_remove_callbacks", "signal_source_stop"]

_loaded = {}              # path -> a library with a prototype table, loaded (_load)
_amd = None
_cbb = None


_tried_build = False


def _need(path):
    """The product libraries are built in-tree (make -C rtl-ws_amd).  If one is
    missing, build once (hipcc/gcc are on every box of this image); if it is
    still missing, fail loudly -- there is no CPU implementation to fall back to."""
    global _tried_build
    if not os.path.exists(path) and not _tried_build and not os.environ.get("RTLWS_HIP_LIB"):
        _tried_build = True
        build()
    if not os.path.exists(path):
        raise RuntimeError(
            "%s is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; "
            "g.build()' or make -C rtl-ws_amd). There is no CPU fallback." % path)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the libraries with a prototype table: one loader, one out-parameter call ----

def _load(path, prototypes):
    """The library at path, loaded once (RTLD_GLOBAL; the build first where it is missing), with its prototypes from a
    table name -> argtypes (an int comes back) or (argtypes, restype)."""
    L = _loaded.get(path)
    if L is None:
        _need(path)
        L = C.CDLL(path, mode=C.RTLD_GLOBAL)
        for name, proto in prototypes.items():
            f = getattr(L, name)
            if isinstance(proto, tuple):
                f.argtypes, f.restype = proto
            else:
                f.argtypes = proto
        _loaded[path] = L
    return L


def _satellite(path, prototypes):
    """A library of its own on top of librtlws_hip.so's engine (include/rtlws_<name>.h): librtlws_hip.so first."""
    hip_lib()
    return _load(path, prototypes)


def _library(name, prototypes):
    """(x_lib, x_last_error) of the satellite library `name`: its loader over X_LIB and its table, and the reader of
    rtlws_<name>_last_error."""
    path = globals()[name.upper() + "_LIB"]

    def lib():
        return _satellite(path, prototypes)

    def last_error():
        return getattr(lib(), "rtlws_%s_last_error" % name)().decode()

    lib.__name__ = lib.__qualname__ = name + "_lib"
    lib.__doc__ = "librtlws_%s.so (include/rtlws_%s.h); it needs librtlws_hip.so's engine." % (name, name)
    last_error.__name__ = last_error.__qualname__ = name + "_last_error"
    return lib, last_error


def _outs(fn, args, types):
    """fn(*args, *outs) -> (rc, *values): behind args one fresh zero-initialised object of each of `types` by reference
    (a ctypes scalar type, whose value comes back; or an array type, passed as it is, which comes back as a tuple)."""
    outs = [t() for t in types]
    rc = fn(*args, *[o if isinstance(o, C.Array) else C.byref(o) for o in outs])
    return (rc,) + tuple(tuple(o) if isinstance(o, C.Array) else o.value for o in outs)


_i, _l, _vp, _ip, _str, _sz = C.c_int, C.c_long, C.c_void_p, C.POINTER(C.c_int), C.c_char_p, C.c_size_t
_desc, _vpp = C.POINTER(SpectraDesc), C.POINTER(C.c_void_p)
_GRID = (C.c_int,) * 4    # what most rtlws_*_grid give: workgroups, threads, LDS bytes and the library's own fourth

# ---- include/rtlws_hip.h ----
_HIP_PROTOTYPES = {
    "rtlws_device_count": [], "rtlws_device_pci_bus_id": [_i, _str, _i], "rtlws_engine_create": ([_i], _vp),
    "rtlws_engine_destroy": [_vp], "rtlws_engine_device": [_vp], "rtlws_engine_stream": ([_vp], _vp),
    "rtlws_engine_prepare": [_vp, _i], "rtlws_engine_prepare_f64": [_vp, _i], "rtlws_engine_set_option": [_vp, _str, _i],
    "rtlws_engine_get_option": [_vp, _str], "rtlws_last_error": ([], _str), "rtlws_dev_alloc": ([_vp, _sz], _vp),
    "rtlws_dev_free": [_vp, _vp], "rtlws_pinned_alloc": ([_sz], _vp), "rtlws_pinned_free": [_vp],
    "rtlws_copy_h2d": [_vp, _vp, _vp, _sz, _vp], "rtlws_copy_d2h": [_vp, _vp, _vp, _sz, _vp],
    "rtlws_copy_d2d": [_vp, _vp, _vp, _sz, _vp], "rtlws_memset_dev": [_vp, _vp, _i, _sz, _vp], "rtlws_stream_sync": [_vp, _vp],
    "rtlws_event_create": ([], _vp), "rtlws_event_create_blocking": ([], _vp), "rtlws_event_destroy": [_vp],
    "rtlws_event_record": [_vp, _vp, _vp], "rtlws_event_elapsed_ms": ([_vp, _vp], C.c_float), "rtlws_event_sync": [_vp],
    "rtlws_queue_create": ([_vp], _vp), "rtlws_queue_destroy": [_vp, _vp], "rtlws_queue_wait_event": [_vp, _vp, _vp],
    "rtlws_spectra_batch": [_vp, _desc, _vp, _l, _vp, _vp], "rtlws_spectra_batch_f64": [_vp, _desc, _vp, _l, _vp, _vp],
    "rtlws_spectra_kernel_kind": [_desc], "rtlws_spectra_grid": [_vp, _desc, _l, _ip, _ip, _ip],
    "rtlws_payload_from_sums": [_vp, _vp, _i, _i, _i, _vp, _vp], "rtlws_payload_from_sums_f64": [_vp, _vp, _i, _i, _i, _vp, _vp],
    "rtlws_welch_accumulate_f64": [_vp, _vp, _vp, _i, _l, _vp, _vp], "rtlws_welch_finish_f64": [_vp, _vp, _i, _l, _vp, _vp],
    "rtlws_cic_block_sums": [_vp, _i, _vp, _l, _vp, _vp], "rtlws_halfband": [_vp, _vp, _vp, _l, _vp],
    "rtlws_fm_demod": [_vp, _vp, _l, _vp, _vp, _vp, _vp], "rtlws_clock_stamp": [_vp, _vp, _i, _vp]}
HIP_SYMBOLS = list(_HIP_PROTOTYPES)


def hip_lib():
    return _load(HIP_LIB, _HIP_PROTOTYPES)


def last_error():
    return hip_lib().rtlws_last_error().decode()


def device_count():
    return hip_lib().rtlws_device_count()


# ---- include/rtlws_long.h ----
_LONG_PROTOTYPES = {
    "rtlws_long_supported": [_desc], "rtlws_long_open": ([_vp, _desc, _l], _vp),
    "rtlws_long_workspace_bytes": ([_vp], _sz), "rtlws_long_run": [_vp, _vp, _l, _vp, _vp],
    "rtlws_long_close": ([_vp], None), "rtlws_long_last_error": ([], _str)}
LONG_SYMBOLS = list(_LONG_PROTOTYPES)
long_lib, long_last_error = _library("long", _LONG_PROTOTYPES)


def long_supported(desc):
    return long_lib().rtlws_long_supported(C.byref(desc))


# ---- include/rtlws_anylen.h ----
_ANYLEN_PROTOTYPES = {
    "rtlws_anylen_supported": [_desc], "rtlws_anylen_conv_log2": [_desc], "rtlws_anylen_open": ([_vp, _desc, _l], _vp),
    "rtlws_anylen_workspace_bytes": ([_vp], _sz), "rtlws_anylen_run": [_vp, _vp, _l, _vp, _vp],
    "rtlws_anylen_close": ([_vp], None), "rtlws_anylen_last_error": ([], _str)}
ANYLEN_SYMBOLS = list(_ANYLEN_PROTOTYPES)
anylen_lib, anylen_last_error = _library("anylen", _ANYLEN_PROTOTYPES)


def anylen_supported(desc):
    return anylen_lib().rtlws_anylen_supported(C.byref(desc))


def anylen_conv_log2(desc):
    """m of the convolution length 2^m the descriptor runs at, -1 if it is not served."""
    return anylen_lib().rtlws_anylen_conv_log2(C.byref(desc))


# ---- include/rtlws_fm.h ----
FM_STATE_FLOATS = 21       # rtlws_fm.h: phase carry, delay line 1, delay line 2
_FM_PROTOTYPES = {
    "rtlws_fm_supported": [_i, _l, _i], "rtlws_fm_grid": [_i, _l, _i, _ip, _ip, _ip, _ip], "rtlws_fm_prepare": [_vp],
    "rtlws_fm_audio_blocks": [_vp, _vp, _i, _l, _vp, _vp, _i, _vp, _vp],
    "rtlws_fm_audio_blocks_cu8": [_vp, _i, _vp, _i, _l, _vp, _vp, _i, _vp, _vp, _vp], "rtlws_fm_last_error": ([], _str)}
FM_SYMBOLS = list(_FM_PROTOTYPES)
fm_lib, fm_last_error = _library("fm", _FM_PROTOTYPES)


def fm_supported(block_len, nblocks=1, cic_r=0):
    return fm_lib().rtlws_fm_supported(int(block_len), int(nblocks), int(cic_r))


def fm_grid(block_len, nblocks, cic_r=0):
    """rtlws_fm_grid: (rc, workgroups, threads, LDS bytes, audio samples per tile).  No GPU needed."""
    return _outs(fm_lib().rtlws_fm_grid, (int(block_len), int(nblocks), int(cic_r)), _GRID)


# ---- include/rtlws_ddc.h ----
DDC_LOG2_PERIOD = 16       # rtlws_ddc.h: the phase period P = 2^16
DDC_MAX_CHANNELS = 32
_DDC_PROTOTYPES = {
    "rtlws_ddc_supported": [_i, _i], "rtlws_ddc_table": [_vp], "rtlws_ddc_tuning_word": [C.c_double, C.c_double, _ip],
    "rtlws_ddc_open": ([_vp], _vp), "rtlws_ddc_grid": [_i, _i, _l, _ip, _ip, _ip, _ip],
    "rtlws_ddc_run": [_vp, _i, _vp, _l, _l, _i, _vp, _vp, _l, _vp], "rtlws_ddc_close": ([_vp], None),
    "rtlws_ddc_last_error": ([], _str)}
DDC_SYMBOLS = list(_DDC_PROTOTYPES)
ddc_lib, ddc_last_error = _library("ddc", _DDC_PROTOTYPES)


def ddc_supported(cic_r, nchannels=1):
    return ddc_lib().rtlws_ddc_supported(int(cic_r), int(nchannels))


def ddc_table():
    """rtlws_ddc_table: the phasor table as the library builds it, int16 [P, 2] = (cos, sin).  No GPU needed."""
    t = np.empty((1 << DDC_LOG2_PERIOD, 2), dtype=np.int16)
    rc = ddc_lib().rtlws_ddc_table(_p(t))
    if rc != 0:
        raise RuntimeError("rtlws_ddc_table failed (rc=%d): %s" % (rc, ddc_last_error()))
    return t


def ddc_tuning_word(offset_hz, sample_rate_hz):
    """rtlws_ddc_tuning_word: (rc, word).  No GPU needed."""
    return _outs(ddc_lib().rtlws_ddc_tuning_word, (float(offset_hz), float(sample_rate_hz)), (C.c_int,))


def ddc_grid(cic_r, nchannels, dec_len):
    """rtlws_ddc_grid: (rc, workgroups, threads, LDS bytes, decimated samples per tile).  No GPU needed."""
    return _outs(ddc_lib().rtlws_ddc_grid, (int(cic_r), int(nchannels), int(dec_len)), _GRID)


# ---- include/rtlws_ddcfir.h ----
DDCFIR_MAX_TAPS, DDCFIR_MAX_TAP, DDCFIR_MAX_SHIFT = 256, 32639, 30       # rtlws_ddcfir.h
_DDCFIR_PROTOTYPES = {
    "rtlws_ddcfir_supported": [_i, _i, _i], "rtlws_ddcfir_samples_needed": ([_i, _i, _l], _l),
    "rtlws_ddcfir_grid": [_i, _i, _i, _l, _ip, _ip, _ip, _ip], "rtlws_ddcfir_design": [_i, _i, _vp],
    "rtlws_ddcfir_bound": [_i, _vp, _i, C.POINTER(C.c_double)], "rtlws_ddcfir_open": ([_vp, _i, _i, _vp], _vp),
    "rtlws_ddcfir_run": [_vp, _vp, _l, _l, _i, _vp, _i, _vp, _l, _vp], "rtlws_ddcfir_close": ([_vp], None),
    "rtlws_ddcfir_last_error": ([], _str)}
DDCFIR_SYMBOLS = list(_DDCFIR_PROTOTYPES)
ddcfir_lib, ddcfir_last_error = _library("ddcfir", _DDCFIR_PROTOTYPES)


def ddcfir_supported(decim, ntaps, nchannels=1):
    return ddcfir_lib().rtlws_ddcfir_supported(int(decim), int(ntaps), int(nchannels))


def ddcfir_samples_needed(decim, ntaps, dec_len):
    """rtlws_ddcfir_samples_needed: (dec_len - 1) * decim + ntaps, or -1.  No GPU needed."""
    return ddcfir_lib().rtlws_ddcfir_samples_needed(int(decim), int(ntaps), int(dec_len))


def ddcfir_grid(decim, ntaps, nchannels, dec_len):
    """rtlws_ddcfir_grid: (rc, workgroups, threads, LDS bytes, decimated samples per tile).  No GPU needed."""
    return _outs(ddcfir_lib().rtlws_ddcfir_grid, (int(decim), int(ntaps), int(nchannels), int(dec_len)), _GRID)


def ddcfir_design(decim, ntaps):
    """rtlws_ddcfir_design: the Hamming-windowed sinc for decimation by decim, int16 [ntaps].  No GPU needed."""
    taps = np.zeros(max(int(ntaps), 1), dtype=np.int16)
    rc = ddcfir_lib().rtlws_ddcfir_design(int(decim), int(ntaps), _p(taps))
    if rc != 0:
        raise RuntimeError("rtlws_ddcfir_design failed (rc=%d): %s" % (rc, ddcfir_last_error()))
    return taps[:ntaps]


def ddcfir_bound(taps, out_shift):
    """rtlws_ddcfir_bound: how far a component lies from the ideal mixer and filter at most.  No GPU needed."""
    taps = np.ascontiguousarray(taps, dtype=np.int16)
    rc, bound = _outs(ddcfir_lib().rtlws_ddcfir_bound, (taps.size, _p(taps), int(out_shift)), (C.c_double,))
    if rc != 0:
        raise RuntimeError("rtlws_ddcfir_bound failed (rc=%d): %s" % (rc, ddcfir_last_error()))
    return bound


# ---- include/rtlws_fmbank.h ----
FMBANK_MAX_CHANNELS = 32
_FMBANK_PROTOTYPES = {
    "rtlws_fmbank_supported": [_i, _i, _i, _l], "rtlws_fmbank_grid": [_i, _i, _i, _l, _ip, _ip, _ip, _ip],
    "rtlws_fmbank_open": ([_vp], _vp), "rtlws_fmbank_run": [_vp, _i, _vp, _i, _l, _l, _i, _vp, _vp, _vp, _vp, _l, _vp],
    "rtlws_fmbank_close": ([_vp], None), "rtlws_fmbank_last_error": ([], _str)}
FMBANK_SYMBOLS = list(_FMBANK_PROTOTYPES)
fmbank_lib, fmbank_last_error = _library("fmbank", _FMBANK_PROTOTYPES)


def fmbank_supported(cic_r, nchannels=1, block_len=20, nblocks=1):
    return fmbank_lib().rtlws_fmbank_supported(int(cic_r), int(nchannels), int(block_len), int(nblocks))


def fmbank_grid(cic_r, nchannels, block_len, nblocks):
    """rtlws_fmbank_grid: (rc, workgroups, threads, LDS bytes, audio samples per tile).  No GPU needed."""
    return _outs(fmbank_lib().rtlws_fmbank_grid, (int(cic_r), int(nchannels), int(block_len), int(nblocks)), _GRID)


# ---- include/rtlws_fmfir.h ----
FMFIR_MAX_CHANNELS = 32                                                   # rtlws_fmfir.h
_FMFIR_PROTOTYPES = {
    "rtlws_fmfir_supported": [_i, _i, _i, _i, _l], "rtlws_fmfir_samples_needed": ([_i, _i, _i, _l], _l),
    "rtlws_fmfir_grid": [_i, _i, _i, _i, _l, _ip, _ip, _ip, _ip], "rtlws_fmfir_open": ([_vp, _i, _i, _vp], _vp),
    "rtlws_fmfir_run": [_vp, _vp, _i, _l, _l, _i, _vp, _i, _vp, _vp, _vp, _l, _vp], "rtlws_fmfir_close": ([_vp], None),
    "rtlws_fmfir_last_error": ([], _str)}
FMFIR_SYMBOLS = list(_FMFIR_PROTOTYPES)
fmfir_lib, fmfir_last_error = _library("fmfir", _FMFIR_PROTOTYPES)


def fmfir_supported(decim, ntaps, nchannels=1, block_len=20, nblocks=1):
    return fmfir_lib().rtlws_fmfir_supported(int(decim), int(ntaps), int(nchannels), int(block_len), int(nblocks))


def fmfir_samples_needed(decim, ntaps, block_len, nblocks):
    """rtlws_fmfir_samples_needed: (nblocks * block_len - 1) * decim + ntaps, 0 without blocks, or -1.  No GPU needed."""
    return fmfir_lib().rtlws_fmfir_samples_needed(int(decim), int(ntaps), int(block_len), int(nblocks))


def fmfir_grid(decim, ntaps, nchannels, block_len, nblocks):
    """rtlws_fmfir_grid: (rc, workgroups, threads, LDS bytes, audio samples per tile).  No GPU needed."""
    return _outs(fmfir_lib().rtlws_fmfir_grid, (int(decim), int(ntaps), int(nchannels), int(block_len), int(nblocks)), _GRID)


def amd_lib():
    global _amd
    if _amd is None:
        hip_lib()
        long_lib()
        anylen_lib()
        fm_lib()
        _need(AMD_LIB)
        L = C.CDLL(AMD_LIB)
        vp, i = C.c_void_p, C.c_int
        L.spectrum_alloc.argtypes = [i]
        L.spectrum_alloc.restype = vp
        for n in ("spectrum_add_cmplx_u8", "spectrum_add_cmplx_s32", "spectrum_add_real_f32"):
            f = getattr(L, n)
            f.argtypes = [vp, vp, vp, i]
            f.restype = i
        L.spectrum_free.argtypes = [vp]
        L.cic_decimate.argtypes = [i, vp, i, vp, i, C.POINTER(CicDelayLine)]
        L.cic_decimate.restype = i
        L.halfband_decimate.argtypes = [vp, vp, i, vp]
        L.halfband_decimate.restype = None
        L.rf_decimator_alloc.restype = vp
        L.rf_decimator_add_callback.argtypes = [vp, vp]
        L.rf_decimator_set_parameters.argtypes = [vp, C.c_double, i]
        L.rf_decimator_set_parameters.restype = i
        L.rf_decimator_decimate_cmplx_u8.argtypes = [vp, vp, i]
        L.rf_decimator_decimate_cmplx_u8.restype = i
        L.rf_decimator_remove_callbacks.argtypes = [vp]
        L.rf_decimator_free.argtypes = [vp]
        lp = C.POINTER(C.c_long)
        L.rtlws_multi_partition.argtypes = [C.c_long, i, i, i, lp, lp]
        L.rtlws_multi_open.argtypes = [i, C.POINTER(i), C.POINTER(SpectraDesc), C.c_long, i]
        L.rtlws_multi_open.restype = vp
        L.rtlws_multi_shards.argtypes = [vp]
        L.rtlws_multi_frames.argtypes = [vp]
        L.rtlws_multi_frames.restype = C.c_long
        L.rtlws_multi_frame_bytes.argtypes = [vp]
        L.rtlws_multi_frame_bytes.restype = C.c_size_t
        L.rtlws_multi_row_bytes.argtypes = [vp]
        L.rtlws_multi_row_bytes.restype = C.c_size_t
        L.rtlws_multi_upload.argtypes = [vp, vp]
        L.rtlws_multi_run.argtypes = [vp, i, vp, C.POINTER(C.c_double)]
        L.rtlws_multi_download.argtypes = [vp, vp]
        L.rtlws_multi_close.argtypes = [vp]
        L.rtlws_multi_error.argtypes = [vp]
        L.rtlws_multi_error.restype = C.c_char_p
        L.rtlws_multi_shard_topology.argtypes = [vp, i, C.POINTER(TopoInfo), C.POINTER(i)]
        L.rtlws_topo_describe.argtypes = [i, C.c_char_p, C.c_char_p, C.POINTER(TopoInfo)]
        L.rtlws_topo_parse_cpulist.argtypes = [C.c_char_p, vp, i]
        L.rtlws_topo_pin_thread.argtypes = [C.POINTER(TopoInfo)]
        L.rtlws_host_error.restype = C.c_char_p
        L.rtlws_host_error_count.restype = C.c_long
        L.rtlws_host_error_clear.restype = None
        _amd = L
    return _amd


# ---- include/rtlws_pfb.h ----
PFB_CHANNEL_MAJOR, PFB_TIME_MAJOR = 0, 1       # rtlws_pfb.h: the output layouts
_PFB_LAYOUTS = {"channel": PFB_CHANNEL_MAJOR, "time": PFB_TIME_MAJOR}
_PFB_PROTOTYPES = {
    "rtlws_pfb_supported": [_i, _i, _i], "rtlws_pfb_design": [_i, _i, _vp], "rtlws_pfb_twiddles": [_i, _vp],
    "rtlws_pfb_samples_needed": ([_i, _i, _i, _l], _l), "rtlws_pfb_grid": [_i, _i, _i, _l, _ip, _ip, _ip, _ip],
    "rtlws_pfb_open": ([_vp, _i, _i, _vp], _vp), "rtlws_pfb_run": [_vp, _vp, _l, _i, _l, _i, _vp, _l, _vp],
    "rtlws_pfb_close": ([_vp], None), "rtlws_pfb_last_error": ([], _str)}
PFB_SYMBOLS = list(_PFB_PROTOTYPES)
pfb_lib, pfb_last_error = _library("pfb", _PFB_PROTOTYPES)


def pfb_supported(log2_channels, taps_per_branch, hop=None):
    """rtlws_pfb_supported; hop None: M.  No GPU needed."""
    hop = (1 << log2_channels if 0 <= log2_channels < 31 else 0) if hop is None else hop
    return pfb_lib().rtlws_pfb_supported(int(log2_channels), int(taps_per_branch), int(hop))


def pfb_design(log2_channels, taps_per_branch):
    """rtlws_pfb_design: the Hamming-windowed sinc prototype, int16 [T * M].  No GPU needed."""
    if pfb_supported(log2_channels, taps_per_branch) != 1:
        raise RuntimeError("rtlws_pfb_design: %s" % pfb_last_error())
    t = np.empty(int(taps_per_branch) << int(log2_channels), dtype=np.int16)
    rc = pfb_lib().rtlws_pfb_design(int(log2_channels), int(taps_per_branch), _p(t))
    if rc != 0:
        raise RuntimeError("rtlws_pfb_design failed (rc=%d): %s" % (rc, pfb_last_error()))
    return t


def pfb_twiddles(log2_channels):
    """rtlws_pfb_twiddles: e^(-2 pi i j / M) as the library builds it, float32 [M, 2].  No GPU needed."""
    if pfb_supported(log2_channels, 1) != 1:
        raise RuntimeError("rtlws_pfb_twiddles: %s" % pfb_last_error())
    t = np.empty((1 << int(log2_channels), 2), dtype=np.float32)
    rc = pfb_lib().rtlws_pfb_twiddles(int(log2_channels), _p(t))
    if rc != 0:
        raise RuntimeError("rtlws_pfb_twiddles failed (rc=%d): %s" % (rc, pfb_last_error()))
    return t


def pfb_samples_needed(log2_channels, taps_per_branch, hop, nframes):
    """rtlws_pfb_samples_needed: (nframes - 1) hop + T M, or -1.  No GPU needed."""
    return pfb_lib().rtlws_pfb_samples_needed(int(log2_channels), int(taps_per_branch), int(hop), int(nframes))


def pfb_grid(log2_channels, taps_per_branch, hop, nframes):
    """rtlws_pfb_grid: (rc, workgroups, threads, LDS bytes, frames per tile).  No GPU needed."""
    return _outs(pfb_lib().rtlws_pfb_grid, (int(log2_channels), int(taps_per_branch), int(hop), int(nframes)), _GRID)


# ---- include/rtlws_pfbspec.h ----
PFBSPEC_MAX_K_AVG = 65536
# rtlws_pfbspec.h's output kinds are enum rtlws_output's values
_PFBSPEC_OUTPUTS = {"power": OUT_POWER_SUM, "db": OUT_MEAN_DB, "payload": OUT_PAYLOAD_U8}
_PFBSPEC_OUTPUTS.update(_OUTPUTS)
_PFBSPEC_PROTOTYPES = {
    "rtlws_pfbspec_supported": [_i, _i, _i, _i, _i], "rtlws_pfbspec_samples_needed": ([_i, _i, _i, _i, _l], _l),
    "rtlws_pfbspec_grid": [_i, _i, _i, _i, _l, _ip, _ip, _ip, _ip], "rtlws_pfbspec_open": ([_vp, _i, _i, _vp], _vp),
    "rtlws_pfbspec_run": [_vp, _vp, _l, _i, _i, _i, _i, C.c_float, _vp, _l, _vp], "rtlws_pfbspec_close": ([_vp], None),
    "rtlws_pfbspec_last_error": ([], _str)}
PFBSPEC_SYMBOLS = list(_PFBSPEC_PROTOTYPES)
pfbspec_lib, pfbspec_last_error = _library("pfbspec", _PFBSPEC_PROTOTYPES)


def pfbspec_supported(log2_channels, taps_per_branch, hop, k_avg, output="power"):
    """rtlws_pfbspec_supported.  No GPU needed."""
    return pfbspec_lib().rtlws_pfbspec_supported(int(log2_channels), int(taps_per_branch), int(hop), int(k_avg),
                                                 int(_PFBSPEC_OUTPUTS.get(output, output)))


def pfbspec_samples_needed(log2_channels, taps_per_branch, hop, k_avg, nspectra):
    """rtlws_pfbspec_samples_needed: (nspectra K - 1) hop + T M, or -1.  No GPU needed."""
    return pfbspec_lib().rtlws_pfbspec_samples_needed(int(log2_channels), int(taps_per_branch), int(hop), int(k_avg),
                                                      int(nspectra))


def pfbspec_grid(log2_channels, taps_per_branch, hop, k_avg, nspectra):
    """rtlws_pfbspec_grid: (rc, workgroups, threads, LDS bytes, spectra per workgroup).  No GPU needed."""
    return _outs(pfbspec_lib().rtlws_pfbspec_grid,
                 (int(log2_channels), int(taps_per_branch), int(hop), int(k_avg), int(nspectra)), _GRID)


# ---- include/rtlws_pfbxc.h ----
PFBXC_MAX_K_AVG = 65536
PFBXC_MIN_INPUTS, PFBXC_MAX_INPUTS = 2, 4
_PFBXC_PROTOTYPES = {
    "rtlws_pfbxc_supported": [_i, _i, _i, _i, _i], "rtlws_pfbxc_samples_needed": ([_i, _i, _i, _i, _l], _l),
    "rtlws_pfbxc_pair_index": [_i, _i, _i], "rtlws_pfbxc_grid": [_i, _i, _i, _i, _i, _l, _ip, _ip, _ip, _ip],
    "rtlws_pfbxc_open": ([_vp, _i, _i, _vp, _i], _vp), "rtlws_pfbxc_run": [_vp, _vpp, _l, _i, _i, _i, _vp, _l, _vp, _l, _vp],
    "rtlws_pfbxc_close": ([_vp], None), "rtlws_pfbxc_last_error": ([], _str)}
PFBXC_SYMBOLS = list(_PFBXC_PROTOTYPES)
pfbxc_lib, pfbxc_last_error = _library("pfbxc", _PFBXC_PROTOTYPES)


def pfbxc_supported(log2_channels, taps_per_branch, hop, k_avg, ninputs=2):
    """rtlws_pfbxc_supported.  No GPU needed."""
    return pfbxc_lib().rtlws_pfbxc_supported(int(log2_channels), int(taps_per_branch), int(hop), int(k_avg), int(ninputs))


def pfbxc_samples_needed(log2_channels, taps_per_branch, hop, k_avg, nspectra):
    """rtlws_pfbxc_samples_needed: (nspectra K - 1) hop + T M per capture, or -1.  No GPU needed."""
    return pfbxc_lib().rtlws_pfbxc_samples_needed(int(log2_channels), int(taps_per_branch), int(hop), int(k_avg),
                                                  int(nspectra))


def pfbxc_pair_index(ninputs, a, b):
    """rtlws_pfbxc_pair_index: the row of the pair a < b among a spectrum's cross rows, or -1.  No GPU needed."""
    return pfbxc_lib().rtlws_pfbxc_pair_index(int(ninputs), int(a), int(b))


def pfbxc_grid(log2_channels, taps_per_branch, hop, k_avg, ninputs, nspectra):
    """rtlws_pfbxc_grid: (rc, workgroups, threads, LDS bytes, spectra per workgroup).  No GPU needed."""
    return _outs(pfbxc_lib().rtlws_pfbxc_grid,
                 (int(log2_channels), int(taps_per_branch), int(hop), int(k_avg), int(ninputs), int(nspectra)), _GRID)


# ---- include/rtlws_pfbbf.h ----
PFBBF_MAX_K_AVG = 65536
PFBBF_MIN_INPUTS, PFBBF_MAX_INPUTS = 1, 8
PFBBF_MIN_BEAMS, PFBBF_MAX_BEAMS = 1, 4
_PFBBF_PROTOTYPES = {
    "rtlws_pfbbf_supported": [_i, _i, _i, _i, _i], "rtlws_pfbbf_samples_needed": ([_i, _i, _i, _i, _l], _l),
    "rtlws_pfbbf_grid": [_i, _i, _i, _i, _l, _ip, _ip, _ip, _ip], "rtlws_pfbbf_open": ([_vp, _i, _i, _vp, _i, _i], _vp),
    "rtlws_pfbbf_run": [_vp, _vpp, _i, _vp, _i, _l, _i, _l, _i, _vp, _l, _l, _vp],
    "rtlws_pfbbf_power": [_vp, _vpp, _i, _vp, _i, _l, _i, _i, _i, _vp, _l, _vp], "rtlws_pfbbf_close": ([_vp], None),
    "rtlws_pfbbf_last_error": ([], _str)}
PFBBF_SYMBOLS = list(_PFBBF_PROTOTYPES)
pfbbf_lib, pfbbf_last_error = _library("pfbbf", _PFBBF_PROTOTYPES)


def pfbbf_supported(log2_channels, taps_per_branch, hop, ninputs=1, nbeams=1):
    """rtlws_pfbbf_supported.  No GPU needed."""
    return pfbbf_lib().rtlws_pfbbf_supported(int(log2_channels), int(taps_per_branch), int(hop), int(ninputs), int(nbeams))


def pfbbf_samples_needed(log2_channels, taps_per_branch, hop, k_avg, count):
    """rtlws_pfbbf_samples_needed per capture: k_avg 0 (voltage mode) (count - 1) hop + T M for count frames, else
    (count K - 1) hop + T M for count spectra; or -1.  No GPU needed."""
    return pfbbf_lib().rtlws_pfbbf_samples_needed(int(log2_channels), int(taps_per_branch), int(hop), int(k_avg), int(count))


def pfbbf_grid(log2_channels, taps_per_branch, hop, k_avg, count):
    """rtlws_pfbbf_grid: (rc, workgroups, threads, LDS bytes, frames (k_avg 0) or spectra per workgroup).  No GPU needed."""
    return _outs(pfbbf_lib().rtlws_pfbbf_grid,
                 (int(log2_channels), int(taps_per_branch), int(hop), int(k_avg), int(count)), _GRID)


# ---- include/rtlws_pfbsk.h ----
PFBSK_MAX_K_AVG, PFBSK_MAX_NSUB = 65536, 65535
_fp = C.POINTER(C.c_float)
_PFBSK_PROTOTYPES = {
    "rtlws_pfbsk_supported": [_i, _i, _i, _i, _i, _i], "rtlws_pfbsk_samples_needed": ([_i, _i, _i, _i, _i, _l], _l),
    "rtlws_pfbsk_grid": [_i, _i, _i, _i, _i, _l, _ip, _ip, _ip, _ip], "rtlws_pfbsk_power_scale": ([_i, _i, _vp], C.c_float),
    "rtlws_pfbsk_bounds": [_i, C.c_double, C.c_double, _fp, _fp], "rtlws_pfbsk_open": ([_vp, _i, _i, _vp], _vp),
    "rtlws_pfbsk_run": [_vp, _vp, _l, _i, _i, _i, C.c_float, C.c_float, C.c_float, _i, _i, C.c_float, _vp, _l, _vp, _l, _vp, _vp,
                        _l, _vp],
    "rtlws_pfbsk_close": ([_vp], None), "rtlws_pfbsk_last_error": ([], _str)}
PFBSK_SYMBOLS = list(_PFBSK_PROTOTYPES)
pfbsk_lib, pfbsk_last_error = _library("pfbsk", _PFBSK_PROTOTYPES)


def pfbsk_supported(log2_channels, taps_per_branch, hop, k_avg, nsub, output="power"):
    """rtlws_pfbsk_supported.  No GPU needed."""
    return pfbsk_lib().rtlws_pfbsk_supported(int(log2_channels), int(taps_per_branch), int(hop), int(k_avg), int(nsub),
                                             int(_PFBSPEC_OUTPUTS.get(output, output)))


def pfbsk_samples_needed(log2_channels, taps_per_branch, hop, k_avg, nsub, nspectra):
    """rtlws_pfbsk_samples_needed: (nspectra L K - 1) hop + T M, or -1.  No GPU needed."""
    return pfbsk_lib().rtlws_pfbsk_samples_needed(int(log2_channels), int(taps_per_branch), int(hop), int(k_avg), int(nsub),
                                                  int(nspectra))


def pfbsk_grid(log2_channels, taps_per_branch, hop, k_avg, nsub, nspectra):
    """rtlws_pfbsk_grid: (rc, workgroups, threads, LDS bytes, output rows per workgroup).  No GPU needed."""
    return _outs(pfbsk_lib().rtlws_pfbsk_grid,
                 (int(log2_channels), int(taps_per_branch), int(hop), int(k_avg), int(nsub), int(nspectra)), _GRID)


def pfbsk_power_scale(log2_channels, taps):
    """rtlws_pfbsk_power_scale of a prototype int16 [T * M]: 2^(-2 ceil(log2(128 sum|h|))) as a float.  No GPU needed."""
    taps = np.ascontiguousarray(taps, dtype=np.int16).reshape(-1)
    s = pfbsk_lib().rtlws_pfbsk_power_scale(int(log2_channels), taps.size >> int(log2_channels), _p(taps))
    if s == 0.0:
        raise RuntimeError("rtlws_pfbsk_power_scale failed: %s" % pfbsk_last_error())
    return s


def pfbsk_bounds(k_avg, sk_lo, sk_hi):
    """rtlws_pfbsk_bounds: thresholds on the estimator -> (ratio_lo, ratio_hi) as floats.  No GPU needed."""
    rc, lo, hi = _outs(pfbsk_lib().rtlws_pfbsk_bounds, (int(k_avg), float(sk_lo), float(sk_hi)), (C.c_float,) * 2)
    if rc != 0:
        raise RuntimeError("rtlws_pfbsk_bounds failed (rc=%d): %s" % (rc, pfbsk_last_error()))
    return lo, hi


# ---- include/rtlws_dedisp.h ----
DEDISP_MIN_NCHAN, DEDISP_MAX_NCHAN, DEDISP_MAX_TRIALS, DEDISP_MAX_DELAY = 4, 4096, 4096, 65535
_DEDISP_PROTOTYPES = {
    "rtlws_dedisp_supported": [_i, _i], "rtlws_dedisp_delays": [_i, _i, C.c_double, C.c_double, C.c_double, _i, C.c_double, C.c_double, _vp],
    "rtlws_dedisp_geometry": [_i, _i, _vp, _vp, _l, _ip, _ip, _ip, _ip, _ip, _ip], "rtlws_dedisp_open": ([_vp, _i, _i, _vp, _vp], _vp),
    "rtlws_dedisp_rows_needed": ([_vp, _l], _l), "rtlws_dedisp_run": [_vp, _vp, _l, _l, _vp, _l, _vp],
    "rtlws_dedisp_close": ([_vp], None), "rtlws_dedisp_last_error": ([], _str)}
DEDISP_SYMBOLS = list(_DEDISP_PROTOTYPES)
dedisp_lib, dedisp_last_error = _library("dedisp", _DEDISP_PROTOTYPES)


def dedisp_supported(nchan, ntrials):
    """rtlws_dedisp_supported.  No GPU needed."""
    return dedisp_lib().rtlws_dedisp_supported(int(nchan), int(ntrials))


def dedisp_delays(nchan, shifted, f_centre_hz, bandwidth_hz, row_seconds, ntrials, dm0, dm_step):
    """rtlws_dedisp_delays: the delays in rows of ntrials dispersion measures dm0 + t dm_step, int32 [ntrials, nchan].  No
    GPU needed."""
    out = np.zeros((max(int(ntrials), 0), max(int(nchan), 0)), np.int32)
    rc = dedisp_lib().rtlws_dedisp_delays(int(nchan), int(shifted), float(f_centre_hz), float(bandwidth_hz), float(row_seconds),
                                          int(ntrials), float(dm0), float(dm_step), _p(out))
    if rc != 0:
        raise RuntimeError("rtlws_dedisp_delays failed (rc=%d): %s" % (rc, dedisp_last_error()))
    return out


def _dedisp_table(delays, mask):
    """The table int32 [ntrials, nchan] and the mask (uint8 [nchan] or None) as the library reads them."""
    delays = np.ascontiguousarray(delays, dtype=np.int32)
    if delays.ndim != 2:
        raise RuntimeError("rtlws_dedisp: the table is [ntrials, nchan]")
    if mask is not None:
        mask = np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
        if mask.size != delays.shape[1]:
            raise RuntimeError("rtlws_dedisp: the mask holds nchan bytes")
    return delays, mask


def dedisp_geometry(delays, mask=None, nout=0):
    """rtlws_dedisp_geometry of a table int32 [ntrials, nchan]: (rc, workgroups, threads, LDS bytes, outputs per
    workgroup, trials per workgroup, largest delay over the kept positions).  No GPU needed."""
    delays, mask = _dedisp_table(delays, mask)
    return _outs(dedisp_lib().rtlws_dedisp_geometry,
                 (delays.shape[1], delays.shape[0], _p(delays), None if mask is None else _p(mask), int(nout)), (C.c_int,) * 6)


# ---- include/rtlws_pulse.h ----
PULSE_MAX_WIDTHS, PULSE_MAX_WIDTH, PULSE_MIN_SEG, PULSE_MAX_SEG, PULSE_MAX_TRIALS, PULSE_MAX_NOUT = 16, 1024, 64, 1 << 20, 65536, 1 << 30
PULSE_GUARD = 8            # Engine.pulse(fill=...): preset elements behind every output array
_lp = C.POINTER(C.c_long)
_PULSE_PROTOTYPES = {
    "rtlws_pulse_supported": [_i, _vp, _l], "rtlws_pulse_geometry": [_i, _vp, _l, _i, _l, _ip, _ip, _ip, _ip, _ip, _lp],
    "rtlws_pulse_open": ([_vp, _i, _vp, _l], _vp), "rtlws_pulse_samples_needed": ([_vp, _l], _l),
    "rtlws_pulse_segments": ([_vp, _l], _l), "rtlws_pulse_run": [_vp, _vp, _l, _i, _l, _vp, _vp, _vp, _vp],
    "rtlws_pulse_snr": ([C.c_double, _i, C.c_double, C.c_double, _l], C.c_double),
    "rtlws_pulse_close": ([_vp], None), "rtlws_pulse_last_error": ([], _str)}
PULSE_SYMBOLS = list(_PULSE_PROTOTYPES)
pulse_lib, pulse_last_error = _library("pulse", _PULSE_PROTOTYPES)


def _pulse_widths(widths):
    """The table as the library reads it: int32 [nwidths], or None (a NULL table)."""
    return None if widths is None else np.ascontiguousarray(widths, dtype=np.int32).reshape(-1)


def pulse_supported(widths, seg):
    """rtlws_pulse_supported.  No GPU needed."""
    widths = _pulse_widths(widths)
    return pulse_lib().rtlws_pulse_supported(0 if widths is None else widths.size, None if widths is None else _p(widths), int(seg))


def pulse_geometry(widths, seg, ntrials=1, nout=0):
    """rtlws_pulse_geometry: (rc, workgroups, threads, LDS bytes, outputs per tile, levels kept, segments).  No GPU
    needed."""
    widths = _pulse_widths(widths)
    return _outs(pulse_lib().rtlws_pulse_geometry,
                 (0 if widths is None else widths.size, None if widths is None else _p(widths), int(seg), int(ntrials), int(nout)),
                 (C.c_int,) * 5 + (C.c_long,))


def pulse_snr(peak, width, sum1, sum2, count):
    """rtlws_pulse_snr: (peak - width mean) / sqrt(width var) in double, NaN where it is not defined.  No GPU needed."""
    return pulse_lib().rtlws_pulse_snr(float(peak), int(width), float(sum1), float(sum2), int(count))


# ---- include/rtlws_fold.h ----
FOLD_MAX_PERIODS, FOLD_MIN_BINS, FOLD_MAX_BINS, FOLD_MIN_SUB, FOLD_MAX_SUB, FOLD_MAX_TRIALS, FOLD_MAX_NSAMP = 4096, 2, 256, 64, 1 << 24, 65536, 1 << 30
FOLD_GUARD = 8             # Engine.fold(fill=...): preset elements behind both output arrays
_u64 = C.c_uint64
_FOLD_PROTOTYPES = {
    "rtlws_fold_supported": [_i, _vp, _vp, _i, _l], "rtlws_fold_geometry": [_i, _i, _l, _i, _l, _ip, _ip, _ip, _ip, _ip, _lp],
    "rtlws_fold_open": ([_vp, _i, _vp, _vp, _i, _l], _vp), "rtlws_fold_subints": ([_vp, _l], _l),
    "rtlws_fold_run": [_vp, _vp, _l, _i, _l, _vp, _vp, _vp], "rtlws_fold_step": ([C.c_double], _u64),
    "rtlws_fold_phase_at": ([_u64, _u64, _l], _u64),
    "rtlws_fold_chi2": ([_vp, _vp, _i, C.c_double, C.c_double, _l], C.c_double),
    "rtlws_fold_close": ([_vp], None), "rtlws_fold_last_error": ([], _str)}
FOLD_SYMBOLS = list(_FOLD_PROTOTYPES)
fold_lib, fold_last_error = _library("fold", _FOLD_PROTOTYPES)


def _fold_table(values):
    """A table as the library reads it: uint64 [nperiods], or None (a NULL table)."""
    return None if values is None else np.ascontiguousarray(values, dtype=np.uint64).reshape(-1)


def fold_supported(steps, phases, nbins, sub):
    """rtlws_fold_supported of two tables uint64 [nperiods] (nperiods: the steps').  No GPU needed."""
    steps, phases = _fold_table(steps), _fold_table(phases)
    return fold_lib().rtlws_fold_supported(0 if steps is None else steps.size, None if steps is None else _p(steps),
                                           None if phases is None else _p(phases), int(nbins), int(sub))


def fold_geometry(nperiods, nbins, sub, ntrials=1, nsamp=0):
    """rtlws_fold_geometry: (rc, workgroups, threads, LDS bytes, samples per tile, wavefronts per workgroup, sub-integrations).
    No GPU needed."""
    return _outs(fold_lib().rtlws_fold_geometry, (int(nperiods), int(nbins), int(sub), int(ntrials), int(nsamp)),
                 (C.c_int,) * 5 + (C.c_long,))


def fold_step(period_in_samples):
    """rtlws_fold_step: the integer nearest to 2^64 / P, exactly; 0 outside 2 .. 2^32.  No GPU needed."""
    return int(fold_lib().rtlws_fold_step(float(period_in_samples)))


def fold_phase_at(step, phi0, n0):
    """rtlws_fold_phase_at: (phi0 + n0 step) mod 2^64.  No GPU needed."""
    return int(fold_lib().rtlws_fold_phase_at(int(step), int(phi0), int(n0)))


def fold_chi2(prof, hits, sum1, sum2, count):
    """rtlws_fold_chi2 of one profile float32 [nbins] and its hits uint32 [nbins], in double; NaN where it is not defined.
    No GPU needed."""
    prof, hits = np.ascontiguousarray(prof, dtype=np.float32).reshape(-1), np.ascontiguousarray(hits, dtype=np.uint32).reshape(-1)
    assert prof.size == hits.size
    return fold_lib().rtlws_fold_chi2(_p(prof) if prof.size else None, _p(hits) if hits.size else None, prof.size, float(sum1),
                                      float(sum2), int(count))


# ---- include/rtlws_period.h ----
PERIOD_MIN_LOG2N, PERIOD_MAX_LOG2N, PERIOD_MAX_LEVELS, PERIOD_MIN_NORM, PERIOD_MIN_SEG, PERIOD_MAX_TRIALS = 10, 15, 5, 16, 64, 65536
PERIOD_GUARD = 8           # Engine.period(fill=...): preset elements behind every output array
_PERIOD_PROTOTYPES = {
    "rtlws_period_supported": [_i, _i, _i, _i, _i], "rtlws_period_geometry": [_i, _i, _i, _i, _i, _i, _ip, _ip, _ip, _ip],
    "rtlws_period_open": ([_vp, _i, _i, _i, _i, _i], _vp), "rtlws_period_run": [_vp, _vp, _l, _i, _i, _vp, _vp, _vp, _vp, _vp],
    "rtlws_period_samples": ([_i, _i, _i], C.c_double), "rtlws_period_lnq": ([C.c_double, _i], C.c_double),
    "rtlws_period_close": ([_vp], None), "rtlws_period_last_error": ([], _str)}
PERIOD_SYMBOLS = list(_PERIOD_PROTOTYPES)
period_lib, period_last_error = _library("period", _PERIOD_PROTOTYPES)


def period_supported(log2n, levels, norm, seg, klo):
    """rtlws_period_supported.  No GPU needed."""
    return period_lib().rtlws_period_supported(int(log2n), int(levels), int(norm), int(seg), int(klo))


def period_geometry(log2n, levels, norm, seg, klo, ntrials=1):
    """rtlws_period_geometry: (rc, workgroups, threads, LDS bytes, segments).  No GPU needed."""
    return _outs(period_lib().rtlws_period_geometry, (int(log2n), int(levels), int(norm), int(seg), int(klo), int(ntrials)), _GRID)


def period_samples(log2n, level, k):
    """rtlws_period_samples: N 2^level / k, the fundamental's period in samples; 0 where an argument is out of range.  No
    GPU needed."""
    return period_lib().rtlws_period_samples(int(log2n), int(level), int(k))


def period_lnq(s, h):
    """rtlws_period_lnq: ln of the false-alarm probability of a sum s of h whitened powers; NaN where it is not defined.  No
    GPU needed."""
    return period_lib().rtlws_period_lnq(float(s), int(h))


# ---- include/rtlws_periodlong.h ----
PERIODLONG_MIN_LOG2N, PERIODLONG_MAX_LOG2N, PERIODLONG_MAX_LEVELS, PERIODLONG_MAX_TRIALS, PERIODLONG_STAGES = 16, 22, 5, 65536, 6
PERIODLONG_MIN_NORM, PERIODLONG_MAX_NORM, PERIODLONG_MIN_SEG, PERIODLONG_MAX_SEG = 16, 16384, 64, 16384
PERIODLONG_WORKSPACE_CAP = 1 << 30
_PERIODLONG_PROTOTYPES = {
    "rtlws_periodlong_supported": [_i, _i, _i, _i, _i], "rtlws_periodlong_geometry": [_i, _i, _i, _i, _i, _i, _ip, _ip, _ip, _ip],
    "rtlws_periodlong_open": ([_vp, _i, _i, _i, _i, _i, _i], _vp), "rtlws_periodlong_workspace_bytes": ([_vp], _sz),
    "rtlws_periodlong_run": [_vp, _vp, _l, _i, _i, _vp, _vp, _vp, _vp, _vp], "rtlws_periodlong_samples": ([_i, _i, _i], C.c_double),
    "rtlws_periodlong_close": ([_vp], None), "rtlws_periodlong_last_error": ([], _str)}
PERIODLONG_SYMBOLS = list(_PERIODLONG_PROTOTYPES)
periodlong_lib, periodlong_last_error = _library("periodlong", _PERIODLONG_PROTOTYPES)


def periodlong_supported(log2n, levels, norm, seg, klo):
    """rtlws_periodlong_supported.  No GPU needed."""
    return periodlong_lib().rtlws_periodlong_supported(int(log2n), int(levels), int(norm), int(seg), int(klo))


def periodlong_geometry(log2n, levels, norm, seg, klo, ntrials=1):
    """rtlws_periodlong_geometry: (rc, workgroups, threads, LDS bytes -- a tuple of PERIODLONG_STAGES each: mean, columns,
    rows, untangling, whitening, peaks -- and segments).  No GPU needed."""
    return _outs(periodlong_lib().rtlws_periodlong_geometry, (int(log2n), int(levels), int(norm), int(seg), int(klo), int(ntrials)),
                 (C.c_int * PERIODLONG_STAGES,) * 3 + (C.c_int,))


def periodlong_samples(log2n, level, k):
    """rtlws_periodlong_samples: N 2^level / k, the fundamental's period in samples; 0 where an argument is out of range.
    No GPU needed."""
    return periodlong_lib().rtlws_periodlong_samples(int(log2n), int(level), int(k))


# ---- include/rtlws_accel.h ----
ACCEL_MAX_NACCEL, ACCEL_MAX_COEF, ACCEL_MAX_VIRTUAL, ACCEL_STAGES = 1024, 1 << 40, 65536, 6
_i64p = C.POINTER(C.c_int64)
_ACCEL_PROTOTYPES = {
    "rtlws_accel_supported": [_i, _i, _i, _i, _i, _i, _i64p], "rtlws_accel_geometry": [_i, _i, _i, _i, _i, _i, _i64p, _i, _ip, _ip, _ip, _ip],
    "rtlws_accel_open": ([_vp, _i, _i, _i, _i, _i, _i, _i64p, _i], _vp), "rtlws_accel_workspace_bytes": ([_vp], _sz),
    "rtlws_accel_search": [_vp, _vp, _l, _i, _i, _vp, _vp, _vp, _vp, _vp], "rtlws_accel_resample": [_vp, _vp, _l, _i, _i, _i, _i, _vp, _l, _vp],
    "rtlws_accel_coef": ([C.c_double, C.c_double], C.c_int64), "rtlws_accel_coef_from_shift": ([C.c_double, _i], C.c_int64),
    "rtlws_accel_shift": ([C.c_int64, _i, _i], C.c_long), "rtlws_accel_close": ([_vp], None), "rtlws_accel_last_error": ([], _str)}
ACCEL_SYMBOLS = list(_ACCEL_PROTOTYPES)
accel_lib, accel_last_error = _library("accel", _ACCEL_PROTOTYPES)


def _accel_table(coefs):
    """A table as the library reads it: (naccel, int64 [naccel] or None for a NULL table, its pointer or None)."""
    if coefs is None:
        return 0, None, None
    table = np.ascontiguousarray(coefs, dtype=np.int64).reshape(-1)
    return table.size, table, table.ctypes.data_as(_i64p) if table.size else None


def accel_supported(log2n, levels, norm, seg, klo, coefs, naccel=None):
    """rtlws_accel_supported of a table int64 [naccel] (naccel: the table's size unless given; None: a NULL table).  No
    GPU needed."""
    n, _table, ptr = _accel_table(coefs)
    return accel_lib().rtlws_accel_supported(int(log2n), int(levels), int(norm), int(seg), int(klo), n if naccel is None else int(naccel), ptr)


def accel_geometry(log2n, levels, norm, seg, klo, coefs, ntrials=1, naccel=None):
    """rtlws_accel_geometry: (rc, workgroups over all ntrials * naccel virtual trials, threads, LDS bytes -- a tuple of
    ACCEL_STAGES each -- and segments).  No GPU needed."""
    n, _table, ptr = _accel_table(coefs)
    return _outs(accel_lib().rtlws_accel_geometry,
                 (int(log2n), int(levels), int(norm), int(seg), int(klo), n if naccel is None else int(naccel), ptr, int(ntrials)),
                 (C.c_int * ACCEL_STAGES,) * 3 + (C.c_int,))


def accel_coef(accel_m_s2, tsamp_s):
    """rtlws_accel_coef: the integer nearest accel * tsamp / (2 c) * 2^64; 0 where it is refused.  No GPU needed."""
    return int(accel_lib().rtlws_accel_coef(float(accel_m_s2), float(tsamp_s)))


def accel_coef_from_shift(mid_shift_samples, nsamp):
    """rtlws_accel_coef_from_shift: the integer nearest shift * 4 / (nsamp - 1)^2 * 2^64; 0 where it is refused.  No GPU
    needed."""
    return int(accel_lib().rtlws_accel_coef_from_shift(float(mid_shift_samples), int(nsamp)))


def accel_shift(coef, nsamp, n):
    """rtlws_accel_shift: s_c(n), exactly; 0 where an argument is out of range.  No GPU needed."""
    return int(accel_lib().rtlws_accel_shift(int(coef), int(nsamp), int(n)))


def host_error():
    """(count, first message) of include/rtlws_host.h's sticky failure record."""
    L = amd_lib()
    return L.rtlws_host_error_count(), L.rtlws_host_error().decode()


def host_error_clear():
    amd_lib().rtlws_host_error_clear()


STREAM_ENGINE, STREAM_DEFAULT = None, 1     # include/rtlws_hip.h "Streams"


def torch_stream_handle(stream=None):
    """The `stream` argument for a torch caller: torch's default stream has handle 0, which
    the C-ABI reads as "the engine's own non-blocking stream" (NOT ordered against torch's
    kernels) -- so 0 is mapped to RTLWS_STREAM_DEFAULT, HIP's default stream itself."""
    import torch
    h = (torch.cuda.current_stream() if stream is None else stream).cuda_stream
    return h if h else STREAM_DEFAULT


def make_desc(n_fft, k_avg=1, input="cu8", window="rect", output="power_sum", cic_r=0, gain_db=0, flags=0):
    return SpectraDesc(int(n_fft), int(k_avg), _INPUTS.get(input, input), _WINDOWS.get(window, window),
                       _OUTPUTS.get(output, output), int(cic_r), int(gain_db), int(flags))


class DevBuf:
    def __init__(self, eng, nbytes):
        self.eng, self.nbytes = eng, int(nbytes)
        self.ptr = hip_lib().rtlws_dev_alloc(eng.h, self.nbytes)
        if not self.ptr:
            raise RuntimeError("rtlws_dev_alloc(%d) failed: %s" % (nbytes, last_error()))

    def free(self):
        if self.ptr:
            hip_lib().rtlws_dev_free(self.eng.h, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _PlanBase:
    """What every satellite library's plan shares: the library (_name, _lib), the handle h of rtlws_<name>_open, the
    calls through it, close.  eng may be None (as a C caller's NULL engine): open then fails with the library's text.
    A subclass names its library, hands _open what its open takes behind the engine, and keeps its run signatures.
    The plans of this module derive from _Plan below; a library's submodule derives from this."""
    _name, _lib, h = None, None, None

    def _open(self, eng, *args):
        self.eng = eng
        self.h = self._fn("open")(eng.h if eng is not None else None, *args)
        if not self.h:
            raise RuntimeError("rtlws_%s_open failed: %s" % (self._name, self._fn("last_error")().decode()))

    @classmethod
    def open(cls, *args, **kwargs):
        return cls(*args, **kwargs)

    @classmethod
    def _fn(cls, what):
        return getattr(cls._lib(), "rtlws_%s_%s" % (cls._name, what))

    @staticmethod
    def _ptr(x):
        return None if x is None else Engine._ptr(x)

    @classmethod
    def _array(cls, d_iqs):
        """The captures' device buffers or pointers as a C array, or None (a NULL array)."""
        return None if d_iqs is None else (C.c_void_p * max(len(d_iqs), 1))(*[cls._ptr(x) for x in d_iqs])

    def _call(self, what, check, *args):
        rc = self._fn(what)(self.h, *args)
        if check and rc != 0:
            raise RuntimeError("rtlws_%s_%s failed (rc=%d): %s" % (self._name, what, rc, self._fn("last_error")().decode()))
        return rc

    def close(self):
        if self.h:
            self._fn("close")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Plan(_PlanBase):
    """The plans of the libraries this module binds (tests/test_python_api_cpu.py pins its subclasses)."""


def _words(tuning_words):
    """The tuning words as a C array of int (never empty: a NULL array is not what an empty list means)."""
    return (C.c_int * max(len(tuning_words), 1))(*[int(k) for k in tuning_words])


class _FramesPlan(_Plan):
    """The plans of one descriptor (include/rtlws_long.h, include/rtlws_anylen.h): the same open, workspace and run."""

    def __init__(self, eng, desc, max_frames=1):
        self.desc = desc
        self._open(eng, C.byref(desc), int(max_frames))

    @property
    def workspace_bytes(self):
        return self._fn("workspace_bytes")(self.h)

    def run(self, d_in, nframes, d_out, stream=None, check=True):
        return self._call("run", check, self._ptr(d_in), int(nframes), self._ptr(d_out), stream)


class LongPlan(_FramesPlan):
    """rtlws_long_plan* of include/rtlws_long.h: one descriptor, tables and workspace for up to max_frames frames
    per group.  eng may be None (as a C caller's NULL engine): open then fails with the library's text."""
    _name, _lib = "long", staticmethod(long_lib)


class AnyLenPlan(_FramesPlan):
    """rtlws_anylen_plan* of include/rtlws_anylen.h: one descriptor, tables and workspaces for up to max_frames
    frames per group.  eng may be None (as a C caller's NULL engine): open then fails with the library's text."""
    _name, _lib = "anylen", staticmethod(anylen_lib)


class DdcPlan(_Plan):
    """rtlws_ddc_plan* of include/rtlws_ddc.h: the phasor table on the engine's device, the kernels loaded.  eng may
    be None (as a C caller's NULL engine): open then fails with the library's text."""
    _name, _lib = "ddc", staticmethod(ddc_lib)

    def __init__(self, eng):
        self._open(eng)

    def run(self, cic_r, d_iq, dec_len, tuning_words, d_out, out_stride=None, first_dec_index=0, stream=None, check=True):
        """One launch: channel c of the bank is the cmplx_s32 stream at d_out + c * out_stride samples."""
        return self._call("run", check, int(cic_r), self._ptr(d_iq), int(dec_len), int(first_dec_index), len(tuning_words),
                          _words(tuning_words), self._ptr(d_out), int(dec_len if out_stride is None else out_stride), stream)


class DdcFirPlan(_Plan):
    """rtlws_ddcfir_plan* of include/rtlws_ddcfir.h: the taps and the phasor table on the engine's device, the kernel of
    (decim, ntaps) loaded.  eng may be None (as a C caller's NULL engine): open then fails with the library's text."""
    _name, _lib = "ddcfir", staticmethod(ddcfir_lib)

    def __init__(self, eng, decim, taps):
        self.decim = int(decim)
        self.taps = None if taps is None else np.ascontiguousarray(taps, dtype=np.int16).reshape(-1)
        self.ntaps = 0 if self.taps is None else self.taps.size
        self._open(eng, self.decim, self.ntaps, None if self.taps is None else _p(self.taps))

    def run(self, d_iq, dec_len, tuning_words, d_out, out_shift=14, out_stride=None, first_dec_index=0, stream=None, check=True):
        """One launch: channel c of the bank is the cmplx_s32 stream at d_out + c * out_stride samples."""
        return self._call("run", check, self._ptr(d_iq), int(dec_len), int(first_dec_index), len(tuning_words),
                          _words(tuning_words), int(out_shift), self._ptr(d_out),
                          int(dec_len if out_stride is None else out_stride), stream)


class FmBankPlan(_Plan):
    """rtlws_fmbank_plan* of include/rtlws_fmbank.h: the phasor table on the engine's device, the kernels loaded.  eng
    may be None (as a C caller's NULL engine): open then fails with the library's text."""
    _name, _lib = "fmbank", staticmethod(fmbank_lib)

    def __init__(self, eng):
        self._open(eng)

    def run(self, cic_r, d_iq, block_len, nblocks, tuning_words, d_state_in, d_state_out, d_audio, audio_stride=None,
            first_dec_index=0, stream=None, check=True):
        """One launch: audio of channel c at d_audio + c * audio_stride floats, states channel-major [C, 21]."""
        stride = int(nblocks) * (int(block_len) // 4) if audio_stride is None else int(audio_stride)
        return self._call("run", check, int(cic_r), self._ptr(d_iq), int(block_len), int(nblocks), int(first_dec_index),
                          len(tuning_words), _words(tuning_words), self._ptr(d_state_in), self._ptr(d_state_out),
                          self._ptr(d_audio), stride, stream)


class FmFirPlan(_Plan):
    """rtlws_fmfir_plan* of include/rtlws_fmfir.h: the taps and the phasor table on the engine's device, the kernel of
    (decim, ntaps) and the state copy loaded.  eng may be None (as a C caller's NULL engine): open then fails with the
    library's text."""
    _name, _lib = "fmfir", staticmethod(fmfir_lib)

    def __init__(self, eng, decim, taps):
        self.decim = int(decim)
        self.taps = None if taps is None else np.ascontiguousarray(taps, dtype=np.int16).reshape(-1)
        self.ntaps = 0 if self.taps is None else self.taps.size
        self._open(eng, self.decim, self.ntaps, None if self.taps is None else _p(self.taps))

    def run(self, d_iq, block_len, nblocks, tuning_words, d_state_in, d_state_out, d_audio, out_shift=14, audio_stride=None,
            first_dec_index=0, stream=None, check=True):
        """One launch: audio of channel c at d_audio + c * audio_stride floats, states channel-major [C, 21]."""
        stride = int(nblocks) * (int(block_len) // 4) if audio_stride is None else int(audio_stride)
        return self._call("run", check, self._ptr(d_iq), int(block_len), int(nblocks), int(first_dec_index),
                          len(tuning_words), _words(tuning_words), int(out_shift), self._ptr(d_state_in),
                          self._ptr(d_state_out), self._ptr(d_audio), stride, stream)


class _PolyphasePlan(_Plan):
    """What the plans of the polyphase family add (include/rtlws_pfb.h and the headers on top of it): the prototype
    (int16 [T * M]) and the transform's table on the engine's device, the kernels loaded.  A subclass hands __init__
    what its open takes behind the taps."""

    def __init__(self, eng, log2_channels, taps, *counts):
        """counts: what the library's open takes behind the taps (none, ninputs, or ninputs and nbeams)."""
        self.log2_channels = int(log2_channels)
        taps = np.ascontiguousarray(taps, dtype=np.int16).reshape(-1)
        m = 1 << self.log2_channels if 0 <= self.log2_channels < 31 else 0
        if m == 0 or taps.size == 0 or taps.size % m:
            raise RuntimeError("rtlws_%s_open: the prototype holds taps_per_branch * M taps" % self._name)
        self.taps_per_branch = taps.size // m
        self._open(eng, self.log2_channels, self.taps_per_branch, _p(taps), *counts)


class PfbSpecPlan(_PolyphasePlan):
    """rtlws_pfbspec_plan* of include/rtlws_pfbspec.h: the prototype (int16 [T * M]) and the transform's table on the
    engine's device, the kernel loaded.  eng may be None (as a C caller's NULL engine): open then fails with the
    library's text."""
    _name, _lib = "pfbspec", staticmethod(pfbspec_lib)

    def run(self, d_iq, nspectra, k_avg, d_out, hop=None, output="power", shifted=False, scale=1.0, out_stride=None,
            stream=None, check=True):
        """One launch: row j at d_out + j * out_stride elements (f32, or bytes for "payload").  output: "power", "db",
        "payload" or a value of enum rtlws_output."""
        m = 1 << self.log2_channels
        return self._call("run", check, self._ptr(d_iq), int(nspectra), int(m if hop is None else hop), int(k_avg),
                          int(_PFBSPEC_OUTPUTS.get(output, output)), int(shifted), float(scale), self._ptr(d_out),
                          int(m if out_stride is None else out_stride), stream)


class PfbSkPlan(_PolyphasePlan):
    """rtlws_pfbsk_plan* of include/rtlws_pfbsk.h: the prototype (int16 [T * M]) and the transform's table on the
    engine's device, the kernel loaded.  eng may be None (as a C caller's NULL engine): open then fails with the
    library's text."""
    _name, _lib = "pfbsk", staticmethod(pfbsk_lib)

    def run(self, d_iq, nspectra, k_avg, nsub, power_scale, d_clean, ratio_lo=0.0, ratio_hi=float("inf"), d_kept=None,
            d_s1=None, d_s2=None, hop=None, output="power", shifted=False, scale=1.0, clean_stride=None, kept_stride=None,
            sub_stride=None, stream=None, check=True):
        """One launch: clean row j at d_clean + j * clean_stride elements (f32, or bytes for "payload"), its counts at
        d_kept + j * kept_stride (uint32), the S1 and S2 rows of sub-integration q at d_s1 and d_s2 + q * sub_stride
        (f32); d_kept, and d_s1 with d_s2, may be None.  output: "power", "db", "payload" or a value of enum
        rtlws_output."""
        m = 1 << self.log2_channels
        return self._call("run", check, self._ptr(d_iq), int(nspectra), int(m if hop is None else hop), int(k_avg), int(nsub),
                          float(power_scale), float(ratio_lo), float(ratio_hi), int(_PFBSPEC_OUTPUTS.get(output, output)),
                          int(shifted), float(scale), self._ptr(d_clean), int(m if clean_stride is None else clean_stride),
                          self._ptr(d_kept), int(m if kept_stride is None else kept_stride), self._ptr(d_s1), self._ptr(d_s2),
                          int(m if sub_stride is None else sub_stride), stream)


class DedispPlan(_Plan):
    """rtlws_dedisp_plan* of include/rtlws_dedisp.h: the table (int32 [ntrials, nchan]) and the mask (uint8 [nchan] or
    None) on the engine's device in the kernel's form, the kernel loaded.  eng may be None (as a C caller's NULL engine):
    open then fails with the library's text."""
    _name, _lib = "dedisp", staticmethod(dedisp_lib)

    def __init__(self, eng, delays, mask=None):
        delays, mask = _dedisp_table(delays, mask)
        self.ntrials, self.nchan = delays.shape
        self._open(eng, self.nchan, self.ntrials, _p(delays), None if mask is None else _p(mask))

    def rows_needed(self, nout):
        return self._fn("rows_needed")(self.h, int(nout))

    def run(self, d_rows, nout, d_out, in_stride=None, out_stride=None, stream=None, check=True):
        """One launch: trial t at d_out + t * out_stride elements (f32), row j of the input at d_rows + j * in_stride."""
        return self._call("run", check, self._ptr(d_rows), int(self.nchan if in_stride is None else in_stride), int(nout),
                          self._ptr(d_out), int(nout if out_stride is None else out_stride), stream)


class PulsePlan(_Plan):
    """rtlws_pulse_plan* of include/rtlws_pulse.h: the table of widths (int32 [nwidths]) on the engine's device in the
    kernel's form, the kernel loaded.  eng may be None (as a C caller's NULL engine): open then fails with the library's
    text."""
    _name, _lib = "pulse", staticmethod(pulse_lib)

    def __init__(self, eng, widths, seg):
        widths = _pulse_widths(widths)
        self.nwidths, self.seg = widths.size, int(seg)
        self._open(eng, self.nwidths, _p(widths), self.seg)

    def samples_needed(self, nout):
        return self._fn("samples_needed")(self.h, int(nout))

    def segments(self, nout):
        return self._fn("segments")(self.h, int(nout))

    def run(self, d_in, in_stride, ntrials, nout, d_peak, d_at, d_mom=None, stream=None, check=True):
        """One launch: trial t at d_in + t * in_stride elements; d_peak and d_at [ntrials, nwidths, nseg] (f32, int32),
        d_mom [ntrials, nseg, 2] (f64) or None."""
        return self._call("run", check, self._ptr(d_in), int(in_stride), int(ntrials), int(nout), self._ptr(d_peak),
                          self._ptr(d_at), self._ptr(d_mom), stream)


class FoldPlan(_Plan):
    """rtlws_fold_plan* of include/rtlws_fold.h: the steps and the phases (uint64 [nperiods] each) on the engine's device,
    the kernel of nbins' block shape loaded.  eng may be None (as a C caller's NULL engine): open then fails with the
    library's text."""
    _name, _lib = "fold", staticmethod(fold_lib)

    def __init__(self, eng, steps, phases, nbins, sub):
        steps, phases = _fold_table(steps), _fold_table(phases)
        assert steps.size == phases.size, "a phase for every step"
        self.nperiods, self.nbins, self.sub = steps.size, int(nbins), int(sub)
        self._open(eng, self.nperiods, _p(steps), _p(phases), self.nbins, self.sub)

    def subints(self, nsamp):
        return self._fn("subints")(self.h, int(nsamp))

    def run(self, d_in, in_stride, ntrials, nsamp, d_prof, d_hits=None, stream=None, check=True):
        """One launch: trial t at d_in + t * in_stride elements; d_prof [ntrials, nperiods, nsub, nbins] (f32), d_hits
        [nperiods, nsub, nbins] (uint32) or None."""
        return self._call("run", check, self._ptr(d_in), int(in_stride), int(ntrials), int(nsamp), self._ptr(d_prof),
                          self._ptr(d_hits), stream)


class _SearchPlan(_Plan):
    """The plans of the periodicity-search family (include/rtlws_period.h, rtlws_periodlong.h, rtlws_accel.h): the five
    plan parameters, nbins = M and nseg = M / seg, and the marshalling of a search.  A subclass names its library and hands
    __init__ what its open takes behind klo.  eng may be None (as a C caller's NULL engine): open then fails with the
    library's text."""

    def __init__(self, eng, log2n, levels, norm, seg, klo, *more):
        self.log2n, self.levels, self.norm, self.seg, self.klo = int(log2n), int(levels), int(norm), int(seg), int(klo)
        self._open(eng, self.log2n, self.levels, self.norm, self.seg, self.klo, *more)
        self.nbins = 1 << (self.log2n - 1)
        self.nseg = self.nbins // self.seg

    def _search(self, what, d_in, in_stride, ntrials, nsamp, d_best, d_at, d_power, d_white, stream, check):
        return self._call(what, check, self._ptr(d_in), int(in_stride), int(ntrials), int(nsamp), self._ptr(d_best),
                          self._ptr(d_at), self._ptr(d_power), self._ptr(d_white), stream)


class _LongSearchPlan(_SearchPlan):
    """The two plans that keep a workspace on the device (the long frames')."""

    def workspace_bytes(self):
        return self._fn("workspace_bytes")(self.h)


class PeriodPlan(_SearchPlan):
    """rtlws_period_plan* of include/rtlws_period.h: the transform's table on the engine's device, the kernel of the frame
    length loaded."""
    _name, _lib = "period", staticmethod(period_lib)

    def __init__(self, eng, log2n, levels, norm, seg, klo):
        super().__init__(eng, log2n, levels, norm, seg, klo)

    def run(self, d_in, in_stride, ntrials, nsamp, d_best, d_at, d_power=None, d_white=None, stream=None, check=True):
        """One launch: trial t at d_in + t * in_stride elements; d_best and d_at [ntrials, levels, nseg] (f32, int32),
        d_power and d_white [ntrials, M] (f32) or None."""
        return self._search("run", d_in, in_stride, ntrials, nsamp, d_best, d_at, d_power, d_white, stream, check)


class PeriodLongPlan(_LongSearchPlan):
    """rtlws_periodlong_plan* of include/rtlws_periodlong.h: the tables and a workspace for min(max_trials, what fits under
    the cap) trials in flight on the engine's device, the kernels of the frame length loaded."""
    _name, _lib = "periodlong", staticmethod(periodlong_lib)

    def __init__(self, eng, log2n, levels, norm, seg, klo, max_trials=1):
        super().__init__(eng, log2n, levels, norm, seg, klo, int(max_trials))

    def run(self, d_in, in_stride, ntrials, nsamp, d_best, d_at, d_power=None, d_white=None, stream=None, check=True):
        """Six launches a group of trials: trial t at d_in + t * in_stride elements; d_best and d_at [ntrials, levels,
        nseg] (f32, int32), d_power and d_white [ntrials, M] (f32) or None."""
        return self._search("run", d_in, in_stride, ntrials, nsamp, d_best, d_at, d_power, d_white, stream, check)


class AccelPlan(_LongSearchPlan):
    """rtlws_accel_plan* of include/rtlws_accel.h: rtlws_periodlong.h's tables, the coefficients (int64 [naccel]) and a
    workspace for min(max_trials, what fits under the cap) virtual trials in flight on the engine's device, the kernels of
    the frame length loaded."""
    _name, _lib = "accel", staticmethod(accel_lib)

    def __init__(self, eng, log2n, levels, norm, seg, klo, coefs, max_trials=1):
        self.naccel, self.coefs, ptr = _accel_table(coefs)
        super().__init__(eng, log2n, levels, norm, seg, klo, self.naccel, ptr, int(max_trials))

    def search(self, d_in, in_stride, ntrials, nsamp, d_best, d_at, d_power=None, d_white=None, stream=None, check=True):
        """Six launches a group of virtual trials: trial t at d_in + t * in_stride elements; d_best and d_at [ntrials,
        naccel, levels, nseg] (f32, int32), d_power and d_white [ntrials, naccel, M] (f32) or None."""
        return self._search("search", d_in, in_stride, ntrials, nsamp, d_best, d_at, d_power, d_white, stream, check)

    def resample(self, d_in, in_stride, ntrials, nsamp, a_first, a_count, d_out, out_stride, stream=None, check=True):
        """One launch: the series of (t, a), a = a_first .. a_first + a_count - 1, at d_out + (t * a_count + a - a_first) *
        out_stride elements."""
        return self._call("resample", check, self._ptr(d_in), int(in_stride), int(ntrials), int(nsamp), int(a_first), int(a_count),
                          self._ptr(d_out), int(out_stride), stream)


class PfbXcPlan(_PolyphasePlan):
    """rtlws_pfbxc_plan* of include/rtlws_pfbxc.h: the prototype (int16 [T * M]) and the transform's table on the
    engine's device, the kernel for ninputs captures loaded.  eng may be None (as a C caller's NULL engine): open then
    fails with the library's text."""
    _name, _lib = "pfbxc", staticmethod(pfbxc_lib)

    def __init__(self, eng, log2_channels, taps, ninputs):
        self.ninputs = int(ninputs)
        super().__init__(eng, log2_channels, taps, self.ninputs)

    def run(self, d_iqs, nspectra, k_avg, d_auto, d_cross, hop=None, shifted=False, auto_stride=None, cross_stride=None,
            stream=None, check=True):
        """One launch.  d_iqs: the captures' device buffers or pointers, or None (a NULL array).  Row j * A + a of
        d_auto (auto_stride floats apart) is S_a[j]; row j * NX + x of d_cross (cross_stride complex values apart)
        is V_ab[j]."""
        m = 1 << self.log2_channels
        return self._call("run", check, self._array(d_iqs), int(nspectra), int(m if hop is None else hop), int(k_avg),
                          int(shifted), self._ptr(d_auto), int(m if auto_stride is None else auto_stride), self._ptr(d_cross),
                          int(m if cross_stride is None else cross_stride), stream)


class PfbBfPlan(_PolyphasePlan):
    """rtlws_pfbbf_plan* of include/rtlws_pfbbf.h: the prototype (int16 [T * M]) and the transform's table on the
    engine's device, both kernels for nbeams beams loaded.  eng may be None (as a C caller's NULL engine): open then
    fails with the library's text."""
    _name, _lib = "pfbbf", staticmethod(pfbbf_lib)

    def __init__(self, eng, log2_channels, taps, ninputs, nbeams):
        self.ninputs, self.nbeams = int(ninputs), int(nbeams)
        super().__init__(eng, log2_channels, taps, self.ninputs, self.nbeams)

    def run(self, d_iqs, d_weights, nframes, d_out, hop=None, out_stride=None, beam_stride=None, first_frame_index=0,
            layout="channel", stream=None, check=True, ninputs=None, nbeams=None):
        """Voltage mode, one launch.  d_iqs: the captures' device buffers or pointers, or None (a NULL array);
        d_weights: complex f32 [B, A, M] on the device.  Beam b at d_out + b * beam_stride values, inside it layout
        "channel": channel c at c * out_stride; "time": frame m at m * out_stride.  The strides default to the
        densest."""
        m = 1 << self.log2_channels
        lay = _PFB_LAYOUTS.get(layout, layout)
        if out_stride is None:
            out_stride = m if lay == PFB_TIME_MAJOR else nframes
        if beam_stride is None:
            beam_stride = m * nframes
        return self._call("run", check, self._array(d_iqs), int(self.ninputs if ninputs is None else ninputs),
                          self._ptr(d_weights), int(self.nbeams if nbeams is None else nbeams), int(nframes),
                          int(m if hop is None else hop), int(first_frame_index), int(lay), self._ptr(d_out),
                          int(out_stride), int(beam_stride), stream)

    def power(self, d_iqs, d_weights, nspectra, k_avg, d_out, hop=None, shifted=False, row_stride=None, stream=None,
              check=True, ninputs=None, nbeams=None):
        """Power mode, one launch.  Row j * B + b of d_out (row_stride floats apart) is S_b[j]."""
        m = 1 << self.log2_channels
        return self._call("power", check, self._array(d_iqs), int(self.ninputs if ninputs is None else ninputs),
                          self._ptr(d_weights), int(self.nbeams if nbeams is None else nbeams), int(nspectra),
                          int(m if hop is None else hop), int(k_avg), int(shifted), self._ptr(d_out),
                          int(m if row_stride is None else row_stride), stream)


class PfbPlan(_PolyphasePlan):
    """rtlws_pfb_plan* of include/rtlws_pfb.h: the prototype (int16 [T * M]) and the transform's table on the engine's
    device, the kernel loaded.  eng may be None (as a C caller's NULL engine): open then fails with the library's text."""
    _name, _lib = "pfb", staticmethod(pfb_lib)

    def run(self, d_iq, nframes, d_out, hop=None, out_stride=None, first_frame_index=0, layout="channel", stream=None,
            check=True):
        """One launch.  layout "channel": channel c at d_out + c * out_stride values; "time": frame m at
        d_out + m * out_stride values (or an integer: rtlws_pfb.h's constants)."""
        m = 1 << self.log2_channels
        lay = _PFB_LAYOUTS.get(layout, layout)
        if out_stride is None:
            out_stride = m if lay == PFB_TIME_MAJOR else nframes
        return self._call("run", check, self._ptr(d_iq), int(nframes), int(m if hop is None else hop), int(first_frame_index),
                          int(lay), self._ptr(d_out), int(out_stride), stream)


class Engine:
    """One engine per device (include/rtlws_hip.h). Fails loudly without a GPU."""

    def __init__(self, device=0):
        self.h = hip_lib().rtlws_engine_create(int(device))
        if not self.h:
            raise RuntimeError("rtlws_engine_create(%d) failed: %s" % (device, last_error()))
        self.device = device

    def close(self):
        if self.h:
            hip_lib().rtlws_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- memory ----------------------------------------------------------
    def alloc(self, nbytes):
        return DevBuf(self, nbytes)

    def upload(self, arr, stream=None):
        arr = np.ascontiguousarray(arr)
        buf = DevBuf(self, arr.nbytes)
        try:
            self._chk(hip_lib().rtlws_copy_h2d(self.h, buf.ptr, _p(arr), arr.nbytes, stream), "h2d")
            self.sync(stream)
        except Exception:
            buf.free()                                    # nobody else holds it yet
            raise
        return buf

    def download(self, buf, dtype, shape, stream=None):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= buf.nbytes
        self._chk(hip_lib().rtlws_copy_d2h(self.h, _p(out), buf.ptr, out.nbytes, stream), "d2h")
        self.sync(stream)
        return out

    def sync(self, stream=None):
        self._chk(hip_lib().rtlws_stream_sync(self.h, stream), "sync")

    def clock_stamp(self, d_out, slots, stream=None):
        """`slots` one-wavefront workgroups on `stream` write {shader clocks, 100 MHz ticks, place, magic} to the
        device pointer d_out (slots x 4 64-bit words)."""
        self._chk(hip_lib().rtlws_clock_stamp(self.h, self._ptr(d_out), int(slots), stream), "rtlws_clock_stamp")

    @staticmethod
    def clock_from_stamps(a0, a1):
        """(sclk_ghz, seconds, places) between two stamp launches (arrays of shape [slots, 4]): the records are paired
        by place -- s_memtime is a counter of the place it is read at -- and the median of d(memtime) / d(memrealtime)
        x 100 MHz over the places both launches reached is returned, with the median interval and the number of
        places; (None, 0.0, 0) when no place is common or the interval is empty."""
        first = {}
        for mt, rt, place, magic in np.asarray(a0).astype(np.int64).tolist():
            if magic == 0x5354414d50 and place not in first:
                first[place] = (mt, rt)
        ghz, secs = [], []
        seen = set()
        for mt, rt, place, magic in np.asarray(a1).astype(np.int64).tolist():
            if magic == 0x5354414d50 and place in first and place not in seen:
                seen.add(place)
                dmt, drt = mt - first[place][0], rt - first[place][1]
                if drt > 0 and dmt > 0:
                    ghz.append(dmt / (drt * 10.0))
                    secs.append(drt * 1e-8)
        if not ghz:
            return None, 0.0, 0
        return float(np.median(ghz)), float(np.median(secs)), len(ghz)

    def set_option(self, name, value):
        """Kernel-selection switch of this engine (include/rtlws_hip.h: rtlws_engine_set_option)."""
        self._chk(hip_lib().rtlws_engine_set_option(self.h, name.encode(), int(value)), "set_option(%s)" % name)

    def get_option(self, name):
        return hip_lib().rtlws_engine_get_option(self.h, name.encode())

    def option(self, name, value):
        """Context manager: the option set to `value` inside the block, restored afterwards."""
        eng = self

        class _Scope:
            def __enter__(self_):
                self_.old = eng.get_option(name)
                eng.set_option(name, value)

            def __exit__(self_, *exc):
                eng.set_option(name, self_.old)
        return _Scope()

    def _chk(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed (rc=%d): %s" % (what, rc, last_error()))

    # -- kernels (device pointers: ints or DevBuf) --------------------------
    @staticmethod
    def _ptr(x):
        return x.ptr if isinstance(x, DevBuf) else int(x)

    def spectra_batch(self, desc, d_in, nframes, d_out, stream=None, check=True):
        rc = hip_lib().rtlws_spectra_batch(self.h, C.byref(desc), self._ptr(d_in), int(nframes),
                                           self._ptr(d_out), stream)
        if check:
            self._chk(rc, "rtlws_spectra_batch")
        return rc

    def spectra_batch_f64(self, desc, d_in, nframes, d_out, stream=None, check=True):
        rc = hip_lib().rtlws_spectra_batch_f64(self.h, C.byref(desc), self._ptr(d_in), int(nframes),
                                               self._ptr(d_out), stream)
        if check:
            self._chk(rc, "rtlws_spectra_batch_f64")
        return rc

    def cic_block_sums(self, R, d_src, dst_len, d_dst, stream=None, check=True):
        rc = hip_lib().rtlws_cic_block_sums(self.h, int(R), self._ptr(d_src), int(dst_len),
                                            self._ptr(d_dst), stream)
        if check:
            self._chk(rc, "rtlws_cic_block_sums")
        return rc

    def halfband(self, d_x, d_y, out_len, stream=None):
        self._chk(hip_lib().rtlws_halfband(self.h, self._ptr(d_x), self._ptr(d_y), int(out_len),
                                           stream), "rtlws_halfband")

    def grid(self, desc, nframes):
        return _outs(hip_lib().rtlws_spectra_grid, (self.h, C.byref(desc), int(nframes)), (C.c_int,) * 3)

    # -- what the host-in, host-out drivers below share ----------------------
    def _drive(self, plan, inputs, outputs, call):
        """One run from host arrays to host arrays, and whatever raises, every device buffer freed and `plan` (None: no
        plan) closed before it leaves.
        inputs: host arrays, each uploaded once however often it is given (an empty one: a 16-byte stub), or None (no
        buffer: a NULL pointer).  outputs: (dtype, shape), allocated and not initialised; or a preset host array,
        uploaded; or None (no buffer, None comes back).  Then call(inputs' buffers, outputs' buffers), sync, and the
        outputs downloaded -> their list; one of no bytes is not downloaded and comes back empty, or as it was preset.
        A shape with a negative count is no work here (a stub): the refusal a caller sees is the library's own."""
        made, by_id, d_out = [], {}, []

        def nbytes(o):
            if isinstance(o, np.ndarray):
                return o.nbytes
            count = np.dtype(o[0]).itemsize
            for n in o[1]:
                count *= max(int(n), 0)
            return count

        try:
            for x in inputs:
                if x is not None and id(x) not in by_id:
                    made.append(self.upload(x) if x.nbytes else self.alloc(16))
                    by_id[id(x)] = made[-1]
            for o in outputs:
                if o is not None:
                    made.append(self.upload(o) if isinstance(o, np.ndarray) and o.nbytes else self.alloc(nbytes(o) or 16))
                d_out.append(None if o is None else made[-1])
            call([None if x is None else by_id[id(x)] for x in inputs], d_out)
            self.sync()
            got = []
            for o, b in zip(outputs, d_out):
                if o is None or not nbytes(o):
                    got.append(o if o is None or isinstance(o, np.ndarray) else np.zeros(o[1], o[0]))
                else:
                    got.append(self.download(b, *((o.dtype, o.shape) if isinstance(o, np.ndarray) else o)))
            return got
        finally:
            try:
                if plan is not None:
                    plan.close()
            finally:
                for b in made:
                    b.free()

    @staticmethod
    def _frames_held(samples, t, m, hop):
        """the frames of T * M samples, hop apart, that a capture of `samples` holds"""
        return (samples - t * m) // hop + 1 if samples >= t * m and hop > 0 else 0

    @staticmethod
    def _captures(iqs, null=False):
        """several captures as uint8 [nsamples, 2] each; an array given twice stays one array, so that _drive uploads it
        once and its pointer is passed twice.  null: a None stays None (a NULL pointer among the captures); without it a
        None is converted like an array, which raises numpy's TypeError"""
        same = {id(x): np.ascontiguousarray(x, dtype=np.uint8).reshape(-1, 2) for x in iqs if not (null and x is None)}
        return [same.get(id(x)) for x in iqs]

    @staticmethod
    def _preset(count, fill, guard, dtype=np.float32):
        """a flat output of count elements preset to fill (None: zeros, and no guard), `guard` more behind them with a
        fill: a float32's value for float32, its bits for the integer types, float64(fill) for float64"""
        preset = np.float32(0.0 if fill is None else fill)
        value = preset.view(dtype) if np.dtype(dtype).kind in "iu" else dtype(preset)
        return np.full(count + (0 if fill is None else guard), value, dtype)

    @staticmethod
    def _rows(data, n_fft, k_avg, per_sample, output, f64_rows):
        """spectra*: the frames of n_fft samples of per_sample bytes that data holds, all of it -> (data, nframes, the
        rows as (dtype, shape))"""
        data = np.ascontiguousarray(data)
        nframes = data.nbytes // (per_sample * n_fft)
        assert nframes * per_sample * n_fft == data.nbytes
        dtype = np.uint8 if output == "payload_u8" else (np.float64 if f64_rows else np.float32)
        return data, nframes, (dtype, (nframes // k_avg, n_fft))

    # -- include/rtlws_fm.h: host arrays in, (audio, new state[, decimated samples]) out ----
    def _fm_run(self, call, src, nsamples, block_len, state, run_stage2, want_dec):
        nblocks = nsamples // block_len if block_len > 0 else 0
        assert block_len <= 0 or nblocks * block_len == nsamples
        state = np.ascontiguousarray(state, dtype=np.float32)
        assert state.size == FM_STATE_FLOATS
        naudio = max(nblocks * (block_len // 4), 0)
        d_src = self.upload(src) if src.nbytes else self.alloc(16)
        d_st = self.upload(np.concatenate([state, np.zeros(3, np.float32), np.zeros(FM_STATE_FLOATS, np.float32)]))
        d_audio = self.alloc(max(naudio, 1) * 4)
        d_dec = self.alloc(max(nsamples, 1) * 8) if want_dec else None
        try:
            rc = call(d_src.ptr, nblocks, d_st.ptr, d_st.ptr + 96, d_audio.ptr, d_dec.ptr if d_dec else None)
            if rc != 0:
                raise RuntimeError("rtlws_fm_audio_blocks failed (rc=%d): %s" % (rc, fm_last_error()))
            audio = self.download(d_audio, np.float32, (naudio,)) if run_stage2 and naudio else np.zeros(0, np.float32)
            new_state = self.download(d_st, np.float32, (24 + FM_STATE_FLOATS,))[24:]
            dec = self.download(d_dec, np.int32, (nsamples, 2)) if d_dec and nsamples else None
        finally:
            for b in (d_src, d_st, d_audio, d_dec):
                if b:
                    b.free()
        return (audio, new_state, dec) if want_dec else (audio, new_state)

    def fm_audio_blocks(self, iq, block_len, state, run_stage2=True):
        """rtlws_fm_audio_blocks: iq int32 [nblocks * block_len, 2], state f32[21] -> (audio f32, new state)."""
        iq = np.ascontiguousarray(iq, dtype=np.int32).reshape(-1, 2)
        return self._fm_run(lambda s, nb, si, so, a, d: fm_lib().rtlws_fm_audio_blocks(
            self.h, s, int(block_len), nb, si, so, int(bool(run_stage2)), a, None),
            iq, iq.shape[0], int(block_len), state, run_stage2, False)

    def fm_audio_blocks_cu8(self, iq, cic_r, block_len, state, run_stage2=True, want_dec=False):
        """rtlws_fm_audio_blocks_cu8: iq uint8 [nblocks * block_len * cic_r, 2] -> (audio, new state[, decimated int32])."""
        iq = np.ascontiguousarray(iq, dtype=np.uint8).reshape(-1, 2)
        n = iq.shape[0] // cic_r if cic_r > 0 else 0
        assert cic_r <= 0 or n * cic_r == iq.shape[0]
        return self._fm_run(lambda s, nb, si, so, a, d: fm_lib().rtlws_fm_audio_blocks_cu8(
            self.h, int(cic_r), s, int(block_len), nb, si, so, int(bool(run_stage2)), a, d, None),
            iq, n, int(block_len), state, run_stage2, want_dec)

    # -- include/rtlws_ddc.h: host arrays in, the bank's streams out ----
    def ddc(self, iq, cic_r, tuning_words, first_dec_index=0):
        """rtlws_ddc_run: iq uint8 [dec_len * cic_r, 2], one tuning word per channel -> int32 [C, dec_len, 2]."""
        iq = np.ascontiguousarray(iq, dtype=np.uint8).reshape(-1, 2)
        dec_len = iq.shape[0] // cic_r if cic_r > 0 else 0
        assert cic_r <= 0 or dec_len * cic_r == iq.shape[0]
        plan = DdcPlan(self)
        return self._drive(plan, [iq], [(np.int32, (len(tuning_words), dec_len, 2))], lambda i, o: plan.run(
            cic_r, i[0], dec_len, tuning_words, o[0], dec_len, first_dec_index))[0]

    # -- include/rtlws_ddcfir.h: host arrays in, the filtered bank's streams out ----
    def ddcfir(self, iq, decim, taps, tuning_words, out_shift=14, first_dec_index=0, dec_len=None):
        """rtlws_ddcfir_run: iq uint8 [(dec_len - 1) * decim + ntaps, 2] (dec_len: as many as iq holds), taps int16 [ntaps],
        one tuning word per channel -> int32 [C, dec_len, 2].  The capture is uploaded at exactly the samples needed."""
        iq = np.ascontiguousarray(iq, dtype=np.uint8).reshape(-1, 2)
        plan = DdcFirPlan(self, decim, taps)
        if dec_len is None:
            dec_len = (iq.shape[0] - plan.ntaps) // plan.decim + 1 if iq.shape[0] >= plan.ntaps else 0
        need = ddcfir_samples_needed(plan.decim, plan.ntaps, dec_len)
        assert 0 <= need <= iq.shape[0]
        return self._drive(plan, [iq[:need]], [(np.int32, (len(tuning_words), dec_len, 2))], lambda i, o: plan.run(
            i[0], dec_len, tuning_words, o[0], out_shift, dec_len, first_dec_index))[0]

    # -- include/rtlws_pfb.h: host arrays in, all channels out ----
    def pfb(self, iq, log2_channels, taps, hop=None, first_frame_index=0, layout="channel", nframes=None):
        """rtlws_pfb_run: iq uint8 [(nframes - 1) * hop + T * M, 2], taps int16 [T * M] -> complex64 [M, nframes]
        (layout "channel") or [nframes, M] ("time").  nframes None: as many as the capture holds."""
        iq = np.ascontiguousarray(iq, dtype=np.uint8).reshape(-1, 2)
        plan = PfbPlan(self, log2_channels, taps)
        m, t = 1 << plan.log2_channels, plan.taps_per_branch
        hop = m if hop is None else int(hop)
        if nframes is None:
            nframes = self._frames_held(iq.shape[0], t, m, hop)
        need = pfb_samples_needed(plan.log2_channels, t, hop, nframes)
        assert need < 0 or iq.shape[0] >= need, "the capture is shorter than rtlws_pfb_samples_needed"
        shape = (nframes, m) if _PFB_LAYOUTS.get(layout, layout) == PFB_TIME_MAJOR else (m, nframes)
        return self._drive(plan, [iq], [(np.complex64, shape)], lambda i, o: plan.run(
            i[0], nframes, o[0], hop, None, first_frame_index, layout))[0]

    # -- include/rtlws_pfbspec.h: host arrays in, one row per K frames out ----
    def pfbspec(self, iq, log2_channels, taps, k_avg, hop=None, output="power", shifted=False, scale=1.0, nspectra=None):
        """rtlws_pfbspec_run: iq uint8 [(nspectra * k_avg - 1) * hop + T * M, 2], taps int16 [T * M] -> float32
        [nspectra, M] ("power": the K-frame sums; "db": 10 log10(sum * scale / K)) or uint8 [nspectra, M] ("payload").
        nspectra None: as many as the capture holds."""
        iq = np.ascontiguousarray(iq, dtype=np.uint8).reshape(-1, 2)
        plan = PfbSpecPlan(self, log2_channels, taps)
        m, t, k_avg = 1 << plan.log2_channels, plan.taps_per_branch, int(k_avg)
        hop = m if hop is None else int(hop)
        if nspectra is None:
            nspectra = self._frames_held(iq.shape[0], t, m, hop) // k_avg if k_avg > 0 else 0
        need = pfbspec_samples_needed(plan.log2_channels, t, hop, k_avg, nspectra)
        assert need < 0 or iq.shape[0] >= need, "the capture is shorter than rtlws_pfbspec_samples_needed"
        dtype = np.uint8 if _PFBSPEC_OUTPUTS.get(output, output) == OUT_PAYLOAD_U8 else np.float32
        return self._drive(plan, [iq], [(dtype, (nspectra, m))], lambda i, o: plan.run(
            i[0], nspectra, k_avg, o[0], hop, output, shifted, scale))[0]

    # -- include/rtlws_pfbsk.h: host arrays in, (clean rows, kept counts[, S1 rows, S2 rows]) out ----
    def pfbsk(self, iq, log2_channels, taps, k_avg, nsub, ratio_lo=0.0, ratio_hi=float("inf"), power_scale=None, hop=None,
              output="power", shifted=False, scale=1.0, nspectra=None, sub_rows=False):
        """rtlws_pfbsk_run: iq uint8 [(nspectra * nsub * k_avg - 1) * hop + T * M, 2], taps int16 [T * M] -> (float32
        [nspectra, M] ("power": the sums over the kept sub-integrations; "db") or uint8 [nspectra, M] ("payload"),
        uint32 [nspectra, M] the numbers kept) and, with sub_rows, float32 [nspectra * nsub, M] S1 and S2 behind them.
        power_scale None: rtlws_pfbsk_power_scale's.  nspectra None: as many as the capture holds."""
        iq = np.ascontiguousarray(iq, dtype=np.uint8).reshape(-1, 2)
        plan = PfbSkPlan(self, log2_channels, taps)
        m, t, k_avg, nsub = 1 << plan.log2_channels, plan.taps_per_branch, int(k_avg), int(nsub)
        hop = m if hop is None else int(hop)
        if power_scale is None:
            power_scale = pfbsk_power_scale(plan.log2_channels, taps)
        if nspectra is None:
            nspectra = self._frames_held(iq.shape[0], t, m, hop) // (k_avg * nsub) if k_avg > 0 and nsub > 0 else 0
        need = pfbsk_samples_needed(plan.log2_channels, t, hop, k_avg, nsub, nspectra)
        assert need < 0 or iq.shape[0] >= need, "the capture is shorter than rtlws_pfbsk_samples_needed"
        dtype = np.uint8 if _PFBSPEC_OUTPUTS.get(output, output) == OUT_PAYLOAD_U8 else np.float32
        shapes = [(dtype, (nspectra, m)), (np.uint32, (nspectra, m))] + [(np.float32, (nspectra * max(nsub, 0), m))] * (2 if sub_rows else 0)
        return tuple(self._drive(plan, [iq], shapes, lambda i, o: plan.run(
            i[0], nspectra, k_avg, nsub, power_scale, o[0], ratio_lo, ratio_hi, *o[1:], hop=hop, output=output, shifted=shifted,
            scale=scale)))

    # -- include/rtlws_dedisp.h: host rows in, one time series per trial out ----
    def dedisp(self, rows, delays, mask=None, nout=None, in_stride=None, out_stride=None, fill=None):
        """rtlws_dedisp_run: rows float32 [nrows, nchan] (with in_stride: [nrows, in_stride], the padding as the caller
        left it), delays int32 [ntrials, nchan], mask uint8 [nchan] or None -> float32 [ntrials, nout].  nout None: as
        many as the rows hold.  With out_stride the whole buffer [ntrials, out_stride] comes back, every element preset
        to `fill` (a float32; None: zeros), so that a caller sees what the run left untouched."""
        plan = DedispPlan(self, delays, mask)
        width = plan.nchan if in_stride is None else int(in_stride)
        rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, width)
        if nout is None:
            nout = max(rows.shape[0] - (plan.rows_needed(1) - 1), 0)
        nout = int(nout)
        assert rows.shape[0] >= plan.rows_needed(nout), "fewer rows than rtlws_dedisp_rows_needed"
        stride = nout if out_stride is None else int(out_stride)
        host = np.full((plan.ntrials, max(stride, 0)), 0.0 if fill is None else fill, np.float32)
        out, = self._drive(plan, [rows], [host], lambda i, o: plan.run(i[0], nout, o[0], width, stride))
        return out if out_stride is not None else out[:, :nout]

    # -- what the searches over series share: the shaped, padded series; the preset buffers, the run and the download ----
    @staticmethod
    def _series(series, in_stride, what="nsamp"):
        """series as float32 [ntrials, width] (with in_stride: rows of in_stride elements, the padding as the caller left
        it; without: zeros behind the samples up to a multiple of 4, the library's stride) -> (the array, its samples)"""
        series = np.ascontiguousarray(series, dtype=np.float32)
        if in_stride is not None:
            series = series.reshape(-1, int(in_stride))
        assert series.ndim == 2, "the series are [ntrials, %s]" % what
        samples = series.shape[1]
        if in_stride is None and samples % 4:
            series = np.concatenate([series, np.zeros((series.shape[0], -samples % 4), np.float32)], axis=1)
        return series, samples

    def _search(self, plan, call, series, nsamp, lead_shape, want_power, want_white, fill):
        """call(d_in, in_stride, ntrials, nsamp, d_best, d_at, d_power, d_white) of `plan` over the uploaded series into
        preset buffers, the plan closed behind it -> (best, at, power, white) with lead_shape in front of [levels, nseg]
        and [M]; an optional row that is neither wanted nor preset is not allocated and comes back None.  With `fill` the
        four whole flat buffers, PERIOD_GUARD elements longer than the outputs, every element preset to fill."""
        ntrials, width = series.shape
        nv = int(np.prod(lead_shape))
        npeaks, nrows = nv * plan.levels * plan.nseg, nv * plan.nbins
        hosts = [self._preset(npeaks, fill, PERIOD_GUARD), self._preset(npeaks, fill, PERIOD_GUARD, np.int32),
                 self._preset(nrows if want_power or fill is not None else 0, fill, PERIOD_GUARD),
                 self._preset(nrows if want_white or fill is not None else 0, fill, PERIOD_GUARD)]
        got = self._drive(plan, [series], [h if h.size else None for h in hosts], lambda i, o: call(
            i[0], width, ntrials, nsamp, o[0], o[1], o[2] if want_power else None, o[3] if want_white else None))
        best, at, power, white = [h if g is None else g for g, h in zip(got, hosts)]
        if fill is not None:
            return best, at, power, white
        shape = tuple(lead_shape) + (plan.levels, plan.nseg)
        return (best.reshape(shape), at.reshape(shape), power.reshape(tuple(lead_shape) + (plan.nbins,)) if want_power else None,
                white.reshape(tuple(lead_shape) + (plan.nbins,)) if want_white else None)

    # -- include/rtlws_pulse.h: host series in, (peaks, places, moments) out ----
    def pulse(self, series, widths, seg, nout=None, in_stride=None, want_moments=True, fill=None):
        """rtlws_pulse_run: series float32 [ntrials, nsamples] (with in_stride: [ntrials, in_stride], the padding as the
        caller left it), widths int32 [nwidths] -> (float32 [ntrials, nwidths, nseg] the peaks, int32 of that shape
        their places, float64 [ntrials, nseg, 2] the moments, or None without want_moments).  nout None: as many as the
        samples hold.  With `fill` (a float32) the three come back as the whole flat buffers, PULSE_GUARD elements
        longer than the outputs, every element preset to fill (peaks), to fill's bits (places) and to float64(fill)
        (moments), so that a caller sees what the run left untouched; without want_moments the run gets a NULL d_mom and
        the preset moments buffer comes back as it was."""
        plan = PulsePlan(self, widths, seg)
        series, samples = self._series(series, in_stride, "nsamples")
        ntrials, width = series.shape
        if nout is None:
            nout = max(samples - (plan.samples_needed(1) - 1), 0)
        nout = int(nout)
        assert samples >= plan.samples_needed(nout), "fewer samples than rtlws_pulse_samples_needed"
        nseg = plan.segments(nout)
        hosts = [self._preset(ntrials * plan.nwidths * nseg, fill, PULSE_GUARD),
                 self._preset(ntrials * plan.nwidths * nseg, fill, PULSE_GUARD, np.int32),
                 self._preset(ntrials * nseg * 2, fill, PULSE_GUARD, np.float64)]
        peak, at, mom = self._drive(plan, [series], hosts, lambda i, o: plan.run(
            i[0], width, ntrials, nout, o[0], o[1], o[2] if want_moments else None))
        if fill is not None:
            return peak, at, mom
        return (peak.reshape(ntrials, plan.nwidths, nseg), at.reshape(ntrials, plan.nwidths, nseg),
                mom.reshape(ntrials, nseg, 2) if want_moments else None)

    # -- include/rtlws_fold.h: host series in, (profiles, hits) out ----
    def fold(self, series, steps, phases, nbins, sub, nsamp=None, in_stride=None, want_hits=True, fill=None):
        """rtlws_fold_run: series float32 [ntrials, nsamp] (with in_stride: [ntrials, in_stride], the padding as the caller
        left it), steps and phases uint64 [nperiods] -> (float32 [ntrials, nperiods, nsub, nbins] the profiles, uint32
        [nperiods, nsub, nbins] the hits, or None without want_hits).  nsamp None: the samples the series hold.  With
        `fill` (a float32) the two come back as the whole flat buffers, FOLD_GUARD elements longer than the outputs,
        every element preset to fill (profiles) and to fill's bits (hits), so that a caller sees what the run left
        untouched; without want_hits the run gets a NULL d_hits and the preset hits buffer comes back as it was."""
        plan = FoldPlan(self, steps, phases, nbins, sub)
        series, samples = self._series(series, in_stride)
        ntrials, width = series.shape
        nsamp = samples if nsamp is None else int(nsamp)
        assert samples >= nsamp, "fewer samples than nsamp"
        nsub = plan.subints(nsamp)
        hosts = [self._preset(ntrials * plan.nperiods * nsub * plan.nbins, fill, FOLD_GUARD),
                 self._preset(plan.nperiods * nsub * plan.nbins, fill, FOLD_GUARD, np.uint32)]
        prof, hits = self._drive(plan, [series], hosts, lambda i, o: plan.run(
            i[0], width, ntrials, nsamp, o[0], o[1] if want_hits else None))
        if fill is not None:
            return prof, hits
        return (prof.reshape(ntrials, plan.nperiods, nsub, plan.nbins),
                hits.reshape(plan.nperiods, nsub, plan.nbins) if want_hits else None)

    # -- include/rtlws_period.h: host series in, (best, at, power, white) out ----
    def period(self, series, log2n, levels, norm, seg, klo, nsamp=None, in_stride=None, want_rows=True, fill=None):
        """rtlws_period_run: series float32 [ntrials, nsamp] (with in_stride: [ntrials, in_stride], the padding as the
        caller left it) -> (float32 [ntrials, levels, nseg] the peaks, int32 of that shape their bins, float32
        [ntrials, M] the power spectra and the whitened ones, or None for both without want_rows).  nsamp None: the
        samples the series hold.  With `fill` (a float32) the four come back as the whole flat buffers, PERIOD_GUARD
        elements longer than the outputs, every element preset to fill (to fill's bits: the bins), so that a caller sees
        what the run left untouched; without want_rows the run gets NULL rows and the preset buffers come back as they
        were."""
        plan = PeriodPlan(self, log2n, levels, norm, seg, klo)
        series, samples = self._series(series, in_stride)
        nsamp = samples if nsamp is None else int(nsamp)
        assert samples >= nsamp, "fewer samples than nsamp"
        return self._search(plan, plan.run, series, nsamp, (series.shape[0],), want_rows, want_rows, fill)

    # -- include/rtlws_periodlong.h: host series in, (best, at, power, white) out ----
    def periodlong(self, series, log2n, levels, norm, seg, klo, nsamp=None, in_stride=None, want_rows=True, fill=None, max_trials=None,
                   want_power=None, want_white=None):
        """rtlws_periodlong_run with Engine.period's arguments and results.  max_trials: what the plan is opened for (None:
        the trials given); want_power / want_white: one optional row alone (None: want_rows)."""
        series, samples = self._series(series, in_stride)
        ntrials = series.shape[0]
        plan = PeriodLongPlan(self, log2n, levels, norm, seg, klo, ntrials if max_trials is None else max_trials)
        nsamp = samples if nsamp is None else int(nsamp)
        assert samples >= nsamp, "fewer samples than nsamp"
        return self._search(plan, plan.run, series, nsamp, (ntrials,), want_rows if want_power is None else want_power,
                            want_rows if want_white is None else want_white, fill)

    # -- include/rtlws_accel.h: host series in, (best, at, power, white) out with a leading [ntrials, naccel] ----
    def accel_search(self, series, log2n, levels, norm, seg, klo, coefs, nsamp=None, in_stride=None, want_rows=True, fill=None,
                     max_trials=None, want_power=None, want_white=None):
        """rtlws_accel_search with Engine.periodlong's arguments and, over the ntrials * naccel virtual trials, its
        results: (float32 [ntrials, naccel, levels, nseg] the peaks, int32 of that shape their bins, float32 [ntrials,
        naccel, M] the power spectra and the whitened ones, or None).  max_trials counts virtual trials (None: all of
        them).  With `fill` the four come back as the whole flat buffers, PERIOD_GUARD elements longer than the outputs."""
        series, samples = self._series(series, in_stride)
        nsamp = samples if nsamp is None else int(nsamp)
        assert samples >= nsamp, "fewer samples than nsamp"
        ntrials, naccel = series.shape[0], np.asarray(coefs).size
        plan = AccelPlan(self, log2n, levels, norm, seg, klo, coefs, ntrials * naccel if max_trials is None else max_trials)
        return self._search(plan, plan.search, series, nsamp, (ntrials, naccel), want_rows if want_power is None else want_power,
                            want_rows if want_white is None else want_white, fill)

    def accel_resample(self, series, log2n, coefs, a_first=0, a_count=None, nsamp=None, in_stride=None, out_stride=None, fill=None):
        """rtlws_accel_resample: series float32 [ntrials, nsamp] (with in_stride: [ntrials, in_stride], the padding as the
        caller left it), coefs int64 [naccel] -> float32 [ntrials, a_count, nsamp], the series read through the maps of
        accelerations a_first .. a_first + a_count - 1 (a_count None: the rest of the table).  out_stride None: nsamp
        rounded up to a multiple of 4.  With `fill` (a float32) the whole flat buffer comes back, [ntrials * a_count *
        out_stride + PERIOD_GUARD] elements preset to fill, so that a caller sees what the run left untouched."""
        series, samples = self._series(series, in_stride)
        nsamp = samples if nsamp is None else int(nsamp)
        assert samples >= nsamp, "fewer samples than nsamp"
        ntrials, width = series.shape
        naccel = np.asarray(coefs).size
        a_count = naccel - int(a_first) if a_count is None else int(a_count)
        out_stride = (nsamp + 3) // 4 * 4 if out_stride is None else int(out_stride)
        plan = AccelPlan(self, log2n, 1, PERIODLONG_MIN_NORM, PERIODLONG_MIN_SEG, 1, coefs)
        host = np.full(ntrials * a_count * out_stride + PERIOD_GUARD, np.float32(0.0 if fill is None else fill), np.float32)
        out, = self._drive(plan, [series], [host], lambda i, o: plan.resample(
            i[0], width, ntrials, nsamp, a_first, a_count, o[0], out_stride))
        if fill is not None:
            return out
        return out[:ntrials * a_count * out_stride].reshape(ntrials, a_count, out_stride)[:, :, :nsamp]

    # -- include/rtlws_pfbxc.h: host arrays in, (auto rows, cross rows) out ----
    def pfbxc(self, iqs, log2_channels, taps, k_avg, hop=None, shifted=False, nspectra=None):
        """rtlws_pfbxc_run: iqs a sequence of A = 2 .. 4 captures, each uint8 [(nspectra * k_avg - 1) * hop + T * M, 2]
        (one array may be given twice: it is uploaded once and its pointer passed twice), taps int16 [T * M] ->
        (float32 [nspectra, A, M], the K-frame powers; complex64 [nspectra, A (A - 1) / 2, M], the K-frame
        cross-spectra of the pairs a < b row-major).  nspectra None: as many as the shortest capture holds."""
        iqs = self._captures(iqs, null=True)
        a = len(iqs)
        plan = PfbXcPlan(self, log2_channels, taps, a)
        nx = a * (a - 1) // 2
        m, t, k_avg = 1 << plan.log2_channels, plan.taps_per_branch, int(k_avg)
        hop = m if hop is None else int(hop)
        shortest = min(x.shape[0] for x in iqs if x is not None)
        if nspectra is None:
            nspectra = self._frames_held(shortest, t, m, hop) // k_avg if k_avg > 0 else 0
        need = pfbxc_samples_needed(plan.log2_channels, t, hop, k_avg, nspectra)
        assert need < 0 or shortest >= need, "a capture is shorter than rtlws_pfbxc_samples_needed"
        autos, cross = self._drive(plan, iqs, [(np.float32, (nspectra, a, m)), (np.complex64, (nspectra, nx, m))],
                                   lambda i, o: plan.run(i, nspectra, k_avg, o[0], o[1], hop, shifted))
        return autos, cross

    # -- include/rtlws_pfbbf.h: host arrays in, the beams out ----
    def _pfbbf_inputs(self, iqs, weights, log2_channels, taps):
        """-> (plan, the captures, the weights complex64 [B, A, M], the shortest capture's samples)"""
        iqs = self._captures(iqs)
        weights = np.ascontiguousarray(weights, dtype=np.complex64)
        assert weights.ndim == 3 and weights.shape[1:] == (len(iqs), 1 << int(log2_channels)), "the weights are [B, A, M]"
        return PfbBfPlan(self, log2_channels, taps, len(iqs), weights.shape[0]), iqs, weights, min(x.shape[0] for x in iqs)

    def pfbbf(self, iqs, weights, log2_channels, taps, hop=None, first_frame_index=0, layout="channel", nframes=None):
        """rtlws_pfbbf_run: iqs a sequence of A = 1 .. 8 captures, each uint8 [(nframes - 1) * hop + T * M, 2], weights
        complex64 [B, A, M], taps int16 [T * M] -> complex64 [B, M, nframes] (layout "channel") or [B, nframes, M]
        ("time").  nframes None: as many as the shortest capture holds."""
        plan, iqs, weights, shortest = self._pfbbf_inputs(iqs, weights, log2_channels, taps)
        m, t, nb = 1 << plan.log2_channels, plan.taps_per_branch, plan.nbeams
        hop = m if hop is None else int(hop)
        if nframes is None:
            nframes = self._frames_held(shortest, t, m, hop)
        need = pfbbf_samples_needed(plan.log2_channels, t, hop, 0, nframes)
        assert need < 0 or shortest >= need, "a capture is shorter than rtlws_pfbbf_samples_needed"
        shape = (nb, nframes, m) if _PFB_LAYOUTS.get(layout, layout) == PFB_TIME_MAJOR else (nb, m, nframes)
        return self._drive(plan, iqs + [weights], [(np.complex64, shape)], lambda i, o: plan.run(
            i[:-1], i[-1], nframes, o[0], hop, None, None, first_frame_index, layout))[0]

    def pfbbf_power(self, iqs, weights, log2_channels, taps, k_avg, hop=None, shifted=False, nspectra=None):
        """rtlws_pfbbf_power: the captures and weights of pfbbf, each capture uint8 [(nspectra * k_avg - 1) * hop +
        T * M, 2] -> float32 [nspectra, B, M], the K-frame powers of the beams.  nspectra None: as many as the shortest
        capture holds."""
        plan, iqs, weights, shortest = self._pfbbf_inputs(iqs, weights, log2_channels, taps)
        m, t, nb, k_avg = 1 << plan.log2_channels, plan.taps_per_branch, plan.nbeams, int(k_avg)
        hop = m if hop is None else int(hop)
        if nspectra is None:
            nspectra = self._frames_held(shortest, t, m, hop) // k_avg if k_avg > 0 else 0
        need = pfbbf_samples_needed(plan.log2_channels, t, hop, k_avg, nspectra) if k_avg > 0 else -1
        assert need < 0 or shortest >= need, "a capture is shorter than rtlws_pfbbf_samples_needed"
        return self._drive(plan, iqs + [weights], [(np.float32, (nspectra, nb, m))], lambda i, o: plan.power(
            i[:-1], i[-1], nspectra, k_avg, o[0], hop, shifted))[0]

    # -- include/rtlws_fmbank.h: host arrays in, (audio, new states) out ----
    def fm_bank(self, iq, cic_r, tuning_words, block_len, states, first_dec_index=0):
        """rtlws_fmbank_run: iq uint8 [nblocks * block_len * cic_r, 2], one tuning word and one state f32[21] per
        channel -> (audio f32 [C, nblocks * quarter], new states f32 [C, 21])."""
        iq = np.ascontiguousarray(iq, dtype=np.uint8).reshape(-1, 2)
        nch = len(tuning_words)
        states = np.ascontiguousarray(states, dtype=np.float32).reshape(nch, FM_STATE_FLOATS)
        per_block = int(block_len) * int(cic_r)
        nblocks = iq.shape[0] // per_block if per_block > 0 else 0
        assert per_block <= 0 or nblocks * per_block == iq.shape[0]
        n = max(nblocks * (int(block_len) // 4), 0)
        plan = FmBankPlan(self)
        new_states, audio = self._drive(plan, [iq, states], [(np.float32, states.shape), (np.float32, (nch, n))], lambda i, o: plan.run(
            cic_r, i[0], block_len, nblocks, tuning_words, i[1], o[0], o[1], n, first_dec_index))
        return audio, new_states

    # -- include/rtlws_fmfir.h: host arrays in, (audio, new states) out ----
    def fm_fir_bank(self, iq, decim, taps, tuning_words, block_len, states, out_shift=14, first_dec_index=0):
        """rtlws_fmfir_run: iq uint8 [(nblocks * block_len - 1) * decim + ntaps, 2] (as many blocks as iq holds), taps
        int16 [ntaps], one tuning word and one state f32[21] per channel -> (audio f32 [C, nblocks * quarter], new states
        f32 [C, 21]).  The capture is uploaded at exactly the samples needed."""
        iq = np.ascontiguousarray(iq, dtype=np.uint8).reshape(-1, 2)
        nch = len(tuning_words)
        states = np.ascontiguousarray(states, dtype=np.float32).reshape(nch, FM_STATE_FLOATS)
        plan = FmFirPlan(self, decim, taps)
        dec_len = (iq.shape[0] - plan.ntaps) // plan.decim + 1 if iq.shape[0] >= plan.ntaps else 0
        nblocks = dec_len // int(block_len) if block_len > 0 else 0
        need = fmfir_samples_needed(plan.decim, plan.ntaps, block_len, nblocks)
        assert 0 <= need <= iq.shape[0]
        n = max(int(nblocks) * (int(block_len) // 4), 0)
        new_states, audio = self._drive(plan, [iq[:need], states], [(np.float32, states.shape), (np.float32, (nch, n))], lambda i, o: plan.run(
            i[0], block_len, nblocks, tuning_words, i[1], o[0], o[1], out_shift, n, first_dec_index))
        return audio, new_states

    # -- convenience: host arrays in, host arrays out ------------------------
    def spectra(self, data, n_fft, k_avg=1, input="cu8", window="rect", output="power_sum",
                cic_r=0, gain_db=0, f64=False, rows_f32=False):
        """f64=True: rtlws_spectra_batch_f64 (the reference-precision kernels, f64 rows;
        rows_f32=True: the same arithmetic with rows rounded once to f32, RTLWS_FLAG_ROWS_F32)."""
        desc = make_desc(n_fft, k_avg, input, window, output, cic_r, gain_db,
                         FLAG_ROWS_F32 if (f64 and rows_f32) else 0)
        data, nframes, rows = self._rows(data, n_fft, k_avg, _SAMPLE_BYTES[input] * max(int(cic_r), 1), output, f64 and not rows_f32)
        batch = self.spectra_batch_f64 if f64 else self.spectra_batch
        return self._drive(None, [data], [rows], lambda i, o: batch(desc, i[0], nframes, o[0]))[0]

    def _spectra_plan(self, cls, desc, data, input, output, max_frames):
        """spectra_long and spectra_anylen: the plan of `cls` for the frames data holds, run over all of them"""
        data, nframes, rows = self._rows(data, desc.n_fft, desc.k_avg, _SAMPLE_BYTES[input], output, not desc.flags & FLAG_ROWS_F32)
        plan = cls(self, desc, nframes if max_frames is None else max_frames)
        return self._drive(plan, [data], [rows], lambda i, o: plan.run(i[0], nframes, o[0]))[0]

    def spectra_long(self, data, n_fft, k_avg=1, input="cu8", output="power_sum", gain_db=0, rows_f32=False,
                     max_frames=None):
        """Engine.spectra for 2^14 .. 2^20-point frames (include/rtlws_long.h): host arrays in, f64 rows out
        (rows_f32=True: the same arithmetic, rows rounded once to f32).  max_frames: the plan's group size
        (default: the whole batch)."""
        desc = make_desc(n_fft, k_avg, input, "rect", output, 0, gain_db, FLAG_ROWS_F32 if rows_f32 else 0)
        return self._spectra_plan(LongPlan, desc, data, input, output, max_frames)

    def spectra_anylen(self, data, n_fft, k_avg=1, input="cu8", output="power_sum", gain_db=0, rows_f32=False,
                       max_frames=None):
        """Engine.spectra_long for any frame length 2 .. 2^19 (include/rtlws_anylen.h).  The device buffers are
        exactly as long as the frames and the rows: nothing lies behind the last frame."""
        desc = make_desc(n_fft, k_avg, input, "rect", output, 0, gain_db, FLAG_ROWS_F32 if rows_f32 else 0)
        return self._spectra_plan(AnyLenPlan, desc, data, input, output, max_frames)


# ---- drop-in API (librtlws_amd.so) -----------------------------------------

class Spectrum:
    """struct spectrum* of include/spectrum.h."""

    def __init__(self, N):
        self.N = N
        self.h = amd_lib().spectrum_alloc(int(N))
        if not self.h:
            raise RuntimeError("spectrum_alloc(%d) returned NULL: %s" % (N, last_error()))

    def add_cmplx_u8(self, src, ps, length=None):
        src = np.ascontiguousarray(src, dtype=np.uint8)
        return amd_lib().spectrum_add_cmplx_u8(self.h, _p(src), _p(ps),
                                               self.N if length is None else length)

    def add_cmplx_s32(self, src, ps, length=None):
        src = np.ascontiguousarray(src, dtype=np.int32)
        return amd_lib().spectrum_add_cmplx_s32(self.h, _p(src), _p(ps),
                                                self.N if length is None else length)

    def add_real_f32(self, src, ps, length=None):
        src = np.ascontiguousarray(src, dtype=np.float32)
        return amd_lib().spectrum_add_real_f32(self.h, _p(src), _p(ps),
                                               self.N if length is None else length)

    def free(self):
        if self.h:
            amd_lib().spectrum_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def cic_decimate(R, src, state=None, dst_len=None):
    """include/resample.h cic_decimate. Returns (rc, dst int32[dst_len,2], state int32[4])."""
    src = np.ascontiguousarray(src, dtype=np.uint8).reshape(-1, 2)
    src_len = src.shape[0]
    if dst_len is None:
        dst_len = src_len // R if R > 0 else 0
    dst = np.zeros((max(dst_len, 0), 2), dtype=np.int32)
    st = [0, 0, 0, 0] if state is None else [int(x) for x in state]
    d = CicDelayLine(CmplxS32(st[0], st[1]), CmplxS32(st[2], st[3]))
    rc = amd_lib().cic_decimate(int(R), _p(src), src_len, _p(dst), dst_len, C.byref(d))
    out_state = np.array([d.integrator_prev_out.re, d.integrator_prev_out.im,
                          d.comb_prev_in.re, d.comb_prev_in.im], dtype=np.int32)
    return rc, dst, out_state


def halfband_decimate(inp, delay):
    inp = np.ascontiguousarray(inp, dtype=np.float32)
    assert delay.dtype == np.float32 and delay.size == 10
    out = np.empty(inp.size // 2, dtype=np.float32)
    amd_lib().halfband_decimate(_p(inp), _p(out), out.size, _p(delay))
    return out


_RF_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int)


class RfDecimator:
    """struct rf_decimator* of include/rf_decimator.h; callback blocks are collected."""

    def __init__(self):
        self.h = amd_lib().rf_decimator_alloc()
        self.blocks = []

        def _cb(ptr, n):
            a = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int32)), shape=(n, 2))
            self.blocks.append(a.copy())

        self._cb = _RF_CB(_cb)
        amd_lib().rf_decimator_add_callback(self.h, C.cast(self._cb, C.c_void_p))

    def set_parameters(self, sample_rate, down_factor):
        return amd_lib().rf_decimator_set_parameters(self.h, float(sample_rate), int(down_factor))

    def decimate(self, iq):
        iq = np.ascontiguousarray(iq, dtype=np.uint8).reshape(-1, 2)
        return amd_lib().rf_decimator_decimate_cmplx_u8(self.h, _p(iq), iq.shape[0])

    def free(self):
        if self.h:
            amd_lib().rf_decimator_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---- include/rtlws_multi.h ----------------------------------------------------

class MultiShardStats(C.Structure):
    _fields_ = [("device", C.c_int), ("first_frame", C.c_long), ("frames", C.c_long), ("launches", C.c_int),
                ("event_ms", C.c_double), ("wall_ms", C.c_double), ("rc", C.c_int)]


def multi_partition(nframes, k_avg, shards, g):
    """rtlws_multi_partition: (rc, first_frame, frame_count).  No GPU needed."""
    a, b = C.c_long(-1), C.c_long(-1)
    rc = amd_lib().rtlws_multi_partition(int(nframes), int(k_avg), int(shards), int(g), C.byref(a), C.byref(b))
    return rc, a.value, b.value


class MultiBatch:
    """rtlws_multi*: one batch sharded over devices (device_ids: one shard per entry; None = every device)."""

    def __init__(self, desc, nframes, device_ids=None, f64=False):
        L = amd_lib()
        n = 0 if device_ids is None else len(device_ids)
        ids = None if device_ids is None else (C.c_int * n)(*device_ids)
        self.desc, self.f64 = desc, f64
        self.h = L.rtlws_multi_open(n, ids, C.byref(desc), int(nframes), 1 if f64 else 0)
        if not self.h:
            raise RuntimeError("rtlws_multi_open failed: %s" % (L.rtlws_multi_error(None).decode() or last_error()))
        self.shards = L.rtlws_multi_shards(self.h)
        self.frames = L.rtlws_multi_frames(self.h)

    def upload(self, frames):
        frames = np.ascontiguousarray(frames)
        assert frames.nbytes >= self.frames * amd_lib().rtlws_multi_frame_bytes(self.h)
        rc = amd_lib().rtlws_multi_upload(self.h, _p(frames))
        if rc:
            raise RuntimeError("rtlws_multi_upload rc=%d: %s" % (rc, self.error()))

    def run(self, launches=1):
        st = (MultiShardStats * self.shards)()
        wall = C.c_double(0.0)
        rc = amd_lib().rtlws_multi_run(self.h, int(launches), st, C.byref(wall))
        if rc:
            raise RuntimeError("rtlws_multi_run rc=%d: %s" % (rc, self.error()))
        return list(st), wall.value

    def download(self):
        rows = self.frames // self.desc.k_avg
        rb = amd_lib().rtlws_multi_row_bytes(self.h)
        dt = np.uint8 if self.desc.output == OUT_PAYLOAD_U8 else {4: np.float32, 8: np.float64}[rb // self.desc.n_fft]
        out = np.empty((rows, self.desc.n_fft), dtype=dt)
        rc = amd_lib().rtlws_multi_download(self.h, _p(out))
        if rc:
            raise RuntimeError("rtlws_multi_download rc=%d: %s" % (rc, self.error()))
        return out

    def error(self):
        """why the last upload / run / download failed (the failing call ran on a shard's own thread)"""
        return amd_lib().rtlws_multi_error(self.h).decode()

    def topology(self, g):
        """(TopoInfo, cpus the shard's thread pinned itself to) of shard g"""
        t, n = TopoInfo(), C.c_int(0)
        if amd_lib().rtlws_multi_shard_topology(self.h, int(g), C.byref(t), C.byref(n)) != 0:
            raise IndexError(g)
        return t, n.value

    def close(self):
        if self.h:
            amd_lib().rtlws_multi_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def topo_describe(device=-1, bus_id=None, sysfs_root=None):
    """rtlws_topo_describe: TopoInfo of a device (bus_id given: no GPU is asked).  None on bad arguments."""
    t = TopoInfo()
    rc = amd_lib().rtlws_topo_describe(int(device), None if bus_id is None else bus_id.encode(),
                                       None if sysfs_root is None else str(sysfs_root).encode(), C.byref(t))
    return t if rc == 0 else None


# ---- boundary #2 (librtlws_cbb.so over the synthetic sensor) ------------------

def cbb_lib():
    """cbb_main.h entry points.  The sensor / signal-source symbols they need
    come from librtlws_synth.so here (in rtl-ws they come from the server's own
    rtl_sensor.c / signal_source.c)."""
    global _cbb
    if _cbb is None:
        amd_lib()
        _need(SYNTH_LIB)
        _need(CBB_LIB)
        C.CDLL(SYNTH_LIB, mode=C.RTLD_GLOBAL)
        L = C.CDLL(CBB_LIB)
        L.cbb_init.argtypes = [C.c_int]
        L.cbb_init.restype = None
        L.cbb_rf_decimator.restype = C.c_void_p
        L.cbb_get_rtl_dev.restype = C.c_void_p
        L.cbb_new_spectrum_available.restype = C.c_int
        L.cbb_get_spectrum_payload.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.cbb_get_spectrum_payload.restype = C.c_int
        L.cbb_close.restype = None
        L.rtlws_cbb_samples_seen.restype = C.c_uint64
        _cbb = L
    return _cbb


def cbb_payload(gain_db, buf_len=8192):
    buf = np.zeros(buf_len, dtype=np.uint8)
    n = cbb_lib().cbb_get_spectrum_payload(_p(buf), buf_len, int(gain_db))
    return buf[:n].copy()
