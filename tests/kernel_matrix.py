"""A model of the spectrum launch tables: which template instantiation a descriptor launches.

Restated from rtl-ws_amd/csrc (no GPU, no build needed):
  shim.hip ........... plan_f32, plan_f64, cic_in_kind, use_v2
  rtlws_internal.h ... cicr_kind and friends, fused_kone_kind, f64_fused_kind, the Flag<> rule
  spectrum_fused.hip / spectrum_fused_v2.hip / spectrum_f64_fused.hip (f64f_table) /
  spectrum_f64_1024x.hip (x_table) / spectrum_f64.hip / spectrum_direct.hip ... the pick() nests

CASES lists descriptors (plus the engine options they need) that together reach every instantiation the
code objects hold, one case per instantiation where it can, and a few more for the runtime-only fields of the
row-per-workgroup kernels.  tests/test_kernel_matrix_cpu.py holds the model to the built library,
tests/test_kernel_matrix_gpu.py runs every case against the f64 oracle.
"""
from collections import namedtuple

# rtlws_internal.h: the kernels' input kinds
(IN_CU8, IN_CS32, IN_RF32, IN_CU8_CIC8, IN_CU8_CICR2, IN_CU8_CICR4, IN_CU8_CICR8, IN_CU8_CICR16,
 IN_CU8_CICR_LDS4, IN_CU8_CICR_LDS2, IN_CU8_CICR_LDS1, IN_CU8_CIC10, IN_CU8_CIC12) = range(13)
OUT_SUM, OUT_DB, OUT_PAYLOAD = 0, 1, 2
INPUTS = {"cu8": IN_CU8, "cs32": IN_CS32, "rf32": IN_RF32}
OUTPUTS = {"power_sum": OUT_SUM, "mean_db": OUT_DB, "payload_u8": OUT_PAYLOAD}
FUSED_N = (1024, 2048, 4096)
CICR_LDS_WAVE_BYTES = 9216

# shim.hip kOptions: the defaults of the options a case may set
DEFAULT_OPTS = {"v2": -1, "f64_fused": 1, "f64_x1024": 1, "f64_x_waves": 0, "cic_direct": 0, "cic_round": 0}


def cicr_lds_max_r(rnd):
    return CICR_LDS_WAVE_BYTES // (rnd * 128)


def cicr_direct_kind(R):
    return IN_CU8_CICR16 if R % 8 == 0 else IN_CU8_CICR8 if R % 4 == 0 else IN_CU8_CICR4 if R % 2 == 0 else IN_CU8_CICR2


def cicr_lds_kind(R, rnd):
    if R < 2 or R > cicr_lds_max_r(rnd):
        return -1
    return {4: IN_CU8_CICR_LDS4, 2: IN_CU8_CICR_LDS2, 1: IN_CU8_CICR_LDS1}[rnd]


def cicr_kind(R):
    if R == 10:
        return IN_CU8_CIC10
    if R == 12:
        return IN_CU8_CIC12
    if R < 3 or R > cicr_lds_max_r(1):
        return cicr_direct_kind(R)
    return IN_CU8_CICR_LDS4 if R <= cicr_lds_max_r(4) else IN_CU8_CICR_LDS2 if R <= cicr_lds_max_r(2) else IN_CU8_CICR_LDS1


def cic_in_kind(R, opts):
    if R == 8:
        return IN_CU8_CIC8
    if opts["cic_direct"]:
        return cicr_direct_kind(R)
    if opts["cic_round"]:
        k = cicr_lds_kind(R, opts["cic_round"])
        if k >= 0:
            return k
    return cicr_kind(R)


def fused_kone_kind(in_kind):
    return in_kind in (IN_CU8, IN_CU8_CIC8) or in_kind >= IN_CU8_CIC10


def f64_fused_kind(n_fft, in_kind):
    return n_fft in FUSED_N and in_kind in (IN_CU8, IN_CS32, IN_RF32, IN_CU8_CIC8, IN_CU8_CIC10, IN_CU8_CIC12)


def use_v2(n_fft, in_kind, k_avg, opts):
    if not (n_fft in (2048, 4096) and in_kind == IN_CU8):
        return False
    return opts["v2"] != 0 if opts["v2"] >= 0 else k_avg == 1


class Case(namedtuple("Case", "f64 N input cic_r K window output gain_db rows_f32 opts")):
    """One descriptor of rtlws_spectra_batch (f64=False) or rtlws_spectra_batch_f64 (f64=True); `opts` is a
    tuple of (engine option, value) pairs the case runs under."""

    def options(self):
        o = dict(DEFAULT_OPTS)
        o.update(dict(self.opts))
        return o

    def in_kind(self):
        return cic_in_kind(self.cic_r, self.options()) if self.cic_r > 1 else INPUTS[self.input]

    def label(self):
        s = "%s N=%d %s%s K=%d %s %s" % ("f64" if self.f64 else "f32", self.N, self.input,
                                         "/R%d" % self.cic_r if self.cic_r > 1 else "", self.K, self.window,
                                         self.output)
        if self.output == "payload_u8":
            s += " gain=%d" % self.gain_db
        if self.rows_f32:
            s += " rows_f32"
        if self.opts:
            s += " " + ",".join("%s=%d" % kv for kv in self.opts)
        return s


def instantiation(c):
    """(kernel name, template arguments) of the instantiation rtlws_spectra_batch[_f64] launches for case c, as the
    demangled name in the code object spells it: spectra_fused<1024, 12, true, 2, false> -> ("spectra_fused",
    (1024, 12, True, 2, False))."""
    o = c.options()
    win = c.window == "hann"
    out = OUTPUTS[c.output]
    if not c.f64:                                             # plan_f32
        if c.N not in FUSED_N:
            return ("spectra_direct", (INPUTS[c.input],))
        k = c.in_kind()
        if use_v2(c.N, k, c.K, o):
            return ("spectra_fused_v2", (c.N, win, out, c.K == 1))
        return ("spectra_fused", (c.N, k, win, out, c.K == 1 and fused_kone_kind(k)))
    k = c.in_kind()                                           # plan_f64 (16-byte aligned buffers)
    if not (f64_fused_kind(c.N, k) and o["f64_fused"]):
        return ("spectra_f64", (INPUTS[c.input],))
    rowf32 = c.rows_f32 and out != OUT_PAYLOAD                # Flag<out != OUT_PAYLOAD>
    if c.N == 1024 and k == IN_CU8 and not win and o["f64_x1024"] and (out == OUT_SUM or c.K == 1):
        waves = o["f64_x_waves"]
        if waves not in (1, 8):
            return None                                       # by batch size: a case names its waves instead
        return ("spectra_f64_1024x", (out, c.K == 1, rowf32, waves))
    return ("spectra_f64_fused", (c.N, k, win, out, c.K == 1 and fused_kone_kind(k), rowf32))


# ---- the cases --------------------------------------------------------------------------------------------------

# one R per CIC input kind (small ones, odd where the kind allows: the LDS stages' half-wavefront tail): default
# routing, then with cic_direct = 1
CIC_DEFAULT = (5, 19, 37, 8, 10, 12)                          # LDS4, LDS2, LDS1, CIC8, CIC10, CIC12
CIC_DIRECT = (3, 6, 4, 16)                                    # CICR2, CICR4, CICR8, CICR16
K_MANY = 2                                                    # K > 1: two frames per row
# payload gains: +40 dB lifts the int32-extreme cmplx_s32 rows past 255 (so every cs32 payload case takes it), -30 dB
# leaves most u8 bins below 0 dB; the GPU test asserts that both clamps occur
PAYLOAD_GAINS = (40, -30)


def _routes(f64):
    """(input, cic_r, opts) of every input stage the tables tell apart."""
    r = [("cu8", 0, ()), ("cs32", 0, ()), ("rf32", 0, ())]
    r += [("cu8", R, ()) for R in CIC_DEFAULT]
    if not f64:
        r += [("cu8", R, (("cic_direct", 1),)) for R in CIC_DIRECT]
    return r


def _candidates():
    """Descriptors in the order the cases are drawn from: defaults before options, so that a case carries an option
    only where the default routing cannot reach its instantiation."""
    for f64 in (False, True):
        for N in FUSED_N:
            for inp, R, opts in _routes(f64):
                for window in ("rect", "hann"):
                    for output in ("power_sum", "mean_db", "payload_u8"):
                        for K in (1, K_MANY):
                            flags = (False, True) if f64 and output != "payload_u8" else (False,)
                            for rows_f32 in flags:
                                variants = [opts]
                                if not f64 and inp == "cu8" and R == 0 and N != 1024:
                                    variants += [opts + (("v2", 0),), opts + (("v2", 1),)]
                                if f64 and inp == "cu8" and R == 0 and N == 1024 and window == "rect":
                                    # the 1024x kernel in both forms, and the two-transposition kernel it shadows
                                    variants += [opts + (("f64_x_waves", 1),), opts + (("f64_x_waves", 8),),
                                                 opts + (("f64_x1024", 0),)]
                                for v in variants:
                                    gain = 0
                                    if output == "payload_u8":
                                        gain = PAYLOAD_GAINS[0 if inp == "cs32" else (N // 1024 + K + R) % 2]
                                    yield Case(f64, N, inp, R, K, window, output, gain, rows_f32, v)


def _runtime_only():
    """spectra_direct<IN> and spectra_f64<IN> take window, output, K, CIC factor and rows_f32 at run time: one case
    per value, beside the one per instantiation."""
    out = []
    for f64 in (False, True):
        for inp in ("cu8", "cs32", "rf32"):
            out.append(Case(f64, 100, inp, 0, 1, "rect", "power_sum", 0, False, ()))
        for output, gain in (("mean_db", 0), ("payload_u8", 40), ("payload_u8", -30)):
            out.append(Case(f64, 100, "cu8", 0, K_MANY, "hann", output, gain, False, ()))
        out.append(Case(f64, 100, "cu8", 3, K_MANY, "rect", "power_sum", 0, False, ()))
    for output in ("power_sum", "mean_db"):
        out.append(Case(True, 100, "cs32", 0, K_MANY, "hann", output, 0, True, ()))
    # a fused size through the general f64 kernel: a CIC factor the fused kernel has no input stage for
    out.append(Case(True, 1024, "cu8", 3, K_MANY, "hann", "power_sum", 0, False, ()))
    out.append(Case(True, 2048, "cu8", 3, 1, "rect", "payload_u8", 40, False, ()))
    return out


def _build():
    cases, seen = [], set()
    for c in _candidates():
        t = instantiation(c)
        if t is not None and t not in seen:
            seen.add(t)
            cases.append(c)
    return cases + _runtime_only()


CASES = _build()

# The gfx950 kernels that are not spectrum instantiations, each with the test that launches it.
OTHER_KERNELS = {
    "cic8_kernel": "tests/test_resample_gpu.py::test_cic_large_block_sums",
    "cicr_kernel<0>": "tests/test_resample_gpu.py::test_cic_block_sums_every_shape",
    "cicr_kernel<10>": "tests/test_resample_gpu.py::test_cic_block_sums_every_shape",
    "cicr_kernel<12>": "tests/test_resample_gpu.py::test_cic_block_sums_every_shape",
    "fm_demod_kernel": "tests/test_audio_gpu.py::test_fm_demod_kernel_vs_oracle",
    "halfband_kernel": "tests/test_resample_gpu.py::test_halfband_vs_oracle",
    "clock_stamp_kernel": "tests/test_bench_gpu.py::test_clock_stamps_bracket_a_plausible_clock",
    "payload_kernel": "tests/test_kernel_matrix_gpu.py::test_payload_from_sums_kernels",
    "payload_f64_kernel": "tests/test_cbb_gpu.py::test_live_path_payload_and_cadence",
    "welch_accumulate_kernel": "tests/test_cbb_gpu.py::test_welch_mode_every_buffer_of_the_interval",
    "welch_finish_kernel": "tests/test_cbb_gpu.py::test_welch_mode_every_buffer_of_the_interval",
}


def family(c):
    """The GPU test's parameter: kernel family and N."""
    name = instantiation(c)[0]
    return "%s-%d" % (name, c.N)


FAMILIES = sorted({family(c) for c in CASES})
