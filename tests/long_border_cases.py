"""The cases of tests/test_long_gpu.py's border tests as data (include/rtlws_long.h, rtl-ws_amd/csrc/spectrum_long.hip;
DESIGN.md 4.9), in the style of anylen_border_cases.py: the sizes m = log2 n_fft per test, the (m, frames) and kind
lists, the group plan of rtlws_long_open restated, the row layout in any precision and the stable accuracy metric.
tests/test_long_borders_cpu.py holds the tables to their conditions.  No GPU is used here.

Every (pass A length, pass B length) = (2^ceil(m/2), 2^floor(m/2)) occurs at exactly one m = 14 .. 20.  A workgroup of
pass A holds T = 8192 / N1 columns, one of pass B 8192 / N2; pass A's grid is frames * N / 8192 workgroups and goes
through xcd_chunked: the identity unless the grid is a multiple of 8."""
import numpy as np

import long_kernels as lk

TILE_POINTS = 8192
INPUTS = ("cu8", "cs32", "rf32")
ROWS = ("f64", "f32", "u8")
SAMPLE_BYTES = {"cu8": 2, "cs32": 8, "rf32": 4}
ROW_BYTES = {"f64": 8, "f32": 4, "u8": 1}
ROW_DTYPE = {"f64": np.float64, "f32": np.float32, "u8": np.uint8}
WORKSPACE_CAP = 1 << 30                      # RTLWS_LONG_WORKSPACE_CAP


def n1(m):
    return 1 << lk.log2_n1(m)


def n2(m):
    return 1 << lk.log2_n2(m)


def pass_a_columns(m):
    return TILE_POINTS // n1(m)


def pass_b_columns(m):
    return TILE_POINTS // n2(m)


def pass_a_grid(m, frames):
    return frames << (m - 13)


def grid_is_permuted(m, frames):
    """xcd_chunked is a permutation across the eight chunks, not the identity"""
    return pass_a_grid(m, frames) % 8 == 0


# ---- which m each test runs ------------------------------------------------------------------------------------------
ACCURACY_M = tuple(lk.SIZES)                 # a: every (N1, N2) pair
PASS_A_FIRST_M = (14, 15, 17, 19)            # the first m that reaches each N1 = 128 .. 1024
PASS_B_FIRST_M = (14, 16, 18, 20)            # the first m that reaches each N2 = 128 .. 1024
STORES_M = PASS_B_FIRST_M                    # b: store_value is pass B's
K_SUMS_M = PASS_B_FIRST_M                    # c: so are the sums
SCALING_M = (14, 15, 17, 19, 20)             # d: every pass A length, and the one m with N2 = 1024
EXTREMES_M = (14, 19)                        # e: T = 64 and T = 8 columns in pass A, where the samples are converted
OWN_ROW_M = (14, 16)                         # f: three frames, an identity and a permuted pass A grid (6 and 24)
STORES_GAIN = dict(zip(STORES_M, (9, -25, 100, 0)))
SATURATION_M, SATURATION_GAIN = 14, 40       # b, once: a cmplx_s32 tone whose bytes reach 255

# g: (m, frames): pass A grids 6, 10 (identity, grid % 8 = 6 and 2), 16 and 256 (permuted)
PLACE_CASES = ((14, 3), (14, 5), (15, 4), (20, 2))

# h: one size, every sample size against two row sizes and back
GROUP_M, GROUP_K, GROUP_FRAMES = 14, 2, 10
GROUP_KINDS = (("cu8", "f64"), ("cs32", "f32"), ("rf32", "u8"), ("cs32", "u8"), ("rf32", "f64"), ("cu8", "f32"))
GROUP_MAX_FRAMES = (10, 4, 3, 1)             # one group; 4, 4, 2; 3 rounded up to a whole row: 4, 4, 2; five groups of one row
GROUP_GAIN = 9

# i: (m, input, rows)
OUTSIDE_CASES = ((14, "cs32", "f32"), (15, "rf32", "u8"), (19, "cu8", "f64"), (20, "cs32", "u8"), (20, "cu8", "f32"))
OUTSIDE_FRAMES, OUTSIDE_GUARD, OUTSIDE_SKEW = 3, 1024, 8      # the frames begin GUARD + SKEW bytes into the buffer
OUTSIDE_GAIN = 9


def tables():
    """The tables tests/test_long_borders_cpu.py holds to their conditions, as one dict of lists."""
    return dict(accuracy=list(ACCURACY_M), stores=list(STORES_M), k_sums=list(K_SUMS_M), scaling=list(SCALING_M),
                extremes=list(EXTREMES_M), own_row=list(OWN_ROW_M), place=list(PLACE_CASES), group_kinds=list(GROUP_KINDS),
                group_max_frames=list(GROUP_MAX_FRAMES), outside=list(OUTSIDE_CASES))


# ---- rtlws_long_open's group rule ------------------------------------------------------------------------------------

def frames_in_flight(N, K, max_frames, cap=WORKSPACE_CAP):
    """max_frames rounded up to whole rows, at most the rows whose frames fit the cap, at least one row"""
    cap_rows = max(cap // (16 * N) // K, 1)
    rows = 1 if max_frames < 1 else (max_frames + K - 1) // K
    return min(rows, cap_rows) * K


def group_plan(nframes, N, K, max_frames, cap=WORKSPACE_CAP):
    """frames per group of rtlws_long_run, in launch order"""
    assert nframes % K == 0
    g = frames_in_flight(N, K, max_frames, cap)
    return [min(g, nframes - done) for done in range(0, nframes, g)]


# ---- frames, rows and the metric -------------------------------------------------------------------------------------

def convert(frames, input, dtype=np.complex128):
    """[F, N(, 2)] samples -> [F, N] complex, as src/spectrum.c:54-58,72-76,90-94 converts them (every step exact)"""
    a = np.asarray(frames)
    real = np.empty(0, dtype).real.dtype
    if input == "cu8":
        return ((a[..., 0].astype(real) - 128) / 128 + 1j * ((a[..., 1].astype(real) - 128) / 128)).astype(dtype)
    if input == "cs32":
        return (a[..., 0].astype(real) / 128 + 1j * (a[..., 1].astype(real) / 128)).astype(dtype)
    return a.astype(real).astype(dtype)


def rows_from_powers(P, K):
    """P: [F, N] |X[k]|^2 per frame, any float type -> [F / K, N] rows in that type: slot i shows bin (i + N/2) mod N
    summed over the row's K frames in frame order from zero; slot N/2 holds sum_k (K - k) P_k[N - 1] instead of bin 0
    (src/spectrum.c:25-33 in closed form, as long_pass_b carries it)."""
    F, N = P.shape
    assert F % K == 0
    P = P.reshape(F // K, K, N)
    rows = np.zeros((F // K, N), dtype=P.dtype)
    dc = np.zeros(F // K, dtype=P.dtype)
    for k in range(K):
        rows += np.roll(P[:, k], -(N // 2), axis=1)
        dc += P.dtype.type(K - k) * P[:, k, N - 1]
    rows[:, N // 2] = dc
    return rows


def truth_rows(frames, input, K=1):
    """The rows in long double: numpy's FFT of the converted frames in np.clongdouble (64-bit mantissa asserted by
    the callers), |X|^2, laid out as rows."""
    x = convert(frames, input, np.clongdouble)
    x = x.reshape(-1, x.shape[-1])
    X = np.fft.fft(x, axis=1)
    assert X.dtype == np.clongdouble, "np.fft.fft fell back to double"
    return rows_from_powers(X.real * X.real + X.imag * X.imag, K)


def four_step_rows(frames, input, K=1):
    """The rows of test_long_cpu.four_step, the kernels' algorithm in numpy f64 with the two-table twiddle"""
    from test_long_cpu import four_step
    x = convert(frames, input)
    X = np.stack([four_step(f) for f in x.reshape(-1, x.shape[-1])])
    return rows_from_powers(X.real ** 2 + X.imag ** 2, K)


def e_metric(row, truth):
    """e(row) = rms(row - truth) / mean(truth), in long double: the whole row's error against the whole row's level,
    where the per-bin metric of helpers.rel_err is set by the row's few weakest bins"""
    d = np.asarray(row).astype(np.longdouble).ravel() - np.asarray(truth, dtype=np.longdouble).ravel()
    return float(np.sqrt(np.mean(d * d)) / np.mean(np.asarray(truth, dtype=np.longdouble)))


def accuracy_frames(m):
    """input -> the one frame of test_accuracy_against_long_double[m]"""
    from rtlws import synth
    N = 1 << m
    rng = np.random.default_rng(600 + m)
    return {"cu8": synth.uniform_iq(1, N, seed=60 + m),
            "cs32": rng.integers(-(1 << 20), (1 << 20) + 1, size=(1, N, 2), dtype=np.int32),
            "rf32": rng.standard_normal((1, N)).astype(np.float32)}


def coverage_text():
    """For the documents: per m the lengths, the columns per workgroup and the tests that run it."""
    lines = []
    for m in lk.SIZES:
        t = [name for name, ms in (("a", ACCURACY_M), ("b", STORES_M), ("c", K_SUMS_M), ("d", SCALING_M), ("e", EXTREMES_M),
                                   ("f", OWN_ROW_M), ("g", [c[0] for c in PLACE_CASES]), ("h", [GROUP_M]),
                                   ("i", [c[0] for c in OUTSIDE_CASES])) if m in ms]
        lines.append("  m = %d: N1 = %d (T = %d), N2 = %d (T = %d): %s" % (m, n1(m), pass_a_columns(m), n2(m), pass_b_columns(m),
                                                                         " ".join(t)))
    return "\n".join(lines)
