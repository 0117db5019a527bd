"""The definition of include/rtlws_pfb.h restated in numpy: the branch filters in int64 (exact), the transform in
f64.  The yardstick of tests/test_pfb_cpu.py and tests/test_pfb_gpu.py."""
import numpy as np

# the shapes the GPU matrix runs: (log2 M, taps per branch)
SHAPES = ((4, 1), (4, 7), (5, 2), (5, 32), (6, 8), (7, 3), (8, 8), (9, 1), (10, 4), (10, 32))


def samples_needed(M, T, D, nframes):
    return (nframes - 1) * D + T * M if nframes > 0 else 0


def design(k, T):
    """rtlws_pfb_design's expression in f64 (before rint) -> float64 [T * M]."""
    M = 1 << k
    N = T * M
    n = np.arange(N, dtype=np.float64)
    return 32767.0 * np.sinc((n - (N - 1) / 2.0) / M) * (0.54 - 0.46 * np.cos(2.0 * np.pi * n / (N - 1)))


def twiddles(k):
    """e^(-2 pi i j / M) in f64, the quadrant points exact, rounded once to f32 -> float32 [M, 2]."""
    M = 1 << k
    j = np.arange(M)
    w = np.exp(-2j * np.pi * j / M)
    q = (4 * j) % M == 0
    w[q] = np.rint(w[q].real) + 1j * np.rint(w[q].imag)
    return np.stack([w.real, w.imag], axis=1).astype(np.float32)


def branch_sums(x, k, taps, D, nframes):
    """v_m[p] = sum_t h[p + t M] x[m D + t M + p] for complex x of any dtype -> [nframes, M]."""
    M = 1 << k
    h = np.asarray(taps).reshape(-1, M)
    T = h.shape[0]
    assert len(x) >= samples_needed(M, T, D, nframes)
    v = np.zeros((nframes, M), dtype=x.dtype)
    for m in range(nframes):
        v[m] = (h * x[m * D:m * D + T * M].reshape(T, M)).sum(axis=0)
    return v


def channelize(x, k, taps, hop=None, first_frame_index=0, nframes=None):
    """The definition on a complex f64 signal x (unquantised) -> complex128 [nframes, M], time-major."""
    M = 1 << k
    T = len(taps) // M
    D = M if hop is None else int(hop)
    assert D in (M, M // 2) and T * M == len(taps)
    if nframes is None:
        nframes = (len(x) - T * M) // D + 1 if len(x) >= T * M else 0
    v = branch_sums(np.asarray(x, dtype=np.complex128), k, np.asarray(taps, dtype=np.float64), D, nframes)
    y = np.fft.fft(v, axis=1)
    if D != M:
        g = first_frame_index + np.arange(nframes, dtype=np.int64)
        y[np.ix_(g % 2 == 1, np.arange(M) % 2 == 1)] *= -1.0
    return y


def pfb_ref(iq, k, taps, hop=None, first_frame_index=0, nframes=None):
    """iq uint8 [n, 2], taps int16 [T * M] -> complex128 [nframes, M] (time-major; channel-major is the transpose).
    The branch sums are exact integers (|v| <= T * 2^22 fits f64 exactly)."""
    iq = np.asarray(iq, dtype=np.uint8).reshape(-1, 2)
    M = 1 << k
    taps = np.asarray(taps)
    assert taps.dtype == np.int16 and 4 <= k <= 10 and taps.size % M == 0 and 1 <= taps.size // M <= 32
    T = taps.size // M
    D = M if hop is None else int(hop)
    assert D in (M, M // 2) and first_frame_index >= 0
    if nframes is None:
        nframes = (iq.shape[0] - T * M) // D + 1 if iq.shape[0] >= T * M else 0
    xi = iq.astype(np.int64) - 128
    vr = branch_sums(xi[:, 0], k, taps.astype(np.int64), D, nframes)
    vi = branch_sums(xi[:, 1], k, taps.astype(np.int64), D, nframes)
    assert max(np.abs(vr).max(initial=0), np.abs(vi).max(initial=0)) < 2 ** 31
    y = np.fft.fft(vr.astype(np.float64) + 1j * vi.astype(np.float64), axis=1)
    if D != M:
        g = first_frame_index + np.arange(nframes, dtype=np.int64)
        y[np.ix_(g % 2 == 1, np.arange(M) % 2 == 1)] *= -1.0
    return y


def bound(k):
    """Per frame: ||got - ref||_2 <= bound(k) * ||ref||_2 (Higham, Thm 24.2, with the conversion of v: DESIGN.md 4.14)."""
    return 8.0 * (k + 1) * 2.0 ** -24


def random_iq(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, 2), dtype=np.uint8)


def full_scale_iq(n, seed):
    """Every byte 0 or 255: with every tap 32767 the int32 range and |v| > 2^24."""
    return (np.random.default_rng(seed).integers(0, 2, size=(n, 2), dtype=np.uint8) * 255).astype(np.uint8)


def random_taps(k, T, seed):
    return np.random.default_rng(seed).integers(-32768, 32768, size=T << k, dtype=np.int64).astype(np.int16)


def tone_iq(n, cycles_per_sample, amplitude=100.0):
    """A u8 capture of one complex tone."""
    ph = 2.0 * np.pi * cycles_per_sample * np.arange(n, dtype=np.float64)
    z = amplitude * np.exp(1j * ph)
    return np.clip(np.rint(np.stack([z.real, z.imag], axis=1)) + 128, 0, 255).astype(np.uint8)


def leakage_db(y, c0):
    """y [nframes, M] of a tone half-way between channels c0 and c0 + 1: the largest mean power of a channel two or
    more away from both, relative to channel c0's mean power, in dB."""
    M = y.shape[1]
    pw = (np.abs(y) ** 2).mean(axis=0)
    c = np.arange(M)
    d0 = np.minimum((c - c0) % M, (c0 - c) % M)
    d1 = np.minimum((c - c0 - 1) % M, (c0 + 1 - c) % M)
    far = (d0 >= 2) & (d1 >= 2)
    return 10.0 * np.log10(pw[far].max() / pw[c0])


def selectivity_case():
    """M = 64, T = 8, hop M: a u8 tone of amplitude 100 half-way between channels c0 and c0 + 1 ->
    (k, T, c0, iq, taps of 32767 on the first M only: the block sum as a prototype)."""
    k, T, c0 = 6, 8, 5
    M = 1 << k
    iq = tone_iq(samples_needed(M, T, M, 64), (c0 + 0.5) / M, 100.0)
    boxcar = np.zeros(T * M, np.int16)
    boxcar[:M] = 32767
    return k, T, c0, iq, boxcar
