"""Reference rows for include/rtlws_anylen.h at frame lengths where the oracle's direct long-double DFT is too slow
(O(N^2) cosl/sinl: minutes at 10^5 points): the reference's row semantics (src/spectrum.c:25-33, 47-99) restated
over np.fft.fft, and the library's algorithm (Bluestein, spectrum_anylen.hip) restated in numpy.
tests/test_anylen_cpu.py pins both to the oracle at small lengths."""
import numpy as np


def convert(frames, input="cu8"):
    """[F, N(, 2)] samples -> [F, N] complex128, as src/spectrum.c:54-58,72-76,90-94 converts them."""
    a = np.asarray(frames)
    if input == "cu8":
        return (a[..., 0].astype(np.float64) - 128) / 128 + 1j * ((a[..., 1].astype(np.float64) - 128) / 128)
    if input == "cs32":
        return a[..., 0].astype(np.float64) / 128 + 1j * (a[..., 1].astype(np.float64) / 128)
    return a.astype(np.float64) + 0j


def rows_from_powers(P, K):
    """P: [F, N] |X[k]|^2 per frame -> [F / K, N] rows: slot i shows bin (N//2 + i) % N summed over the row's K
    frames; the slot that would show bin 0, i0 = N - N//2, holds sum_k (K - k) P_k[N - 1] instead (the running-sum
    rule in closed form, rows starting from a zeroed buffer)."""
    F, N = P.shape
    assert F % K == 0
    h = N // 2
    P = P.reshape(F // K, K, N)
    rows = np.zeros((F // K, N))
    for k in range(K):                                   # the frames in order, like K spectrum_add_* calls
        rows += np.roll(P[:, k], -h, axis=1)
    rows[:, N - h] = sum((K - k) * P[:, k, N - 1] for k in range(K))
    return rows


def rows(frames, N, K=1, input="cu8"):
    """Rows of rtlws_spectra_batch_f64's semantics for any N, from np.fft.fft."""
    x = convert(frames, input).reshape(-1, N)
    X = np.fft.fft(x, axis=1)
    return rows_from_powers(X.real ** 2 + X.imag ** 2, K)


# ---- the library's algorithm -------------------------------------------------------------------------------------

def conv_log2(N):
    m = 14
    while (1 << m) < 2 * N - 1:
        m += 1
    return m


def chirp(N):
    """w[n] = exp(-i pi n^2 / N) from the exact integer q = n^2 mod 2N, the angle in long double, rounded once."""
    n = np.arange(N, dtype=np.uint64)
    q = (n * n) % np.uint64(2 * N)                       # n^2 < 2^38
    a = -np.longdouble("3.141592653589793238462643383279502884") * q.astype(np.longdouble) / np.longdouble(N)
    return np.cos(a).astype(np.float64) + 1j * np.sin(a).astype(np.float64)


def bluestein_powers(x, M=None):
    """x: [F, N] complex -> [F, N] |X[k]|^2 as spectrum_anylen.hip computes them: a = x w zero-padded to M,
    b = conj(w[|n|]) wrapped around M, Bhat = FFT(b) / M, the inverse as the forward transform of the conjugate,
    the final chirp dropped (|w[k]| = 1), elements j >= N discarded."""
    F, N = x.shape
    M = M or (1 << conv_log2(N))
    assert M >= 2 * N - 1
    w = chirp(N)
    b = np.zeros(M, dtype=np.complex128)
    b[:N] = np.conj(w)
    b[M - N + 1:] = np.conj(w[1:][::-1])                 # b[M - n] = conj(w[n]), n = 1 .. N-1
    bhat = np.fft.fft(b) / M
    a = np.zeros((F, M), dtype=np.complex128)
    a[:, :N] = x * w
    z = np.fft.fft(a, axis=1) * bhat
    c = np.fft.fft(np.conj(z), axis=1)[:, :N]            # conj(a (*) b)
    return c.real ** 2 + c.imag ** 2


def bluestein_rows(frames, N, K=1, input="cu8"):
    return rows_from_powers(bluestein_powers(convert(frames, input).reshape(-1, N)), K)
