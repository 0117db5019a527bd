"""include/rtlws_cdd.h restated in numpy: the overlap-save definition in f64, the power rows in f32 as the header orders
them, the chirp and the overlap in extended and double precision, and the two derived error bounds."""
import math

import numpy as np

U = 2.0 ** -24
DISPERSION = 4.148808e3 * 1e6          # microseconds MHz^2 per pc cm^-3: rtlws_dedisp_delays' constant
MIN_LOG2_NFFT, MAX_LOG2_NFFT, MAX_NCHAN, MAX_NSEG = 9, 14, 1024, 1 << 20


def samples_needed(n, lead, trail, nseg):
    return (nseg - 1) * (n - lead - trail) + n if nseg else 0


def cdd(x, tables, lead, trail, nseg):
    """y_c[s hop + j] = (1 / N) sum_k H_c[k] X_s[k] e^(+2 pi i (j + lead) k / N), X_s the transform of points
    s hop .. s hop + N - 1: x complex [nchan, >= samples_needed], tables complex [nchan, N] -> complex128 [nchan, nseg hop]"""
    x, h = np.asarray(x, np.complex128), np.asarray(tables, np.complex128)
    nchan, n = h.shape
    hop = n - lead - trail
    y = np.zeros((nchan, nseg * hop), np.complex128)
    for s in range(nseg):
        seg = np.fft.ifft(np.fft.fft(x[:, s * hop:s * hop + n], axis=1) * h, axis=1)
        y[:, s * hop:(s + 1) * hop] = seg[:, lead:lead + hop]
    return y


def power_rows(volts, ksum):
    """The header's power rows over given voltages, in f32 operation by operation: p = fl(fl(re re) + fl(im im)), one
    accumulator from +0 over ksum samples in ascending order.  volts complex64 [nchan, n] -> float32 [nchan, n / ksum]"""
    v = np.ascontiguousarray(volts, dtype=np.complex64)
    re, im = v.real.astype(np.float32), v.imag.astype(np.float32)
    p = re * re + im * im                                          # three float32 operations, each rounded once
    assert p.dtype == np.float32 and p.shape[1] % ksum == 0
    acc = np.zeros((p.shape[0], p.shape[1] // ksum), np.float32)
    for q in range(ksum):
        acc = acc + p[:, q::ksum]
    return acc


def gamma(n):
    return n * U / (1.0 - n * U)


def b_fft(log2n):
    """Higham, Accuracy and Stability, Thm 24.2 with DESIGN.md 4.22's eta: t radix-2 stages' worth of roundings and
    once-rounded roots.  forward and inverse (its conjugate transpose: the same butterflies and roots) both spend t"""
    eta = U + gamma(4) * (math.sqrt(2.0) + U)
    return log2n * eta / (1.0 - log2n * eta)


def bound(log2n):
    """B1 = B2 = (1 + b)^2 (1 + sqrt 2 gamma_3) - 1, the f32 table taken as exact.
    Per sample, no premise: every path from point m through bin k to sample n carries forward's (1 + theta), the
      product's (1 + delta), |delta| <= sqrt 2 gamma_3, and the inverse's (1 + theta'), |theta|, |theta'| <= b, so
      |y^[n] - y[n]| <= B1 (1 / N) sum_k |H[k]| ||x_s||_1 + underflow.
    Per segment, normwise: ||X^ - X|| <= b ||X||; Z^ = H X^ (1 + delta) is within max|H| ((1 + b)(1 + sqrt 2 gamma_3) - 1)
      ||X|| of Z; the inverse adds b ||A^H Z^|| = b sqrt N ||Z^||; with ||X|| = sqrt N ||x_s|| and the exact 1 / N,
      ||y^_s - y_s||_2 <= B2 max|H| ||x_s||_2 + sqrt N underflow, over all N points and so over the hop kept."""
    b = b_fft(log2n)
    return (1.0 + b) ** 2 * (1.0 + math.sqrt(2.0) * gamma(3)) - 1.0


def underflow(tables):
    """What gradual underflow adds to a sample, stated as DESIGN.md 4.22a states its own: an operation whose result is
    below 2^-126 errs by up to 2^-150 absolutely; fewer than 16 t of them lie on the way to a sample, each reaching it
    with weight at most max(1, |H|) / N times the N terms it enters; the last scaling adds one more: under
    2^-140 (1 + max|H|) for t <= 14.  float64 [nchan]"""
    return 2.0 ** -140 * (1.0 + np.abs(np.asarray(tables, np.complex128)).max(axis=1))


def _segments(x, n, hop, nseg):
    x = np.asarray(x, np.complex128)
    return np.stack([x[:, s * hop:s * hop + n] for s in range(nseg)], axis=1)          # [nchan, nseg, N]


def sample_allowance(x, tables, lead, trail, nseg):
    """the right side of the per-sample bound, one value per (channel, segment): float64 [nchan, nseg]"""
    h = np.abs(np.asarray(tables, np.complex128))
    n = h.shape[1]
    segs = _segments(x, n, n - lead - trail, nseg)
    return bound(n.bit_length() - 1) * h.mean(axis=1)[:, None] * np.abs(segs).sum(axis=2) + underflow(tables)[:, None]


def segment_allowance(x, tables, lead, trail, nseg):
    """the right side of the normwise bound: float64 [nchan, nseg]"""
    h = np.abs(np.asarray(tables, np.complex128))
    n = h.shape[1]
    segs = _segments(x, n, n - lead - trail, nseg)
    return bound(n.bit_length() - 1) * h.max(axis=1)[:, None] * np.sqrt((np.abs(segs) ** 2).sum(axis=2)) + math.sqrt(n) * underflow(tables)[:, None]


def shares(got, x, tables, lead, trail, nseg):
    """(the worst |y^ - y| as a share of sample_allowance, the worst ||y^_s - y_s||_2 as a share of segment_allowance)
    of voltages got complex [nchan, nseg hop] against the f64 definition; a NaN is never within"""
    n = np.asarray(tables).shape[1]
    hop = n - lead - trail
    err = np.abs(np.asarray(got, np.complex128) - cdd(x, tables, lead, trail, nseg)).reshape(-1, nseg, hop)
    err = np.where(np.isnan(err), np.inf, err)
    per_sample = err.max(axis=2) / sample_allowance(x, tables, lead, trail, nseg)
    per_segment = np.sqrt((err ** 2).sum(axis=2)) / segment_allowance(x, tables, lead, trail, nseg)
    return float(per_sample.max()), float(per_segment.max())


def power_allowance(x, tables, lead, trail, nseg, ksum):
    """the per-row allowance of the power rows, by squaring the per-sample bound e: | |y^|^2 - |y|^2 | <= 2 |y| e + e^2;
    p's three roundings are gamma_3 of (|y| + e)^2, the ksum additions gamma_ksum of their sum, and a square below 2^-126
    loses up to 2^-150.  -> (the f64 power rows, their allowance), float64 [nchan, nseg hop / ksum] each"""
    y = np.abs(cdd(x, tables, lead, trail, nseg))
    hop = y.shape[1] // nseg if nseg else 1
    e = np.repeat(sample_allowance(x, tables, lead, trail, nseg), hop, axis=1)
    upper = ((y + e) ** 2).reshape(y.shape[0], -1, ksum).sum(axis=2)
    first = (2.0 * y * e + e * e).reshape(y.shape[0], -1, ksum).sum(axis=2)
    allowance = first + (gamma(3) + gamma(ksum) * (1.0 + gamma(3))) * upper + ksum * 2.0 ** -148
    return (y * y).reshape(y.shape[0], -1, ksum).sum(axis=2), allowance


def chirp(log2_nfft, f_centre_mhz, rate_mhz, dm):
    """rtlws_cdd_chirp's table in numpy.longdouble, not rounded to f32: complex longdouble parts (re, im) [N] each"""
    ld = np.longdouble
    n = 1 << log2_nfft
    k = np.arange(n)
    f = np.where(k < n // 2, k, k - n).astype(ld) * ld(rate_mhz) / ld(n)
    f0 = ld(f_centre_mhz)
    phi = ld(DISPERSION) * ld(dm) * f * f / (f0 * f0 * (f0 + f))
    phi = phi - np.rint(phi)
    two_pi = 2 * np.arctan2(ld(0), ld(-1))
    return np.cos(two_pi * phi), -np.sin(two_pi * phi)


def delay_samples(f_centre_mhz, rate_mhz, dm, f):
    """tau(f) of rtlws_cdd_overlap in Python doubles"""
    f0, w = float(f_centre_mhz), abs(float(rate_mhz))
    return DISPERSION * dm * (1.0 / ((f0 + f) * (f0 + f)) - 1.0 / (f0 * f0)) * w


def overlap(f_centre_mhz, rate_mhz, dm):
    """(lead, trail) of rtlws_cdd_overlap"""
    half = abs(float(rate_mhz)) / 2
    return math.ceil(-delay_samples(f_centre_mhz, rate_mhz, dm, half)), math.ceil(delay_samples(f_centre_mhz, rate_mhz, dm, -half))


def why_not(log2_nfft, lead, trail, nchan, ksum):
    """the library's rule text for a plan's shape, or None when it is served"""
    if not MIN_LOG2_NFFT <= log2_nfft <= MAX_LOG2_NFFT:
        return "log2_nfft must be 9 .. 14"
    if lead < 0 or trail < 0:
        return "lead and trail must be >= 0"
    hop = (1 << log2_nfft) - lead - trail
    if hop < 1:
        return "hop = N - lead - trail must be >= 1"
    if not 1 <= nchan <= MAX_NCHAN:
        return "nchan must be 1 .. 1024"
    if not 0 <= ksum <= hop:
        return "ksum must be 0 .. hop"
    if ksum and hop % ksum:
        return "ksum must divide hop"
    return None
