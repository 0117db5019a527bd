"""The definition of include/rtlws_period.h restated in numpy: the yardstick of tests/test_period_gpu.py.
Stage 1 (the power spectrum) in f64, to be met within bound(log2n); stages 2 - 4 (whitening, harmonic sums, peaks) as
np.float32 arithmetic in the header's order, to be met bit for bit.  tests/test_period_cpu.py holds this file's own
properties."""
import math

import numpy as np

MIN_LOG2N, MAX_LOG2N, MAX_LEVELS, MIN_NORM, MIN_SEG, MAX_TRIALS = 10, 15, 5, 16, 64, 65536
U = 2.0 ** -24                                   # the unit roundoff of f32


def power(x, log2n):
    """P[k], k < M, of one series (float32 [nsamp], nsamp <= N) in f64: the mean removed, zeros behind, the N-point DFT
    squared; the Nyquist bin dropped"""
    n = 1 << log2n
    x = np.asarray(x, np.float32).astype(np.float64)
    assert x.ndim == 1 and 1 <= x.size <= n
    y = np.zeros(n)
    y[:x.size] = x - x.mean()
    return (np.abs(np.fft.rfft(y)) ** 2)[:n // 2]


def nyquist_power(x, log2n):
    """the bin that power() drops (bound()'s premise is about it)"""
    n = 1 << log2n
    x = np.asarray(x, np.float32).astype(np.float64)
    y = np.zeros(n)
    y[:x.size] = x - x.mean()
    return float(np.abs(np.fft.rfft(y)[n // 2]) ** 2)


def bound(log2n):
    """c(log2n): per trial sum_k |P^[k] - P[k]| <= c sum_k P[k], derived, for series whose Nyquist bin
    holds no more power than the M bins kept and whose mean is at most 2^8 of their standard deviation.

    The packed series z has |Z|^2 = M |y|^2 = sum_{k<M} P + (P[M] - P[0]) / 2 <= 1.5 sum P under the first premise.
      input   y = fl(x - mu^): u relative to |y| itself; mu^ - mu <= nsamp 2^-53 mean|x| (f64 sums), at most u |y|_rms
              under the second premise (2^15 2^-53 2^8 (1 + 2^-8) < 2^-29): b_in = 2 u
      FFT     Higham, Accuracy and Stability, Thm 24.2 over t = log2 M radix-2 stages (the radix-16 passes are four of
              them each, with fewer roundings): b_fft = t eta / (1 - t eta), eta = mu + gamma_4 (sqrt 2 + mu), mu = u the
              error of a once-rounded twiddle
      untangling  X[k] = E - i W O, E, O = (Z[k] +- conj Z[M-k]) / 2: one rounding each (u), the product W O with the
              once-rounded W (mu + sqrt 2 gamma_3), the last addition (u): |dX[k]| <= b_u (|E| + |O|), b_u = 3 u + mu +
              sqrt 2 gamma_3, and sum_k (|E| + |O|)^2 <= 2 |Z|^2; the map itself takes |dZ| to at most sqrt 2 |dZ|
      so |dX| <= sqrt 2 (b_z + b_u (1 + b_z)) |Z| <= beta sqrt(sum P), beta = sqrt 3 (b_z + b_u (1 + b_z)),
      b_z = b_in + b_fft (1 + b_in); squaring: | |X^|^2 - |X|^2 | summed is at most (2 beta + beta^2) sum P, and the
      square's own three roundings add gamma_3 (1 + beta)^2."""
    t = log2n - 1
    mu = U
    gamma = lambda n: n * U / (1.0 - n * U)
    eta = mu + gamma(4) * (math.sqrt(2.0) + mu)
    b_fft = t * eta / (1.0 - t * eta)
    b_in = 2.0 * U
    b_z = b_in + b_fft * (1.0 + b_in)
    b_u = 3.0 * U + mu + math.sqrt(2.0) * gamma(3)
    beta = math.sqrt(3.0) * (b_z + b_u * (1.0 + b_z))
    return 2.0 * beta + beta * beta + gamma(3) * (1.0 + beta) ** 2


def path_bound(b_fft):
    """b1 of bound_bin from the transform's per-term error b_fft: |X^[k] - X[k]| <= b1 ||y||_1"""
    gamma3 = 3.0 * U / (1.0 - 3.0 * U)
    b_u = 3.0 * U + U + math.sqrt(2.0) * gamma3
    b_path = math.sqrt(2.0) * b_fft + 2.0 * b_u * (1.0 + b_fft)
    b_y = U + 2.0 ** -52                         # y = fl32(fl64(x - mu^)): relative to y itself
    return b_y + b_path * (1.0 + b_y)


def bound_bin(log2n):
    """b1(log2n): for EVERY bin k < M, with no premise on the series,
        | |X^[k]| - |X[k]| |  <=  A + gamma_3 (|X[k]| + A) + 2^-62,    A = b1 ||y||_1 + (1 + b1) mean_term(x),
    |X^[k]| = sqrt(P^[k]), derived per term of X[k] = sum_n y[n] w^(n k) from bound()'s constants:
      input   y^[n] = (y[n] + mu - mu^)(1 + d), |d| <= b_y = u + 2^-52; the mean's error is mean_term's, no premise
      FFT     every path from a point to a bin passes t = log2 M radix-2 stages' worth of roundings and once-rounded
              roots, (1 + eta) each: (1 + theta), |theta| <= b_fft = t eta / (1 - t eta), so |dZ[k]| <= b_fft ||z||_1
              and ||z||_1 <= ||y||_1.  The radix-16 passes spend 13.9 u of their 4 eta = 26.6 u, with the register
              butterflies' roots made as cos (1 + i tan) from two rounded literals (error 2 u, not u) counted
      untangling  X[k] = Z[k] (1 - i W) / 2 + conj Z[M - k] (1 + i W) / 2, |1 - i W| / 2 + |1 + i W| / 2 <= sqrt 2: the map
              takes the two |dZ| to sqrt 2 b_fft ||y||_1; its own roundings b_u (|E| + |O|) <= 2 b_u (1 + b_fft) ||y||_1
      so b_path = sqrt 2 b_fft + 2 b_u (1 + b_fft), b1 = b_y + b_path (1 + b_y)
      the square's three roundings: sqrt(P^) within gamma_3 of |X^|; 2^-62 is the square root of f32's underflow."""
    t = log2n - 1
    eta = U + 4.0 * U / (1.0 - 4.0 * U) * (math.sqrt(2.0) + U)
    return path_bound(t * eta / (1.0 - t * eta))


def mean_term(x):
    """sum_n |mu^ - mu| over the series: the f64 sum of nsamp samples in any order, one division: at most
    gamma64_(nsamp + 1) sum |x| (what bound() takes as a premise, computed from x)"""
    x = np.asarray(x, np.float32).astype(np.float64)
    g = (x.size + 1) * 2.0 ** -53
    return g / (1.0 - g) * float(np.abs(x).sum())


def bin_allowance(x, ref_power, b1):
    """the right side of bound_bin for one series x (float32 [nsamp]) and its f64 spectrum -> float64 [M]"""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    a = b1 * float(np.abs(x64 - x64.mean()).sum()) + (1.0 + b1) * mean_term(x)
    gamma3 = 3.0 * U / (1.0 - 3.0 * U)
    return a + gamma3 * (np.sqrt(ref_power) + a) + 2.0 ** -62


def bin_share(power_row, x, ref_power, b1):
    """(the worst | |X^| - |X| | over the bins as a share of bin_allowance, its bin)"""
    err = np.abs(np.sqrt(np.asarray(power_row, np.float64)) - np.sqrt(ref_power))
    allow = bin_allowance(x, ref_power, b1)
    share = err / allow                                          # the allowance is at least 2^-62
    share = np.where(np.isnan(share), np.inf, share)             # a NaN in the row is never within
    k = int(share.argmax())
    return float(share[k]), k


def tree_sums(p, norm, pairs_first=True):
    """the block sums of float32 [.., M], flat over the leading axes: the balanced halving tree, adjacent pairs first (pairs_first False: the other
    balanced tree, halves first -- test_period_cpu's check that the order is not idle)"""
    s = np.asarray(p, np.float32).reshape(-1, norm)
    while s.shape[1] > 1:
        h = s.shape[1] // 2
        s = s[:, 0::2] + s[:, 1::2] if pairs_first else s[:, :h] + s[:, h:]
    return s[:, 0]


def whiten(p, norm, pairs_first=True):
    """W = fl(P / fl(sum_b 2^-log2 norm)) of float32 [.., M]; 0 / 0 is NaN"""
    p = np.ascontiguousarray(p, np.float32)
    assert p.shape[-1] % norm == 0 and norm & (norm - 1) == 0
    with np.errstate(all="ignore"):
        mean = tree_sums(p, norm, pairs_first) * np.float32(1.0 / norm)
        w = p / np.repeat(mean, norm).reshape(p.shape)
    assert w.dtype == np.float32
    return w


def sums(w, levels, descending=False):
    """S float32 [.., levels, M] of W [.., M]: acc = W[k]; level l adds W[(k h + 2^(l-1)) >> l] for odd h ascending (descending True:
    the reversed order, for test_period_cpu)"""
    w = np.asarray(w, np.float32)
    k = np.arange(w.shape[-1], dtype=np.int64)
    acc = w.copy()
    out = [acc.copy()]
    with np.errstate(all="ignore"):
        for l in range(1, levels):
            hs = range(1, 1 << l, 2)
            for h in (reversed(hs) if descending else hs):
                acc = acc + w[..., (k * h + (1 << (l - 1))) >> l]
            out.append(acc.copy())
    s = np.stack(out, axis=-2)
    assert s.dtype == np.float32
    return s


def peaks(s, seg, klo):
    """(best float32 [.., nseg], at int32 [.., nseg]) of S [.., M]: over the k of a segment that are >= klo the strict
    maximum, ties to the smaller k, a NaN never taken; (-Inf, -1) where nothing is taken"""
    s = np.asarray(s, np.float32)
    nseg = s.shape[-1] // seg
    v = np.where(np.isnan(s), -np.inf, s).astype(np.float32)
    v[..., :klo] = -np.inf
    v = v.reshape(s.shape[:-1] + (nseg, seg))
    where = v.argmax(axis=-1)                                    # the first of equal maxima
    best = np.take_along_axis(v, where[..., None], axis=-1)[..., 0]
    at = (where + seg * np.arange(nseg)).astype(np.int32)
    at[np.isneginf(best)] = -1
    return best.astype(np.float32), at


def period_ref(power_rows, levels, norm, seg, klo):
    """stages 2 - 4 over float32 [ntrials, M]: (white [ntrials, M], best [ntrials, levels, nseg], at)"""
    white = whiten(power_rows, norm)
    best, at = peaks(sums(white, levels), seg, klo)
    return white, best, at


def samples(log2n, level, k):
    return float(1 << (log2n + level)) / float(k)


def lnq(s, h):
    """ln(e^-S sum_{j<H} S^j / j!) through its largest term; 0 for S <= 0, NaN for H outside 1 .. 16 or S not finite"""
    if not (1 <= h <= 16) or not math.isfinite(s):
        return float("nan")
    if s <= 0.0:
        return 0.0
    terms = [j * math.log(s) - math.lgamma(j + 1.0) for j in range(h)]
    top = max(terms)
    return min(-s + top + math.log(sum(math.exp(t - top) for t in terms)), 0.0)


def geometry(log2n, seg, ntrials):
    m = 1 << (log2n - 1)
    return ntrials, max(64, m // 16), 8 * (m + m // 16), m // seg


def signed_exponent_series(ntrials, nsamp, log2n, seed):
    """series whose spectra have exponents spread over 2^-6 .. 2^6: noise plus tones of amplitudes 2^e"""
    rng = np.random.default_rng(seed)
    n = np.arange(nsamp)
    x = rng.standard_normal((ntrials, nsamp)) * 0.05
    for t in range(ntrials):
        for _ in range(24):
            k = rng.integers(1, 1 << (log2n - 1))
            x[t] += np.exp2(rng.integers(-6, 7) / 2.0) * np.cos(2.0 * np.pi * k * n / (1 << log2n) + rng.uniform(0, 6.28))
    return (x + 3.0).astype(np.float32)
