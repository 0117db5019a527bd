"""Stage 1 of include/rtlws_periodlong.h restated in numpy, and what a plan launches: the yardstick of
tests/test_periodlong_gpu.py beside tests/period_ref.py, whose whiten, sums and peaks serve every frame length as they
are.  The power spectrum in f64, to be met within bound(log2n)."""
import math

import numpy as np

import period_ref

MIN_LOG2N, MAX_LOG2N, MAX_LEVELS, MIN_NORM, MAX_NORM, MIN_SEG, MAX_SEG, MAX_TRIALS = 16, 22, 5, 16, 16384, 64, 16384, 65536
STAGES = 6                                       # mean, columns, rows, untangling, whitening, peaks
WORKSPACE_CAP = 1 << 30
U = 2.0 ** -24                                   # the unit roundoff of f32
MEAN_LIMIT = 2.0 ** 6                            # bound()'s second premise: |mean| <= 2^6 standard deviations


def _frame(x, log2n):
    n = 1 << log2n
    x = np.asarray(x, np.float32).astype(np.float64)
    assert x.ndim == 1 and 1 <= x.size <= n
    y = np.zeros(n)
    y[:x.size] = x - x.mean()
    return np.fft.rfft(y)


def power(x, log2n):
    """P[k], k < M, of one series (float32 [nsamp], nsamp <= N) in f64: the mean removed, zeros behind, the N-point DFT
    squared; the Nyquist bin dropped"""
    return (np.abs(_frame(x, log2n)) ** 2)[:1 << (log2n - 1)]


def nyquist_power(x, log2n):
    """the bin that power() drops (bound()'s first premise is about it)"""
    return float(np.abs(_frame(x, log2n)[1 << (log2n - 1)]) ** 2)


def premises(x, log2n):
    """(the Nyquist bin holds no more power than the M bins kept, |mean| <= MEAN_LIMIT standard deviations) of one series"""
    return power_and_premises(x, log2n)[1:]


def power_and_premises(x, log2n):
    """(power(x), the two premises of bound()) from one transform"""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    p = np.abs(_frame(x, log2n)) ** 2
    m = 1 << (log2n - 1)
    return p[:m], bool(p[m] <= p[:m].sum()), bool(abs(x64.mean()) <= MEAN_LIMIT * x64.std())


def bound(log2n):
    """c(log2n): per trial sum_k |P^[k] - P[k]| <= c sum_k P[k], derived by the route of
    period_ref.bound, for series whose Nyquist bin holds no more power than the M bins kept and whose mean is at most
    2^6 of their standard deviation.

      input   y = fl(x - mu^): u relative to |y| itself; mu^ - mu <= nsamp 2^-53 mean|x| (f64 sums in any order), and
              mean|x| <= |mu| + sigma <= (2^6 + 1) sigma under the second premise, so at nsamp <= 2^22 the mean's error
              is below 2^22 2^-53 2^7 sigma = 2^-24 sigma = u |y|_rms: b_in = 2 u.  (The short frames' 2^8 standard
              deviations would give 2 u only up to nsamp 2^20.)
      FFT     Higham, Accuracy and Stability, Thm 24.2 over t = log2 M radix-2 stages, eta = mu + gamma_4 (sqrt 2 + mu),
              mu = u the error of a once-rounded twiddle; the four-step twist is one more product with a once-rounded
              root between two stages, tau = mu + sqrt 2 gamma_3: (1 + eta)^t (1 + tau) - 1 <= b_fft = s / (1 - s),
              s = t eta + tau.  No twiddle is a product of two table entries.
      untangling and squaring: period_ref.bound's terms as they are."""
    t = log2n - 1
    mu = U
    gamma = lambda n: n * U / (1.0 - n * U)
    eta = mu + gamma(4) * (math.sqrt(2.0) + mu)
    tau = mu + math.sqrt(2.0) * gamma(3)
    s = t * eta + tau
    b_fft = s / (1.0 - s)
    b_in = 2.0 * U
    b_z = b_in + b_fft * (1.0 + b_in)
    b_u = 3.0 * U + mu + math.sqrt(2.0) * gamma(3)
    beta = math.sqrt(3.0) * (b_z + b_u * (1.0 + b_z))
    return 2.0 * beta + beta * beta + gamma(3) * (1.0 + beta) ** 2


def bound_bin(log2n):
    """b1(log2n) of period_ref.bound_bin for the four-step transform: the same per-term route with
    bound()'s b_fft, the twist one more once-rounded root on every path, (1 + eta)^t (1 + tau) - 1 <= s / (1 - s), s = t eta
    + tau; the 256-point columns' inner roots tw256[a q] stand for one of their eight stages' roots.  The assertion, the
    mean's term and the square's are period_ref.bin_allowance's: no premise on the Nyquist bin or on the mean."""
    t = log2n - 1
    gamma = lambda n: n * U / (1.0 - n * U)
    eta = U + gamma(4) * (math.sqrt(2.0) + U)
    tau = U + math.sqrt(2.0) * gamma(3)
    s = t * eta + tau
    return period_ref.path_bound(s / (1.0 - s))


def split(log2n):
    """(log2 M1, log2 M2) of M = M1 M2"""
    l1 = 4 if log2n <= 19 else 8
    return l1, log2n - 1 - l1


def geometry(log2n, seg, ntrials):
    """(workgroups over all trials, threads, LDS bytes: STAGES each; nseg)"""
    l1, l2 = split(log2n)
    m, m1, m2 = 1 << (log2n - 1), 1 << l1, 1 << l2
    cols = 64 if l1 == 4 else 16                 # the untangling's tile: columns k2
    per_trial = (64, m2 // 256 if l1 == 4 else m2 // 16, m1, m2 // (2 * cols), m // 16384, m // 16384)
    threads = (256, 256, max(64, m2 // 16), 256, 1024, 1024)
    lds = (32, 0 if l1 == 4 else 8 * 256 * 17, 8 * (m2 + m2 // 16), 8 * 2 * m1 * (cols + 1), 64, 8 * 5 * 16)
    return tuple(b * ntrials for b in per_trial), threads, lds, m // seg


def trial_bytes(log2n):
    """the workspace of a trial in flight"""
    return 12 * (1 << (log2n - 1)) + 512


def in_flight(log2n, max_trials):
    return min(max_trials, WORKSPACE_CAP // trial_bytes(log2n), 65535)


def samples(log2n, level, k):
    return float(1 << (log2n + level)) / float(k)
