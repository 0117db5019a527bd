"""include/rtlws_accel.h restated in numpy: the quadratic index map in exact integers, the resampled
series, and the search as periodlong_ref.power plus period_ref's whiten, sums and peaks over it.  The yardstick of
tests/test_accel_gpu.py.  The map only copies samples, so stage 1 is held to periodlong_ref.bound unchanged, its two
premises asked of the resampled series."""
from fractions import Fraction

import numpy as np

import period_ref
import periodlong_ref

MAX_NACCEL, MAX_COEF, MAX_VIRTUAL, STAGES = 1024, 1 << 40, 65536, 6
MAX_NSAMP = 1 << 22
LIGHT = 299792458                                # m / s
bound = periodlong_ref.bound
bound_bin = periodlong_ref.bound_bin             # per bin too: the map only copies samples
_LIMB = 22                                       # n, L - n < 2^22; |c| <= 2^40 in two limbs of 22 bits


def shift_exact(c, nsamp, n):
    """s_c(n) = floor((c n (L - n) + 2^63) / 2^64) in Python's integers: the definition itself"""
    last = nsamp - 1
    return (int(c) * int(n) * (last - int(n)) + (1 << 63)) >> 64


def shift(c, nsamp):
    """s_c(n), n = 0 .. nsamp - 1, int64 [nsamp], in exact integers from 22-bit limbs: c = sign (c1 2^22 + c0), n (L - n) =
    p1 2^22 + p0 with p1 < 2^22, so every partial product is below 2^44 and |c| n (L - n) = q2 2^44 + q1 2^22 + q0 with
    the q below 2^46.  floor((+-X + 2^63) / 2^64) is taken from X's integer part above 2^63 and whether anything lies
    below it: for c >= 0 (X + 2^63) >> 64; for c < 0 -((X + 2^63 - 1) >> 64) -- a half goes up for either sign."""
    c = int(c)
    assert abs(c) <= MAX_COEF and 1 <= nsamp <= MAX_NSAMP
    last = nsamp - 1
    n = np.arange(nsamp, dtype=np.int64)
    mask = (1 << _LIMB) - 1
    a, b = n, last - n                           # both below 2^22: the product below 2^44
    p = a * b
    p0, p1 = p & mask, p >> _LIMB
    mag = abs(c)
    c0, c1 = mag & mask, mag >> _LIMB            # c1 <= 2^18
    q0, q1, q2 = c0 * p0, c0 * p1 + c1 * p0, c1 * p1
    # X = q2 2^44 + q1 2^22 + q0 < 2^84; X = hi 2^44 + lo with lo < 2^44
    low = q0 + ((q1 & mask) << _LIMB)            # below 2^45
    hi = q2 + (q1 >> _LIMB) + (low >> 44)
    lo = low & ((1 << 44) - 1)
    # (X + 2^63) >> 64 = (hi + 2^19) >> 20 (lo < 2^44 does not carry); (X + 2^63 - 1) >> 64 = (hi + 2^19 - [lo == 0]) >> 20
    if c >= 0:
        return (hi + (1 << 19)) >> 20
    return -((hi + (1 << 19) - (lo == 0)) >> 20)


def index(c, nsamp):
    """f_c(n) = n + s_c(n), int64 [nsamp]; the properties the library's proof gives are asserted"""
    f = np.arange(nsamp, dtype=np.int64) + shift(c, nsamp)
    assert f[0] == 0 and f[-1] == nsamp - 1 and f.min() >= 0 and f.max() <= nsamp - 1 and np.all(np.diff(f) >= 0), c
    return f


def resample(x, coefs, nsamp=None):
    """R float32 [ntrials, naccel, nsamp] of x float32 [ntrials, >= nsamp]: R[t, a, n] = x[t, f_{coefs[a]}(n)]; nothing
    at or behind nsamp is looked at"""
    x = np.asarray(x, np.float32)
    assert x.ndim == 2
    nsamp = x.shape[1] if nsamp is None else nsamp
    return np.stack([x[:, index(c, nsamp)] for c in np.asarray(coefs, np.int64).reshape(-1)], axis=1)


def search(x, coefs, log2n, levels, norm, seg, klo, nsamp=None):
    """(power f64 [ntrials, naccel, M], white f32, best f32 [ntrials, naccel, levels, nseg], at int32) of the resampled
    series: periodlong_ref.power, rounded once to f32 for the stages behind it, then period_ref's stages 2 - 4"""
    r = resample(x, coefs, nsamp)
    nt, na, _ = r.shape
    power = np.stack([[periodlong_ref.power(r[t, a], log2n) for a in range(na)] for t in range(nt)])
    m = power.shape[-1]
    white, best, at = period_ref.period_ref(power.astype(np.float32).reshape(nt * na, m), levels, norm, seg, klo)
    return power, white.reshape(nt, na, m), best.reshape(nt, na, levels, -1), at.reshape(nt, na, levels, -1)


def _nearest(q):
    """the integer nearest a Fraction, a half away from zero"""
    mag = (abs(q) + Fraction(1, 2)).__floor__()
    return mag if q >= 0 else -mag


def coef(accel_m_s2, tsamp_s):
    """the integer nearest accel tsamp / (2 c) 2^64 from the doubles' exact values; None beyond +-2^40"""
    c = _nearest(Fraction(float(accel_m_s2)) * Fraction(float(tsamp_s)) * (1 << 64) / (2 * LIGHT))
    return c if abs(c) <= MAX_COEF else None


def coef_from_shift(mid_shift_samples, nsamp):
    """the integer nearest shift 4 / (nsamp - 1)^2 2^64 from the double's exact value; None beyond +-2^40"""
    c = _nearest(Fraction(float(mid_shift_samples)) * 4 * (1 << 64) / ((nsamp - 1) ** 2))
    return c if abs(c) <= MAX_COEF else None


def ties(nsamp, want=4):
    """[(c, n)] with c > 0 and c n (L - n) an exact odd multiple of 2^63, found by a search: n (L - n) = 2^j odd leaves c =
    2^(63 - j) odd', |c| <= 2^40, so j >= 23"""
    last, out = nsamp - 1, []
    n = np.arange(1, max(last, 1), dtype=np.int64)
    p = n * (last - n)
    for i in np.flatnonzero((p & -p) >= (1 << 23))[:want]:
        pi = int(p[i])
        c = 1 << (63 - ((pi & -pi).bit_length() - 1))
        assert (c * pi) % (1 << 64) == 1 << 63 and c <= MAX_COEF
        out.append((c, int(n[i])))
    return out


def geometry(log2n, seg, ntrials, naccel):
    return periodlong_ref.geometry(log2n, seg, ntrials * naccel)
