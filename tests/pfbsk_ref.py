"""The definition of include/rtlws_pfbsk.h restated in numpy on top of tests/pfb_ref.py and tests/pfbspec_ref.py: the
two sums of a sub-integration and the ratio K S2 / S1^2 in f64, the decision, the clean rows and their counts; the
decision and the clean sum once more in numpy f32, operation by operation as the header words them; the two host
helpers' formulas; and the fixed cases of tests/test_pfbsk_cpu.py and tests/test_pfbsk_gpu.py."""
import math

import numpy as np

import pfb_ref
import pfbspec_ref

MAX_K_AVG, MAX_NSUB = 65536, 65535
OPEN = (0.0, math.inf)                                    # ratio bounds under which nothing is flagged


def samples_needed(M, T, D, k_avg, nsub, nspectra):
    return pfb_ref.samples_needed(M, T, D, nspectra * nsub * k_avg)


# ---- the two host helpers ----------------------------------------------------------------------------------------------
def power_scale(taps):
    """2^(-2 ceil(log2(128 sum|h|))), 1 for an all-zero prototype."""
    s = 128 * int(np.abs(np.asarray(taps).astype(np.int64)).sum())
    return 1.0 if s == 0 else 2.0 ** (-2 * (s - 1).bit_length())


def bounds(k_avg, sk_lo, sk_hi):
    """ratio = 1 + sk (K - 1) / (K + 1) in double, rounded once -> (float32, float32)"""
    g = float(k_avg - 1) / float(k_avg + 1)
    with np.errstate(over="ignore"):
        return np.float32(1.0 + sk_lo * g), np.float32(1.0 + sk_hi * g)


def estimator(ratio, k_avg):
    """The spectral-kurtosis estimator of a ratio K S2 / S1^2: 1 for Gaussian noise, 0 for a steady carrier."""
    return (k_avg + 1.0) / (k_avg - 1.0) * (np.asarray(ratio, dtype=np.float64) - 1.0)


# ---- the definition in f64 ---------------------------------------------------------------------------------------------
def sub_sums(y, k_avg, scale):
    """y complex [nframes, M] -> (S1, S2) float64 [nframes // K, M]: sum P, and sum p^2 with p = P scale."""
    n = y.shape[0] // k_avg
    p = (y.real.astype(np.float64) ** 2 + y.imag.astype(np.float64) ** 2)[:n * k_avg].reshape(n, k_avg, y.shape[1])
    return p.sum(axis=1), ((p * scale) ** 2).sum(axis=1)


def ratio(s1, s2, k_avg, scale):
    """K S2 / S1^2 of the scaled sums; nan where S1 = 0."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return k_avg * np.asarray(s2, np.float64) / (np.asarray(s1, np.float64) * scale) ** 2


def flagged(s1, s2, k_avg, scale, ratio_lo, ratio_hi):
    """v < ratio_lo u or v > ratio_hi u, both false on NaN (0 times inf among them)."""
    u = (np.asarray(s1, np.float64) * scale) ** 2
    v = k_avg * np.asarray(s2, np.float64)
    with np.errstate(invalid="ignore"):
        return (v < float(ratio_lo) * u) | (v > float(ratio_hi) * u)


def clean_rows(s1, flags, nsub):
    """[n L, M] -> (C float64 [n, M], N uint32 [n, M]): the kept short rows added, and their number."""
    n, M = s1.shape[0] // nsub, s1.shape[1]
    keep = ~flags[:n * nsub].reshape(n, nsub, M)
    return np.where(keep, s1[:n * nsub].reshape(n, nsub, M), 0.0).sum(axis=1), keep.sum(axis=1).astype(np.uint32)


def pfbsk_ref(iq, k, taps, k_avg, nsub, ratio_lo=OPEN[0], ratio_hi=OPEN[1], scale=None, hop=None, shifted=False, nspectra=None):
    """iq uint8 [n, 2], taps int16 [T * M] -> (C [nspectra, M], N, S1 [nspectra L, M], S2), all of the f64 definition."""
    scale = power_scale(taps) if scale is None else scale
    nframes = None if nspectra is None else nspectra * nsub * k_avg
    s1, s2 = sub_sums(pfb_ref.pfb_ref(iq, k, taps, hop, 0, nframes), k_avg, scale)
    c, n = clean_rows(s1, flagged(s1, s2, k_avg, scale, ratio_lo, ratio_hi), nsub)
    out = (c, n, s1[:n.shape[0] * nsub], s2[:n.shape[0] * nsub])
    return tuple(np.fft.fftshift(x, axes=1) for x in out) if shifted else out


def db(clean, kept, scale, k_avg):
    """10 log10(C lin) in f64 with lin = fl(scale / fl((float)K (float)N)) per channel; N = 0 gives -inf."""
    kept = np.asarray(kept)
    with np.errstate(divide="ignore", invalid="ignore"):
        lin = np.float32(scale) / (np.float32(k_avg) * kept.astype(np.float32))
        d = 10.0 * np.log10(np.asarray(clean, dtype=np.float64) * lin.astype(np.float64))
    return np.where(kept == 0, -np.inf, d)


# ---- the decision and the clean sum in numpy f32, as the header words them ----------------------------------------------
def flagged_f32(s1, s2, k_avg, scale, ratio_lo, ratio_hi):
    """s = fl(S1 scale), u = fl(s s), v = fl((float)K S2); flagged <=> v < fl(ratio_lo u) or v > fl(ratio_hi u)."""
    f = np.float32
    s1, s2 = np.asarray(s1, dtype=f), np.asarray(s2, dtype=f)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        s = s1 * f(scale)
        u = s * s
        v = f(k_avg) * s2
        return (v < f(ratio_lo) * u) | (v > f(ratio_hi) * u)


def clean_rows_f32(s1, flags, nsub):
    """C = ((+0 + S1[l0]) + S1[l1]) + .. over the kept l ascending, in f32; N their number."""
    s1 = np.asarray(s1, dtype=np.float32)
    n, M = s1.shape[0] // nsub, s1.shape[1]
    c, cnt = np.zeros((n, M), np.float32), np.zeros((n, M), np.uint32)
    with np.errstate(over="ignore"):
        for l in range(nsub):
            keep = ~flags[l:n * nsub:nsub]
            c = np.where(keep, c + s1[l:n * nsub:nsub], c)
            cnt += keep.astype(np.uint32)
    return c, cnt


# ---- the semantic case --------------------------------------------------------------------------------------------------
# (log2 M, T, hop as a divisor of M, K, L) and the seed of each; two rows
SEMANTIC_SHAPES = ((6, 4, 1, 128, 8), (4, 3, 2, 300, 4), (10, 2, 1, 64, 4), (8, 4, 2, 100, 4))
SEMANTIC_SEEDS = (1, 2, 3, 4)
SEMANTIC_ROWS = 2
SK_LO, SK_HI = 0.5, 1.6
SIGMA, AMPLITUDE = 6.0, 40.0


def tone_channel(M):
    return M // 4 + 1


def burst_channel(M):
    return 3 * M // 4 - 2


def burst_subs(nsub):
    return (3, nsub + 1)


def gated_iq(k, T, D, k_avg, nsub, nspectra, seed):
    """A u8 capture: complex Gaussian noise of SIGMA per component, a steady tone of AMPLITUDE on the centre of
    tone_channel(M), and a tone of AMPLITUDE on the centre of burst_channel(M) that is on only in the first K // 10
    frames of the sub-integrations burst_subs(L): in the D samples each of those frames is the first to read."""
    M = 1 << k
    n = samples_needed(M, T, D, k_avg, nsub, nspectra)
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    z = SIGMA * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    z += AMPLITUDE * np.exp(2j * np.pi * tone_channel(M) * (t % M) / M)
    on = np.zeros(n, dtype=bool)
    for q in burst_subs(nsub):
        first = q * k_avg * D + T * M - D
        on[first:first + (k_avg // 10) * D] = True
    z += np.where(on, AMPLITUDE * np.exp(2j * np.pi * burst_channel(M) * (t % M) / M), 0.0)
    return np.clip(np.rint(np.stack([z.real, z.imag], axis=1)) + 128, 0, 255).astype(np.uint8)


def semantic_case(i):
    """-> (k, T, D, K, L, iq, taps, scale, ratio_lo, ratio_hi) of shape i"""
    k, T, hop_div, K, L = SEMANTIC_SHAPES[i]
    D = (1 << k) // hop_div
    taps = pfbspec_ref.designed_taps(k, T)
    iq = gated_iq(k, T, D, K, L, SEMANTIC_ROWS, SEMANTIC_SEEDS[i])
    return (k, T, D, K, L, iq, taps, power_scale(taps)) + bounds(K, SK_LO, SK_HI)


def near_a_bound(r, ratio_lo, ratio_hi, rel=0.01):
    """Where a f64 ratio lies within rel of either bound: there a f32 decision may differ from the f64 one."""
    r = np.asarray(r, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (np.abs(r - float(ratio_lo)) <= rel * float(ratio_lo)) | (np.abs(r - float(ratio_hi)) <= rel * float(ratio_hi))


# ---- the dB and payload cases of the GPU suite, checked on the CPU by test_pfbsk_cpu.py -----------------------------------
# pfbspec_ref.DB_SHAPES, every one with K in (3, tile + 1), L = 4, three rows and the semantic bounds; the capture is the
# semantic one (its steady tone is flagged everywhere: N = 0), the scale puts a full-scale tone at 118 dB
DB_NSUB, DB_ROWS = 4, 3
# Seeds of the captures, chosen so that fewer than 0.5 % of a case's finite f64 dB values lie within 2e-3 of an integer
DB_SEEDS = {(4, 3): 1, (4, 257): 2, (6, 3): 1, (6, 65): 2, (8, 3): 1, (8, 17): 1, (10, 3): 1, (10, 5): 3}


def db_case(k, T, hop_div, k_avg):
    """-> (iq, taps, D, scale, power_scale, ratio_lo, ratio_hi)"""
    D = (1 << k) // hop_div
    taps = pfbspec_ref.designed_taps(k, T)
    iq = gated_iq(k, T, D, k_avg, DB_NSUB, DB_ROWS, DB_SEEDS[(k, k_avg)])
    scale = 10.0 ** 11.8 / (128.0 * float(taps.astype(np.int64).sum())) ** 2
    return (iq, taps, D, scale, power_scale(taps)) + bounds(k_avg, SK_LO, SK_HI)
