"""The definition of include/rtlws_pfbspec.h restated in numpy on top of tests/pfb_ref.py: |Y|^2 in f64, summed over
K frames; the dB and byte forms in f64; the derived bound.  The yardstick of tests/test_pfbspec_cpu.py and
tests/test_pfbspec_gpu.py."""
import numpy as np

import pfb_ref

OUT_POWER_SUM, OUT_MEAN_DB, OUT_PAYLOAD_U8 = 0, 1, 2      # enum rtlws_output


def samples_needed(M, T, D, k_avg, nspectra):
    return pfb_ref.samples_needed(M, T, D, nspectra * k_avg)


def k_sums(y, k_avg, shifted=False):
    """y complex [nframes, M] -> float64 [nframes // k_avg, M]: sum over K consecutive frames of |y|^2."""
    n = y.shape[0] // k_avg
    p = y.real.astype(np.float64) ** 2 + y.imag.astype(np.float64) ** 2
    s = p[:n * k_avg].reshape(n, k_avg, y.shape[1]).sum(axis=1)
    return np.fft.fftshift(s, axes=1) if shifted else s


def pfbspec_ref(iq, k, taps, k_avg, hop=None, shifted=False, nspectra=None):
    """iq uint8 [n, 2], taps int16 [T * M] -> float64 [nspectra, M], the K-frame power sums.  The sign rule of the
    half hop does not reach the power: first_frame_index = 0."""
    nframes = None if nspectra is None else nspectra * k_avg
    return k_sums(pfb_ref.pfb_ref(iq, k, taps, hop, 0, nframes), k_avg, shifted)


def spectrometer(x, k, taps, k_avg, hop=None, shifted=False):
    """The definition on a complex f64 signal x (unquantised) -> float64 [nspectra, M]."""
    return k_sums(pfb_ref.channelize(x, k, taps, hop), k_avg, shifted)


def lin_f32(scale, k_avg):
    """lin = fl(scale / (float)K) as the library forms it on the host."""
    return np.float32(scale) / np.float32(k_avg)


def db(sums, scale, k_avg):
    """10 log10(S lin) in f64 from the f32 lin; S = 0 gives -inf."""
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(np.asarray(sums, dtype=np.float64) * float(lin_f32(scale, k_avg)))


def payload(db_values):
    """The dB value truncated toward zero and clamped to 0 .. 255 (cbb_get_spectrum_payload); -inf gives 0."""
    d = np.asarray(db_values, dtype=np.float64)
    return np.trunc(np.clip(np.where(np.isnan(d), -1.0, d), 0.0, 255.0)).astype(np.uint8)


def near_integer(db_values, eps=1e-3):
    """Where the f64 dB value lies within eps of an integer: rtlws_hip.h lets the byte differ by one there."""
    d = np.asarray(db_values, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (np.abs(d - np.rint(d)) < eps)


def bound(k, k_avg):
    """Per row: ||got - ref||_1 <= bound * ||ref||_1.  DESIGN.md 4.15: the transform's eps = 8 (log2 M + 1) u gives
    (2 eps + eps^2) ||Y||_2^2, the three roundings of P give 2 u, a K-term f32 sum of non-negative terms (K - 1) u."""
    return (16.0 * (k + 1) + k_avg + 4.0) * 2.0 ** -24


def tone_noise_iq(n, cycles_per_sample, seed, amplitude=60.0, sigma=12.0):
    """A u8 capture of one complex tone in Gaussian noise: a spectrum with a peak, so that a permuted row shows."""
    rng = np.random.default_rng(seed)
    ph = 2.0 * np.pi * cycles_per_sample * np.arange(n, dtype=np.float64)
    z = amplitude * np.exp(1j * ph) + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return np.clip(np.rint(np.stack([z.real, z.imag], axis=1)) + 128, 0, 255).astype(np.uint8)


# ---- the dB and payload cases of the GPU suite (test_db_and_bytes), checked on the CPU by test_pfbspec_cpu.py --------
# (log2 M, T, hop as a divisor of M); every one with K in (3, tile + 1) and five spectra
DB_SHAPES = ((4, 7, 1), (6, 8, 2), (8, 8, 1), (10, 4, 2))
DB_NSPECTRA = 5
# Seeds of the captures, chosen so that fewer than 0.5 % of a case's f64 dB values lie within 2e-3 of an integer
# (a uniform fraction would put 0.4 % there: with 80 values a case needs none)
DB_SEEDS = {(4, 3): 1, (4, 257): 1, (6, 3): 2, (6, 65): 2, (8, 3): 4, (8, 17): 5, (10, 3): 22, (10, 5): 24}


def designed_taps(k, T):
    """pfb_ref.design rounded: the prototype of rtlws_pfb_design up to ties."""
    return np.rint(pfb_ref.design(k, T)).astype(np.int16)


def db_case(k, T, hop_div, k_avg):
    """-> (iq, taps, hop, scale): a tone of amplitude 100, 0.3 channels off a centre, in noise of sigma 1.5; scale puts
    a tone on a centre at 118 dB, so the rows span roughly 30 .. 118 dB."""
    M = 1 << k
    D = M // hop_div
    taps = designed_taps(k, T)
    n = samples_needed(M, T, D, k_avg, DB_NSPECTRA)
    iq = tone_noise_iq(n, (M // 4 + 1.3) / M, DB_SEEDS[(k, k_avg)], amplitude=100.0, sigma=1.5)
    scale = 10.0 ** 11.8 / (100.0 * float(taps.astype(np.int64).sum())) ** 2
    return iq, taps, D, scale


def leakage_db_of_row(row, c0):
    """pfb_ref.leakage_db on a power row: the largest power two or more channels from both neighbours of the tone,
    relative to channel c0."""
    M = row.shape[0]
    c = np.arange(M)
    d0 = np.minimum((c - c0) % M, (c0 - c) % M)
    d1 = np.minimum((c - c0 - 1) % M, (c0 + 1 - c) % M)
    far = (d0 >= 2) & (d1 >= 2)
    return 10.0 * np.log10(row[far].max() / row[c0])
