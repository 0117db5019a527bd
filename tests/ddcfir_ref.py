"""The arithmetic of include/rtlws_ddcfir.h restated in numpy (int64 throughout), the ideal f64 mixer and FIR it
approximates, the bound between the two, the design formula of rtlws_ddcfir_design and the
selectivity measurement.  The yardstick of tests/test_ddcfir_cpu.py and tests/test_ddcfir_gpu.py."""
import numpy as np

import ddc_ref

P = ddc_ref.P
MAX_TAP = 32639
MAX_TAPS = 256
K_SET = (0, 1, -1, 777, -20001, 32767, -32768)
# the (decim, ntaps) at which the GPU suites hold the kernels that form a filtered sample to the restatement
# (tests/test_ddcfir_gpu.py's matrix, tests/fmfir_ref.py's stage-A matrix): every R of R_AXIS with every L of l_axis(R)
R_AXIS = (1, 3, 8, 10, 12, 16, 17, 128)


def l_axis(R):
    return sorted({1, R, R + 1, 17, 33, min(8 * R, 256), 255, 256})


def aligned(R, L):
    """the kernels' instantiation: decim and ntaps multiples of four (8-byte window loads)"""
    return R % 4 == 0 and L % 4 == 0


def samples_needed(R, L, dec_len):
    return (dec_len - 1) * R + L if dec_len > 0 else 0


def _windows(iq, R, L, dec_len):
    """(a, b) int64 [dec_len, L]: re - 128 and im - 128 of the window of every decimated sample."""
    iq = np.asarray(iq, dtype=np.uint8).reshape(-1, 2)
    if dec_len is None:
        dec_len = (iq.shape[0] - L) // R + 1 if iq.shape[0] >= L else 0
    assert samples_needed(R, L, dec_len) <= iq.shape[0]
    idx = np.arange(dec_len, dtype=np.int64)[:, None] * R + np.arange(L, dtype=np.int64)[None, :]
    x = iq.astype(np.int64) - 128
    return x[idx, 0], x[idx, 1], dec_len


def ddcfir_ref(iq, R, taps, words, out_shift=14, first_dec_index=0, dec_len=None):
    """iq uint8 [>= (dec_len - 1) R + L, 2], taps int16 [L], one tuning word per channel -> int32 [C, dec_len, 2]."""
    h = np.asarray(taps).astype(np.int64).reshape(-1)
    L, s = h.size, int(out_shift)
    assert 1 <= R <= 128 and 1 <= L <= MAX_TAPS and 0 <= s <= 30 and first_dec_index >= 0
    assert np.abs(h).max() <= MAX_TAP
    a, b, dec_len = _windows(iq, R, L, dec_len)
    T = ddc_ref.table().astype(np.int64)
    n = np.arange(L, dtype=np.int64)
    g = (int(first_dec_index) + np.arange(dec_len, dtype=np.int64)) % P       # only the low 16 bits of k R g matter
    out = np.empty((len(words), dec_len, 2), dtype=np.int32)
    for ch, k in enumerate(words):
        k = int(k)
        assert -P // 2 <= k < P // 2
        gc = (h * T[(k * n) % P, 0] + (1 << 13)) >> 14
        gs = (h * T[(k * n) % P, 1] + (1 << 13)) >> 14
        assert np.all(np.abs(gc) <= np.abs(h)) and np.all(np.abs(gs) <= np.abs(h))
        ur = a @ gc + b @ gs
        ui = b @ gc - a @ gs
        assert max(np.abs(ur).max(initial=0), np.abs(ui).max(initial=0)) <= 128 * (np.sqrt(2.0) * np.abs(h).sum() + 2 * L)
        blk = (((k * R) % P) * g) % P
        cb, sb = T[blk, 0], T[blk, 1]
        vr = (ur * cb + ui * sb + (1 << (13 + s))) >> (14 + s)
        vi = (ui * cb - ur * sb + (1 << (13 + s))) >> (14 + s)
        assert max(np.abs(vr).max(initial=0), np.abs(vi).max(initial=0)) <= 182 * (np.abs(h).sum() + L) / 2.0 ** s + 1
        out[ch, :, 0], out[ch, :, 1] = vr, vi
    return out


def ddcfir_ideal(iq, R, taps, words, out_shift=14, first_dec_index=0, dec_len=None):
    """2^-s sum_n h[n] (x[m R + n] - 128 (1 + i)) exp(-2 pi i k (g R + n) / P) in f64, the phase reduced mod P in
    integers -> float64 [C, dec_len, 2]."""
    h = np.asarray(taps).astype(np.float64).reshape(-1)
    L = h.size
    a, b, dec_len = _windows(iq, R, L, dec_len)
    z = (a + 1j * b) * h[None, :]
    n = np.arange(L, dtype=np.int64)
    g = (int(first_dec_index) + np.arange(dec_len, dtype=np.int64)) % P
    out = np.empty((len(words), dec_len, 2), dtype=np.float64)
    for ch, k in enumerate(words):
        kp = int(k) % P
        phase = (kp * ((R * g)[:, None] % P + n[None, :])) % P
        y = (z * np.exp(-2j * np.pi * phase / P)).sum(axis=1) / 2.0 ** int(out_shift)
        out[ch, :, 0], out[ch, :, 1] = y.real, y.imag
    return out


def bound(taps, out_shift):
    """|ddcfir_ref - ddcfir_ideal| per component at most: G's own rounding (1/2 per part) and the
    table's rounding scaled by |h| / 16384 (|h| / 2^15 per part) against |a| + |b| <= 256, through the block rotation
    (sqrt(2)); the block phasor's rounding against |U| <= 182 (sum|h| + L); the output rounding (1/2)."""
    sh = float(np.abs(np.asarray(taps).astype(np.int64)).sum())
    L = np.asarray(taps).size
    return 0.5 + np.sqrt(2.0) * (sh / 128.0 + 128.0 * L + 182.0 * (sh + L) / 32768.0) / 2.0 ** int(out_shift)


def design(R, L):
    """rtlws_ddcfir_design's documented formula, evaluated by numpy."""
    n = np.arange(L, dtype=np.float64)
    w = np.ones(1) if L == 1 else 0.54 - 0.46 * np.cos(2.0 * np.pi * n / (L - 1))
    p = np.sinc((n - (L - 1) / 2.0) / R) * w
    a = min(16384.0 * R / p.sum(), MAX_TAP / np.abs(p).max())
    return np.rint(a * p).astype(np.int16)


def boxcar(R):
    """L = R taps of 16384: with out_shift = 14 the bank is rtlws_ddc_run."""
    return np.full(R, 16384, dtype=np.int16)


def tone_iq(n, word, amplitude=100.0):
    """A u8 capture of one complex tone at `word` / P cycles per sample."""
    ph = 2.0 * np.pi * ((int(word) * np.arange(n, dtype=np.int64)) % P) / P
    return (np.rint(amplitude * np.stack([np.cos(ph), np.sin(ph)], axis=1)) + 128).astype(np.uint8)


SELECTIVITY_R = 12
SELECTIVITY_CENTRE = 5000                                 # the channel's word
SELECTIVITY_OFFSET = 3 * P // (2 * SELECTIVITY_R)         # 1.5 / R cycles per sample: 8192 words, exactly


def selectivity_db(run, taps, dec_len=600):
    """Mean output power of a tone 1.5 output bandwidths off the centre of an R = 12 channel relative to the same tone
    at the centre, in dB.  run(iq, R, taps, words, out_shift) -> int32 [1, dec_len, 2]: the restatement or the device."""
    R = SELECTIVITY_R
    n = samples_needed(R, np.asarray(taps).size, dec_len)
    power = []
    for word in (SELECTIVITY_CENTRE, SELECTIVITY_CENTRE + SELECTIVITY_OFFSET):
        y = run(tone_iq(n, word), R, taps, [SELECTIVITY_CENTRE], 14).astype(np.float64)
        power.append((y ** 2).sum(axis=2).mean())
    return 10.0 * np.log10(power[1] / power[0])


def random_taps(L, seed):
    return np.random.default_rng(seed).integers(-MAX_TAP, MAX_TAP + 1, L).astype(np.int16)


random_iq = ddc_ref.random_iq
full_scale_iq = ddc_ref.full_scale_iq
