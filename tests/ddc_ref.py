"""The arithmetic of include/rtlws_ddc.h restated in numpy (int64 throughout), and the ideal f64 mixer and block
sum it approximates.  The yardstick of tests/test_ddc_cpu.py and tests/test_ddc_gpu.py."""
import numpy as np

LOG2_P = 16
P = 1 << LOG2_P          # phase period
S = 1 << 14              # phasor scale
R_SET = (1, 2, 7, 8, 10, 12, 16, 128)
K_SET = (1, -1, 777, 12345, -20001, -32768, 32767)

_table = None


def table():
    """T[j] = (rint(S cos(2 pi j / P)), rint(S sin(2 pi j / P))) as int16 [P, 2]."""
    global _table
    if _table is None:
        a = 2.0 * np.pi * np.arange(P, dtype=np.float64) / P
        t = np.stack([np.rint(S * np.cos(a)), np.rint(S * np.sin(a))], axis=1).astype(np.int16)
        t.setflags(write=False)
        _table = t
    return _table


def ddc_ref(iq, R, words, first_dec_index=0):
    """iq uint8 [dec_len * R, 2], one tuning word per channel -> int32 [C, dec_len, 2]."""
    iq = np.asarray(iq, dtype=np.uint8).reshape(-1, 2)
    dec_len = iq.shape[0] // R
    assert dec_len * R == iq.shape[0] and 1 <= R <= 128 and first_dec_index >= 0
    T = table().astype(np.int64)
    x = iq.astype(np.int64).reshape(dec_len, R, 2) - 128
    a, b = x[..., 0], x[..., 1]
    n = np.arange(R, dtype=np.int64)
    g = (int(first_dec_index) + np.arange(dec_len, dtype=np.int64)) % P       # only the low 16 bits of k R g matter
    out = np.empty((len(words), dec_len, 2), dtype=np.int32)
    for ch, k in enumerate(words):
        k = int(k)
        assert -P // 2 <= k < P // 2
        c, s = T[(k * n) % P, 0], T[(k * n) % P, 1]
        ur = (a * c + b * s).sum(axis=1)
        ui = (b * c - a * s).sum(axis=1)
        assert np.abs(ur).max(initial=0) < 2 ** 31 and np.abs(ui).max(initial=0) < 2 ** 31
        blk = (((k * R) % P) * g) % P
        C, Sn = T[blk, 0], T[blk, 1]
        out[ch, :, 0] = (ur * C + ui * Sn + (1 << 27)) >> 28
        out[ch, :, 1] = (ui * C - ur * Sn + (1 << 27)) >> 28
    return out


def ddc_ideal(iq, R, words, first_dec_index=0):
    """The ideal mixer and block sum in f64: sum_n (x[m R + n] - 128 (1 + i)) exp(-2 pi i k (R g + n) / P), the phase
    reduced mod P in integers -> float64 [C, dec_len, 2]."""
    iq = np.asarray(iq, dtype=np.uint8).reshape(-1, 2)
    dec_len = iq.shape[0] // R
    x = iq.astype(np.float64).reshape(dec_len, R, 2) - 128.0
    z = x[..., 0] + 1j * x[..., 1]
    n = np.arange(R, dtype=np.int64)
    g = (int(first_dec_index) + np.arange(dec_len, dtype=np.int64)) % P
    out = np.empty((len(words), dec_len, 2), dtype=np.float64)
    for ch, k in enumerate(words):
        kp = int(k) % P
        phase = (kp * ((R * g)[:, None] % P + n[None, :])) % P
        y = (z * np.exp(-2j * np.pi * phase / P)).sum(axis=1)
        out[ch, :, 0], out[ch, :, 1] = y.real, y.imag
    return out


def block_sums(iq, R):
    """rtlws_cic_block_sums in numpy: int32 [dec_len, 2]."""
    iq = np.asarray(iq, dtype=np.uint8).reshape(-1, 2)
    return (iq.astype(np.int64).reshape(-1, R, 2) - 128).sum(axis=1).astype(np.int32)


def random_iq(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, 2), dtype=np.uint8)


def full_scale_iq(n, seed):
    """Every byte 0 or 255: the int32 headroom case at R = 128."""
    return (np.random.default_rng(seed).integers(0, 2, size=(n, 2), dtype=np.uint8) * 255).astype(np.uint8)
