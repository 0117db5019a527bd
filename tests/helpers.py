import numpy as np

# Error metric: per bin |got-ref| / max(|ref|, eps * max_bin(ref_row)).
# f32 cannot hold 1e-4 RELATIVE on bins arbitrarily far below the row maximum:
# next to a strong tone the partial sums reach ~N*amplitude and their f32 ulp
# sets an absolute error floor about 6e-8 of the peak amplitude (DESIGN.md,
# "Error budget").  So a single frame (K=1) is judged with eps = 1e-5 (bins
# more than 50 dB below the row maximum are held to the absolute error of a
# bin at that level); K-frame averages (K >= 6, the product's case) never have
# near-empty bins and are judged with the strict eps = 1e-9.
EPS_K1 = 1e-5
EPS_STRICT = 1e-9
TOL = 1e-4
# The reference-API paths (spectrum.h, cbb_main.h) and rtlws_spectra_batch_f64
# compute in double like the reference: they are held to the strict metric
# (eps = 1e-9) at every K, four orders inside north_star's 1e-4.
TOL_F64 = 1e-10
# Guard rails for the f32 batch kernel under the STRICT metric at K = 1 (what
# DESIGN.md "Error budget" reports: max 1.3e-3..3.5e-3, p99.9 3e-5..1.5e-4): a
# regression in the f32 arithmetic must not hide behind the relaxed floor.
STRICT_K1_P999 = 1e-4
STRICT_K1_MAX = 5e-3


def hash_bytes(n, seed):
    """n uniform bytes from a counter hash, uint8: byte i = top byte of splitmix64's finaliser of (seed << 40) + i + 1.
    Integer numpy operations only, so the bytes are the same on every machine: the input of the digest tests."""
    with np.errstate(over="ignore"):
        z = (np.arange(1, n + 1, dtype=np.uint64) + (np.uint64(seed) << np.uint64(40))) * np.uint64(0x9E3779B97F4A7C15)
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return (z >> np.uint64(56)).astype(np.uint8)


def eps_for(K):
    return EPS_K1 if K == 1 else EPS_STRICT


def rel_err(got, ref, eps=EPS_STRICT):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    floor = eps * np.abs(ref).max(axis=-1, keepdims=True)
    floor = np.where(floor > 0, floor, 1.0)       # all-zero rows: absolute error
    return np.abs(got - ref) / np.maximum(np.abs(ref), floor)


def strict_stats(got, ref):
    """(max, 99.9th percentile) of the strict-floor (eps = 1e-9) relative error."""
    e = rel_err(got, ref, EPS_STRICT)
    return float(e.max()), float(np.percentile(e, 99.9))


# f32 dB and payload rows (rtlws_spectra_batch's OUT_MEAN_DB / OUT_PAYLOAD_U8) against the f64 oracle's power sums
# `ref` (rows of K-frame sums).  The f32 error budget in dB of a bin of power p under a row maximum pmax is
# 4.34 * (2 * 6e-8 * sqrt(pmax / p)) ("Error budget"), taken with a 3x margin; the direct-sum kernel
# (fused=False, O(N^2) f32 accumulation) gets ten times that.

def f32_db_bad(got, ref, K, fused=True):
    """Mask of the dB values outside the budget, on bins above the strict floor (1e-9 of the row maximum)."""
    with np.errstate(divide="ignore"):
        want = 10 * np.log10(ref / K)
    mx = ref.max(axis=-1, keepdims=True)
    ok = np.isfinite(want) & (ref > 1e-9 * mx)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        tol_db = np.maximum(3e-4, 4.34 * 4e-7 * np.sqrt(mx / np.maximum(ref, 1e-300)))
        return ok & (np.abs(got - want) > (tol_db if fused else 10 * tol_db))


def f32_payload_bad(got, want, ref, K, gain, fused=True):
    """Mask of the bytes of one row that differ from the oracle's (`want`, src/cbb_main.c:121-130) other than by one
    where the f64 dB value sits within the budget of an integer ((int) truncation is discontinuous there)."""
    diff = got.astype(int) - want.astype(int)
    g = 10.0 ** (int(gain / 10))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = 10 * np.log10(np.abs(g * ref / K))
        tol_db = np.maximum(2e-3, 4.34 * 4e-7 * np.sqrt(ref.max() / np.maximum(ref, 1e-300)))
        near = np.abs(d - np.round(d)) < (tol_db if fused else 10 * tol_db)
    return ~((diff == 0) | (near & (np.abs(diff) == 1)))
