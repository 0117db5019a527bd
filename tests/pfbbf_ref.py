"""The definition of include/rtlws_pfbbf.h restated in numpy on top of tests/pfb_ref.py: the beams Z_b = sum_a W[b][a] Y_a
in f64, their K-frame powers; the derived bounds; the definition's f32 arithmetic in the definition's order, for the
bit-for-bit comparisons; the weights and captures of the delay case.  The yardstick of tests/test_pfbbf_cpu.py and
tests/test_pfbbf_gpu.py."""
import numpy as np

import pfb_ref
import pfbspec_ref
import pfbxc_ref

TILE_POINTS = 4096         # the filter bank's tile: F = TILE_POINTS / M frames
LDS_BYTES = 34816          # one tile, whatever A and B are
U = 2.0 ** -24


def tile_frames(M):
    return TILE_POINTS // M


def spectra_per_block(M, k_avg):
    F = tile_frames(M)
    return 1 if k_avg >= F else F // k_avg


def samples_needed(M, T, D, k_avg, count):
    """Per capture.  k_avg = 0: voltage mode, count frames; else power mode, count spectra of k_avg frames."""
    return pfb_ref.samples_needed(M, T, D, count if k_avg == 0 else count * k_avg)


def grid(M, k_avg, count):
    """-> (workgroups, threads, LDS bytes, frames or spectra per workgroup)"""
    per = tile_frames(M) if k_avg == 0 else spectra_per_block(M, k_avg)
    return -(-count // per), 256, LDS_BYTES, per


def signs(M, D, first_frame_index, nframes):
    """The half hop's sign rule (-1)^(c g), g = first_frame_index + m -> float64 [nframes, M] of +-1."""
    s = np.ones((nframes, M))
    if D != M:
        g = first_frame_index + np.arange(nframes, dtype=np.int64)
        s[np.ix_(g % 2 == 1, np.arange(M) % 2 == 1)] = -1.0
    return s


def frames_of(iqs, k, taps, hop=None, nframes=None):
    """Y_a of every capture BEFORE the sign rule, complex128 [nframes, M].  One array given twice is channelized once."""
    M = 1 << k
    D = M if hop is None else int(hop)
    done = {}
    for x in iqs:
        if id(x) not in done:
            y = pfb_ref.pfb_ref(x, k, taps, D, 0, nframes)
            done[id(x)] = y * signs(M, D, 0, y.shape[0])
    return [done[id(x)] for x in iqs]


def beams(ys, W):
    """ys: A arrays complex [nframes, M], W complex [B, A, M] -> complex128 [B, nframes, M]: Z_b = sum_a W[b][a] Y_a."""
    W = np.asarray(W, dtype=np.complex128)
    assert W.ndim == 3 and W.shape[1] == len(ys)
    z = np.zeros((W.shape[0],) + ys[0].shape, dtype=np.complex128)
    for a, y in enumerate(ys):
        z += W[:, a, None, :] * np.asarray(y, dtype=np.complex128)[None]
    return z


def pfbbf_ref(iqs, W, k, taps, hop=None, first_frame_index=0, nframes=None):
    """Voltage mode: iqs A captures uint8 [n, 2], W complex [B, A, M], taps int16 [T * M] -> complex128
    [B, nframes, M], time-major (channel-major is the transpose of every beam)."""
    M = 1 << k
    D = M if hop is None else int(hop)
    z = beams(frames_of(iqs, k, taps, D, nframes), W)
    return z * signs(M, D, first_frame_index, z.shape[1])[None]


def k_sums(z, k_avg, shifted=False):
    """z complex [B, nframes, M] -> float64 [nframes // k_avg, B, M]: row j B + b is the sum over K frames of |Z_b|^2."""
    B, nframes, M = z.shape
    n = nframes // k_avg
    p = z.real.astype(np.float64) ** 2 + z.imag.astype(np.float64) ** 2
    s = p[:, :n * k_avg].reshape(B, n, k_avg, M).sum(axis=2).transpose(1, 0, 2)
    return np.fft.fftshift(s, axes=2) if shifted else s


def pfbbf_power_ref(iqs, W, k, taps, k_avg, hop=None, shifted=False, nspectra=None):
    """Power mode -> float64 [nspectra, B, M].  The sign rule does not reach the power."""
    nframes = None if nspectra is None else nspectra * k_avg
    return k_sums(beams(frames_of(iqs, k, taps, hop, nframes), W), k_avg, shifted)


# ---- the bounds -----------------------------------------------------------------------------------------------------

def bound(k, A):
    """Per (frame, beam): ||got - ref||_2 <= bound * N, N = sum_a wmax[b][a] ||Y_a,ref[m]||_2, wmax[b][a] = max_c |W[b][a][c]|.
    DESIGN.md 4.17.  The device's Y_a errs by eps ||Y_a||_2, eps = 8 (log2 M + 1) u (pfb_ref.bound).  A complex product
    of four products and two sums errs, component-wise, by gamma_2 (|wr yr| + |wi yi|) and gamma_2 (|wr yi| + |wi yr|),
    in modulus by sqrt(2) gamma_2 |w| |y| < 3 u |w| |y|.  A sequential A-term sum from +0 (the first addition is
    exact) errs per component by (A - 1) u sum |t_a|, so in modulus by (A - 1) u sum_a |t_a| (Minkowski).  Per channel
    |got - ref| <= sum_a |w| (|e_a| + (A + 2) u |Y_a|) up to second order, and over the channels
    (eps + (A + 2) u) N; one more u covers the products of these terms."""
    return (8.0 * (k + 1) + A + 3.0) * U


def power_bound(k, A, k_avg):
    """Per row: ||got - ref||_1 <= power_bound * sum_{m < K} N[m]^2, N as in bound().  With d = bound(k, A):
    ||Z||_2 <= N (the triangle inequality), so sum_c | |got Z|^2 - |Z|^2 | <= ||got Z - Z||_2 (||got Z||_2 + ||Z||_2)
    <= (2 d + d^2) N^2; the three roundings of P give 2 u |got Z|^2 and a K-term f32 sum of non-negative terms
    (K - 1) u: the derivation of pfbspec_ref.bound with d in the place of eps.  It is relative to N, not to ||Z||:
    a nulled beam is covered."""
    return (16.0 * (k + 1) + 2.0 * A + k_avg + 10.0) * U


def norms(ys, W):
    """N[b][m] = sum_a wmax[b][a] ||Y_a[m]||_2 -> float64 [B, nframes]"""
    wmax = np.abs(np.asarray(W, dtype=np.complex128)).max(axis=2)                   # [B, A]
    yn = np.stack([np.linalg.norm(np.asarray(y, dtype=np.complex128), axis=1) for y in ys])   # [A, nframes]
    return wmax @ yn


def voltage_ratio(got, ref, ys, W, k):
    """max over (beam, frame) of ||got - ref||_2 / (bound N); got, ref [B, nframes, M] time-major."""
    err = np.linalg.norm(np.asarray(got, dtype=np.complex128) - ref, axis=2)
    N = norms(ys, W)
    assert not err[N <= 0].any()
    ok = N > 0
    return float((err[ok] / (bound(k, len(ys)) * N[ok])).max()) if ok.any() else 0.0


def power_ratio(got, ref, ys, W, k, k_avg):
    """max over the rows of ||got - ref||_1 / (power_bound sum_m N^2); got, ref [n, B, M]."""
    n = ref.shape[0]
    N2 = (norms(ys, W)[:, :n * k_avg] ** 2).reshape(-1, n, k_avg).sum(axis=2).T     # [n, B]
    err = np.abs(np.asarray(got, dtype=np.float64) - ref).sum(axis=2)
    assert not err[N2 <= 0].any()
    ok = N2 > 0
    return float((err[ok] / (power_bound(k, len(ys), k_avg) * N2[ok])).max()) if ok.any() else 0.0


# ---- the definition's f32 arithmetic, for the comparisons without a tolerance -------------------------------------

SIGN_BIT = np.uint32(0x80000000)


def flip(y, M, D, first_frame_index):
    """complex64 [.., nframes, M]: the sign rule as a flip of both sign bits (its own inverse)."""
    y = np.array(y, dtype=np.complex64)
    mask = signs(M, D, first_frame_index, y.shape[-2]) < 0
    v = y.view(np.uint32).reshape(y.shape + (2,))
    v[..., mask, :] ^= SIGN_BIT
    return y


def beams_f32(ys, W):
    """ys: A arrays complex64 [nframes, M] before the sign rule, W complex64 [B, A, M] -> complex64 [B, nframes, M]:
    t_a = (fl(fl(wr yr) - fl(wi yi)), fl(fl(wr yi) + fl(wi yr))), summed a ascending from +0, every operation f32."""
    W = np.asarray(W, dtype=np.complex64)
    B = W.shape[0]
    zr = np.zeros((B,) + ys[0].shape, dtype=np.float32)
    zi = np.zeros_like(zr)
    for a, y in enumerate(ys):
        yr, yi = np.ascontiguousarray(y.real, dtype=np.float32)[None], np.ascontiguousarray(y.imag, dtype=np.float32)[None]
        wr = np.ascontiguousarray(W[:, a].real, dtype=np.float32)[:, None, :]
        wi = np.ascontiguousarray(W[:, a].imag, dtype=np.float32)[:, None, :]
        zr = zr + ((wr * yr) - (wi * yi))
        zi = zi + ((wr * yi) + (wi * yr))
    assert zr.dtype == np.float32
    out = np.empty(zr.shape, dtype=np.complex64)
    out.real, out.imag = zr, zi
    return out


def powers_f32(z):
    """complex64 -> float32: fl(fl(zr zr) + fl(zi zi))"""
    zr, zi = np.ascontiguousarray(z.real, dtype=np.float32), np.ascontiguousarray(z.imag, dtype=np.float32)
    return (zr * zr) + (zi * zi)


def power_f32(z, k, k_avg, shifted=False):
    """z complex64 [B, nframes, M] (voltages, with or without the sign rule) -> float32 [n, B, M]: the f32 products
    summed in the spectrometer's order (pfbxc_ref.ordered_sums)."""
    s = np.stack([pfbxc_ref.ordered_sums(powers_f32(zb), k, k_avg) for zb in z], axis=1)
    return np.fft.fftshift(s, axes=2) if shifted else s


# ---- weights and captures ---------------------------------------------------------------------------------------------

def random_weights(B, A, M, seed):
    """complex64 [B, A, M], |w| <= 2, every phase."""
    rng = np.random.default_rng(seed)
    w = 1.999 * rng.random((B, A, M)) * np.exp(2j * np.pi * rng.random((B, A, M)))
    return w.astype(np.complex64)


def one_hot(B, A, M, which):
    """complex64 [B, A, M]: beam b passes capture which[b] with weight 1 + 0i; every other weight is 0."""
    w = np.zeros((B, A, M), dtype=np.complex64)
    for b, a0 in enumerate(which):
        w[b, a0] = 1.0
    return w


def random_captures(A, n, seed):
    return [pfb_ref.random_iq(n, seed=seed + 1000 * a) for a in range(A)]


def signed_channels(M):
    c = np.arange(M)
    return np.where(c >= M // 2, c - M, c)


def steering(M, delays):
    """complex64 [A, M]: e^(+2 pi i c d_a / M) / A, c signed: undoes the phase slope of a capture that lags by d_a samples."""
    d = np.asarray(delays, dtype=np.float64)[:, None]
    return (np.exp(2j * np.pi * signed_channels(M)[None] * d / M) / len(delays)).astype(np.complex64)


def delay_case():
    """M = 64, T = 8, the designed prototype, hop M, K = 65, one spectrum; the captures are
    pfbxc_ref.delayed_captures(4, n, seed=9): one noise capture delayed by 0, 1, 3, 6 samples, each with noise of its own.
    -> (k, taps, hop, K, the four captures,
        W_steer complex64 [2, 4, M]: beam 0 the steering weights, beam 1 one element of it (capture 0 at 1 / A),
        W_null  complex64 [2, 2, M] over captures 0 and 1: beam 0 = (1, -e^(+2 pi i c / M)), beam 1 = capture 0 alone)"""
    k, T, K = 6, 8, 65
    M = 1 << k
    taps = pfbspec_ref.designed_taps(k, T)
    iqs = pfbxc_ref.delayed_captures(4, samples_needed(M, T, M, K, 1), seed=9)
    w_steer = np.zeros((2, 4, M), dtype=np.complex64)
    w_steer[0] = steering(M, pfbxc_ref.DELAYS)
    w_steer[1, 0] = 1.0 / 4
    w_null = one_hot(2, 2, M, (0, 0))
    w_null[0, 1] = -(2 * steering(M, pfbxc_ref.DELAYS[:2])[1])
    return k, taps, M, K, iqs, w_steer, w_null


def delay_figures(steer_rows, null_rows):
    """rows [B, M] of one spectrum -> (the steered beam's power over one element's: the array's power gain, A^2 for
    equal captures without noise of their own; the nulled beam's power over capture 0's)."""
    s, n = np.asarray(steer_rows, dtype=np.float64), np.asarray(null_rows, dtype=np.float64)
    return float(s[0].sum() / s[1].sum()), float(n[0].sum() / n[1].sum())


# The restatement's own figures for delay_case() (tests/test_pfbbf_cpu.py computes them again and holds them to
# these), and the thresholds of the physical assertions: half the gain, double the depth.  Measured on the f64
# restatement: gain 15.3708 (A^2 = 16 less the captures' own noise), depth 0.074717 (the own noise of two captures,
# 2 * 36 / 936 = 0.077).  The steering weights carry 1 / A, so against capture 0 at weight 1 the steered beam has the
# power 0.9607: the gain is stated against one element of the same beam, weight 1 / A, which is what the array adds
STEER_GAIN, NULL_DEPTH = 15.3708, 0.074717
STEER_GAIN_MIN, NULL_DEPTH_MAX = STEER_GAIN / 2.0, NULL_DEPTH * 2.0
