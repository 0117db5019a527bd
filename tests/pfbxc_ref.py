"""The definition of include/rtlws_pfbxc.h restated in numpy on top of tests/pfb_ref.py: |Y_a|^2 and Y_a conj(Y_b) in
f64, summed over K frames; the derived bound; an f32 stand-in for the device in the definition's order of
operations; the captures of the delay and multi-receiver cases.  The yardstick of tests/test_pfbxc_cpu.py and
tests/test_pfbxc_gpu.py."""
import numpy as np

import pfb_ref
import pfbspec_ref

TILE_POINTS = 4096         # the filter bank's tile: F = TILE_POINTS / M frames


def samples_needed(M, T, D, k_avg, nspectra):
    """Per capture: the spectrometer's figure."""
    return pfbspec_ref.samples_needed(M, T, D, k_avg, nspectra)


def pairs(A):
    """The pairs a < b row-major: (0,1), (0,2), .., (1,2), ..: the order of a spectrum's cross rows."""
    return [(a, b) for a in range(A) for b in range(a + 1, A)]


def pair_index(A, a, b):
    return pairs(A).index((a, b)) if 2 <= A <= 4 and 0 <= a < b < A else -1


def xc_sums(ys, k_avg, shifted=False):
    """ys: A arrays complex [nframes, M] -> (float64 [n, A, M], complex128 [n, NX, M]) with n = nframes // k_avg: the
    sums over K consecutive frames of |Y_a|^2 and of Y_a conj(Y_b)."""
    A, (nframes, M) = len(ys), ys[0].shape
    n = nframes // k_avg
    ys = [np.asarray(y, dtype=np.complex128)[:n * k_avg].reshape(n, k_avg, M) for y in ys]
    autos = np.stack([(y.real ** 2 + y.imag ** 2).sum(axis=1) for y in ys], axis=1)
    # the products spelled out in real f64 (numpy's complex product may fuse): the same capture twice gives im = 0
    # exactly, and swapping a pair conjugates its row exactly
    cross = np.stack([(ys[a].real * ys[b].real + ys[a].imag * ys[b].imag).sum(axis=1)
                      + 1j * (ys[a].imag * ys[b].real - ys[a].real * ys[b].imag).sum(axis=1) for a, b in pairs(A)], axis=1)
    if shifted:
        autos, cross = np.fft.fftshift(autos, axes=2), np.fft.fftshift(cross, axes=2)
    return autos, cross


def frames_of(iqs, k, taps, hop=None, nframes=None):
    """Y_a of every capture, first_frame_index = 0 (the sign rule multiplies Y_a and Y_b alike and reaches no
    product).  One array given twice is channelized once."""
    done = {}
    for x in iqs:
        if id(x) not in done:
            done[id(x)] = pfb_ref.pfb_ref(x, k, taps, hop, 0, nframes)
    return [done[id(x)] for x in iqs]


def pfbxc_ref(iqs, k, taps, k_avg, hop=None, shifted=False, nspectra=None):
    """iqs: A captures uint8 [n, 2], taps int16 [T * M] -> (autos float64 [nspectra, A, M], cross complex128
    [nspectra, NX, M])."""
    nframes = None if nspectra is None else nspectra * k_avg
    return xc_sums(frames_of(iqs, k, taps, hop, nframes), k_avg, shifted)


def bound(k, k_avg):
    """Per cross row, |.| the complex modulus: sum_c |got - ref| <= bound * sqrt(||ref S_a||_1 ||ref S_b||_1).
    DESIGN.md 4.16: the transform's eps = 8 (log2 M + 1) u gives (2 eps + eps^2) ||Y_a||_2 ||Y_b||_2 per frame
    (Cauchy-Schwarz), the three roundings of a component 2 u |Y_a| |Y_b|, a K-term f32 sum (K - 1) u sum |terms| per
    component; Cauchy-Schwarz over the frames turns sum_m ||Y_a|| ||Y_b|| into sqrt(||S_a||_1 ||S_b||_1).  The auto
    rows keep pfbspec_ref.bound."""
    return (16.0 * (k + 1) + 2.0 * k_avg + 6.0) * 2.0 ** -24


def cross_ratio(got, ref_autos, ref_cross, k, k_avg):
    """max over the cross rows of sum_c |got - ref| / (bound sqrt(||S_a||_1 ||S_b||_1)); got [n, NX, M]."""
    A = ref_autos.shape[1]
    worst = 0.0
    for x, (a, b) in enumerate(pairs(A)):
        err = np.abs(got[:, x].astype(np.complex128) - ref_cross[:, x]).sum(axis=1)
        nrm = np.sqrt(np.abs(ref_autos[:, a]).sum(axis=1) * np.abs(ref_autos[:, b]).sum(axis=1))
        if np.any(nrm <= 0):
            assert not err[nrm <= 0].any()
        ok = nrm > 0
        if ok.any():
            worst = max(worst, float((err[ok] / (bound(k, k_avg) * nrm[ok])).max()))
    return worst


def auto_ratio(got, ref_autos, k, k_avg):
    """max over the auto rows of ||got - ref||_1 / (pfbspec_ref.bound ||ref||_1); got [n, A, M]."""
    err = np.abs(got.astype(np.float64) - ref_autos).sum(axis=2)
    nrm = np.abs(ref_autos).sum(axis=2)
    assert not err[nrm <= 0].any()
    ok = nrm > 0
    return float((err[ok] / (pfbspec_ref.bound(k, k_avg) * nrm[ok])).max()) if ok.any() else 0.0


# ---- the order of the sums and an f32 stand-in for the device -------------------------------------------------

def ordered_sums(terms, k, k_avg):
    """terms float32 [n * K, M] -> float32 [n, M], every row's K terms added in f32 in the order of DESIGN.md 4.15:
    slices of L = min(16, F) frames with F = 4096 / M; where K >= F slice s holds the frames r with
    (r mod F) // L == s, ascending, else the frames s L .. s L + L - 1; a slice sum starts from +0, and the slice
    sums are added in the order s = 0, 1, ..."""
    terms = np.asarray(terms, dtype=np.float32)
    M = terms.shape[1]
    assert M == 1 << k
    F = TILE_POINTS // M
    L = min(16, F)
    n = terms.shape[0] // k_avg
    r = np.arange(k_avg)
    slice_of = (r % F) // L if k_avg >= F else r // L
    out = np.empty((n, M), dtype=np.float32)
    for j in range(n):
        rows = terms[j * k_avg:(j + 1) * k_avg]
        total = None
        for s in range(int(slice_of.max()) + 1):
            acc = np.zeros(M, dtype=np.float32)
            for row in rows[slice_of == s]:
                acc = acc + row
            total = acc if total is None else total + acc
        out[j] = total
    return out


def products_f32(ya, yb):
    """complex64 [n, M] x 2 -> (re, im) float32 of Y_a conj(Y_b): every product and every sum rounded once."""
    ar, ai = ya.real.astype(np.float32), ya.imag.astype(np.float32)
    br, bi = yb.real.astype(np.float32), yb.imag.astype(np.float32)
    return (ar * br) + (ai * bi), (ai * br) - (ar * bi)


def sums_f32(ys, k, k_avg):
    """ys: A arrays complex64 [nframes, M] (a device's frames, or a stand-in's) -> (float32 [n, A, M], complex64
    [n, NX, M]): the definition's f32 arithmetic in the definition's order."""
    autos = np.stack([ordered_sums(products_f32(y, y)[0], k, k_avg) for y in ys], axis=1)
    cross = np.empty((autos.shape[0], len(pairs(len(ys))), autos.shape[2]), dtype=np.complex64)
    for x, (a, b) in enumerate(pairs(len(ys))):
        re, im = products_f32(ys[a], ys[b])
        cross[:, x].real = ordered_sums(re, k, k_avg)
        cross[:, x].imag = ordered_sums(im, k, k_avg)
    return autos, cross


def standin_frames(iq, k, taps, hop, nframes):
    """A stand-in for the device's frames: the exact branch sums rounded to f32, torch's f32 FFT."""
    import torch
    M = 1 << k
    xi = np.asarray(iq, dtype=np.uint8).reshape(-1, 2).astype(np.int64) - 128
    h = np.asarray(taps).astype(np.int64)
    vr = pfb_ref.branch_sums(xi[:, 0], k, h, hop, nframes).astype(np.float32)
    vi = pfb_ref.branch_sums(xi[:, 1], k, h, hop, nframes).astype(np.float32)
    y = torch.fft.fft(torch.complex(torch.from_numpy(vr), torch.from_numpy(vi)), dim=1).numpy()
    assert y.dtype == np.complex64 and y.shape == (nframes, M)
    return y


# ---- captures ---------------------------------------------------------------------------------------------------

def delay_case(hop_div):
    """M = 64, T = 8, the designed prototype, K = 256, one spectrum: x = clip(rint(30 N(0,1)) + 128) from
    default_rng(5), x_a = x[1:], x_b = x[:-1], so x_b[n] = x_a[n - 1]: capture b lags by one sample and V_01[c] has
    the phase +2 pi c / 64, c signed.  -> (k, taps, hop, K, [x_a, x_b])"""
    k, T, K = 6, 8, 256
    M = 1 << k
    D = M // hop_div
    n = samples_needed(M, T, D, K, 1) + 1
    x = np.clip(np.rint(30.0 * np.random.default_rng(5).standard_normal((n, 2))) + 128, 0, 255).astype(np.uint8)
    return k, pfbspec_ref.designed_taps(k, T), D, K, [np.ascontiguousarray(x[1:]), np.ascontiguousarray(x[:-1])]


def delay_figures(cross_row, auto_a, auto_b):
    """-> (the largest distance in radians of V_01[c]'s phase from 2 pi c_signed / M over the channels, the smallest
    coherence |V| / sqrt(S_a S_b)); rows unshifted."""
    M = cross_row.shape[0]
    c = np.arange(M)
    want = 2.0 * np.pi * np.where(c >= M // 2, c - M, c) / M
    v = np.asarray(cross_row, dtype=np.complex128)
    dev = np.angle(v * np.exp(-1j * want))
    coh = np.abs(v) / np.sqrt(np.asarray(auto_a, np.float64) * np.asarray(auto_b, np.float64))
    return float(np.abs(dev).max()), float(coh.min())


DELAYS = (0, 1, 3, 6)


def delayed_captures(A, n, seed, sigma=30.0, own=6.0):
    """A captures of n samples: copies of one Gaussian noise capture delayed by DELAYS[a] samples, each with
    independent noise of its own, as u8.  The pairs' delays are 1, 3, 6, 2, 5, 3: another phase slope for every pair
    but (0,2) and (2,3), whose rows differ by the captures' own noise."""
    rng = np.random.default_rng(seed)
    lead = max(DELAYS)
    common = sigma * (rng.standard_normal(n + lead) + 1j * rng.standard_normal(n + lead))
    out = []
    for a in range(A):
        z = common[lead - DELAYS[a]:lead - DELAYS[a] + n] + own * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        out.append(np.clip(np.rint(np.stack([z.real, z.imag], axis=1)) + 128, 0, 255).astype(np.uint8))
    return out
