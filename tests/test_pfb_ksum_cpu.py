"""CPU suite of the polyphase family's K-frame sums (csrc/pfb_bank.h): the case list of
tests/pfb_ksum_cases.py reaches every class of (log2 M, K) that exists; the index arithmetic of the kernels' "several
spectra in one tile" path restated and checked exhaustively; the numpy yardstick of the order (pfbxc_ref.ordered_sums)
pinned to a second restatement written as the kernels loop; the yardstick alone inside the derived bounds at the K
that tests/test_pfb_ksum_gpu.py adds.  No GPU is used."""
import numpy as np
import pytest

import pfb_ksum_cases as ksum
import pfb_ref
import pfbbf_ref
import pfbspec_ref
import pfbxc_ref

T = 3


def u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def test_the_cases_reach_every_class():
    """All 7 x 65536 (log2 M, K) classified: cases(k) holds a K of every class that occurs, the old K lists do not, and
    the K they lack are the ones written down here."""
    want_new = {4: [16, 17, 32, 48, 144, 272, 273, 512, 528, 529, 768], 5: [16, 17, 32, 48, 80, 144, 145, 256, 272, 273, 384],
                6: [16, 17, 32, 48, 80, 81, 128, 144, 145, 192], 7: [16, 48, 49, 64, 80, 81, 96], 8: [32, 48], 9: [16, 24],
                10: [8, 12, 16]}
    for k in ksum.LOG2_MS:
        F = ksum.tile_frames(k)
        every = {ksum.classify(k, K) for K in range(1, ksum.MAX_K_AVG + 1)}
        assert every == set(ksum.smallest_of_each_class(k))
        got = {ksum.classify(k, K) for K in ksum.cases(k)}
        assert got == every, (k, every - got)
        old = {ksum.classify(k, K) for K in ksum.old_k_list(k)}
        assert old < every, k
        more = ksum.SLICE_COUNTS.get(k, ())
        assert [K for K in ksum.new_k_list(k) if K not in more] == want_new[k], k      # derived there, written down here
        assert set(more) <= set(ksum.cases(k)) and not set(more) & set(want_new[k])
        assert set(ksum.old_k_list(k)) <= set(ksum.cases(k)) and max(ksum.cases(k)) == max(3 * F, 2 * F + 3, *ksum.EXTRAS.get(k, ()))
        assert ksum.classify(k, ksum.MAX_K_AVG) in got
        # the classes by name
        names = {K: ksum.classify(k, K) for K in ksum.cases(k)}
        for K in (2 * F, 3 * F):
            assert names[K][2] == "last iteration full" and names[K][1] != "1 iteration"
        if F > 16:
            assert names[F + 16][2] == "last iteration whole slices" and names[F + 17][2] == "last iteration several slices, ragged"
            assert names[16][:4] == ("K < F", "G > 1", "one slice", "whole slices")
        K = ksum.several_spectra_several_slices(k)
        assert (K is not None) == (k <= 6)
        if K is not None:
            # 16 < K <= F / 2: 112, 48 and 16 values of K, of which 105, 45 and 15 end inside a slice
            assert K == 17 and names[17][3] == "ragged slice"
            assert sum(1 for q in range(1, F) if ksum.classify(k, q)[:3] == names[17][:3]) == F // 2 - 16
            assert sum(1 for q in range(1, F) if ksum.classify(k, q)[:4] == names[17][:4]) == {4: 105, 5: 45, 6: 15}[k]
    assert ksum.classify(4, 144) == ("K < F", "G = 1", "several slices", "whole slices", "frames of the tile unused")


def test_geometry_is_the_librarys(built):
    """geometry() against the three libraries' own *_grid calls at every K of the matrix, and spectra() = 2 per + 1."""
    for k in ksum.LOG2_MS:
        M = 1 << k
        for K in ksum.cases(k) + [ksum.MAX_K_AVG]:
            per = ksum.geometry(k, K)[1]
            n = ksum.spectra(k, K)
            assert n == 2 * per + 1
            for hop in (M, M // 2):
                assert built.pfbspec_grid(k, T, hop, K, n)[::4] == (0, per)
                assert built.pfbxc_grid(k, T, hop, K, 3, n)[::4] == (0, per)
                assert built.pfbbf_grid(k, T, hop, K, n)[::4] == (0, per)
                assert built.pfbspec_grid(k, T, hop, K, n)[1] == 3


def test_the_reciprocal_multiply_is_the_quotient():
    """pfbspec.hip's item w = (g nsl + s) M + c is split by g = (gs * inv) >> 16 with inv = 65536 / nsl + 1: equal to
    gs // nsl for every (log2 M, K < F, gs < G nsl), inside 32 bits, and the items fit the tile."""
    seen = set()
    for k in ksum.LOG2_MS:
        M, F, L = 1 << k, ksum.tile_frames(k), ksum.slice_frames(k)
        for K in range(1, F):
            whole, G, nit, nsl, last = ksum.geometry(k, K)
            assert not whole and nit == 1 and G == F // K and nsl == (K + L - 1) // L and 1 <= nsl <= 16
            assert G * nsl * M <= ksum.TILE_POINTS, (k, K)
            assert G * K <= F
            inv = 65536 // nsl + 1
            gs = np.arange(G * nsl, dtype=np.int64)
            assert gs.size <= 256 and int(gs[-1]) * inv < 2 ** 31
            g = (gs * inv) >> 16
            assert np.array_equal(g, gs // nsl), (k, K)
            s = gs - g * nsl
            assert np.all((0 <= s) & (s < nsl)) and np.all(g * K + s * L + np.minimum(L, K - s * L) <= F)
            seen.add((nsl, G > 1))
    assert {(n, True) for n in range(2, 9)} <= seen                    # nsl = 2 .. 8 with several spectra: M = 16
    launched = {ksum.geometry(4, K)[3] for K in ksum.cases(4) if K < 256 and ksum.geometry(4, K)[1] > 1}
    assert launched == set(range(1, 9))                               # and the GPU matrix launches every one of them


def kernel_order_sums(terms, k, K):
    """The sums as the kernels loop (pfbspec.hip steps 5 and 6; pfbxc.hip and pfbbf.hip restate them), one f32
    operation at a time: K >= F a running sum per slice over the tile iterations, frames of an iteration in order,
    frames at or behind K left out, then the slices added in the order s = 0, 1, ..; K < F every slice from +0 in frame
    order, the first slice taken, the others added.  Written without a look at pfbxc_ref.ordered_sums."""
    terms = np.asarray(terms, dtype=np.float32)
    M = 1 << k
    F = 4096 // M
    SLICE = F if F < 16 else 16
    n = terms.shape[0] // K
    out = np.empty((n, M), dtype=np.float32)
    for j in range(n):
        P = terms[j * K:(j + 1) * K]
        if K >= F:
            nit, nsl = (K + F - 1) // F, F // SLICE
            acc = [np.zeros(M, np.float32) for _ in range(nsl)]
            for it in range(nit):
                for s in range(nsl):
                    nl = min(SLICE, K - (it * F + s * SLICE))
                    for l in range(nl):
                        acc[s] = acc[s] + P[it * F + s * SLICE + l]
            t = acc[0]
            for s in range(1, nsl):
                t = t + acc[s]
        else:
            nsl = (K + SLICE - 1) // SLICE
            t = None
            for s in range(nsl):
                nl = min(SLICE, K - s * SLICE)
                sl = np.zeros(M, np.float32)
                for l in range(nl):
                    sl = sl + P[s * SLICE + l]
                t = sl if s == 0 else t + sl
        assert t.dtype == np.float32
        out[j] = t
    return out


def _terms(k, K, n, seed):
    """-> (integer-valued terms whose every partial sum is exact in f32: a sum in any order, but of other frames, shows;
    terms that cancel, of magnitudes 2^-12 .. 2^12: another order of the same frames shows)"""
    rng = np.random.default_rng(seed)
    M = 1 << k
    whole = rng.integers(-63, 64, size=(n * K, M)).astype(np.float32)
    mixed = (rng.standard_normal((n * K, M)) * 2.0 ** rng.integers(-12, 13, size=(n * K, M))).astype(np.float32)
    return whole, mixed


def _order_is_not_plain(k, K):
    """Several slices of which the second or a later one holds two frames or more: with one frame behind a single full
    slice (K = L + 1 < F) the documented order is the plain running sum."""
    L = ksum.slice_frames(k)
    return ksum.geometry(k, K)[3] > 1 and K > L and not (K < ksum.tile_frames(k) and K == L + 1)


@pytest.mark.parametrize("k", ksum.LOG2_MS)
def test_ordered_sums_is_the_kernels_loop(k):
    """pfbxc_ref.ordered_sums against kernel_order_sums as uint32 at every K of the matrix, two spectra each; where a
    spectrum has several slices a plain running sum over the K frames gives other bits on the cancelling terms, so the
    comparison tells the orders apart."""
    M = 1 << k
    told_apart = 0
    for K in ksum.cases(k):
        whole, mixed = _terms(k, K, 2, seed=100 * k + K)
        for t in (whole, mixed):
            want = kernel_order_sums(t, k, K)
            got = pfbxc_ref.ordered_sums(t, k, K)
            assert got.dtype == np.float32 and got.shape == (2, M)
            assert np.array_equal(u32(got), u32(want)), (k, K)
        exact = whole.astype(np.float64).reshape(2, K, M).sum(axis=1)
        assert np.array_equal(pfbxc_ref.ordered_sums(whole, k, K).astype(np.float64), exact), (k, K)
        if _order_is_not_plain(k, K):
            plain = np.zeros((2, M), np.float32)
            for r in range(K):
                plain = plain + mixed.reshape(2, K, M)[:, r]
            told_apart += int(not np.array_equal(u32(plain), u32(pfbxc_ref.ordered_sums(mixed, k, K))))
    several = [K for K in ksum.cases(k) if _order_is_not_plain(k, K)]
    assert told_apart == len(several), (k, told_apart, several)


def _ragged(k):
    """The largest K of the matrix, and the most ragged: of those whose last tile iteration (K < F: whose K frames) ends
    inside a slice, the one where it holds the most slices, the largest such K."""
    L = ksum.slice_frames(k)
    tail = {K: ksum.geometry(k, K)[4] for K in ksum.cases(k)}
    rag = max((K for K in tail if tail[K] % L), key=lambda K: (-(-tail[K] // L), K))
    return sorted({max(tail), rag})


@pytest.mark.parametrize("k", ksum.LOG2_MS)
def test_the_reference_alone_stays_inside_the_bounds_at_the_new_k(k):
    """pfbxc_ref.standin_frames (the exact branch sums, torch's f32 FFT) summed in f32 in the definition's order against
    the f64 restatements, under the derived bounds pfbspec_ref.bound, pfbxc_ref.bound and pfbbf_ref.power_bound: every
    K the matrix adds at hop M, the largest and the most ragged at hop M / 2 too.  Three captures, two beams."""
    M = 1 << k
    n, A, B = 2, 3, 2
    taps = pfb_ref.random_taps(k, T, seed=100 * k + T)
    W = pfbbf_ref.random_weights(B, A, M, seed=k)
    worst = [0.0, 0.0, 0.0]
    both = _ragged(k)
    assert max(ksum.cases(k)) in both and len(both) == 2
    for D in (M, M // 2):
        ks = sorted(set(ksum.new_k_list(k)) | set(both)) if D == M else both
        longest = n * max(ks)
        iqs = pfbbf_ref.random_captures(A, pfb_ref.samples_needed(M, T, D, longest), seed=k + T + D)
        ys64 = pfbxc_ref.frames_of(iqs, k, taps, D, longest)
        ys32 = [pfbxc_ref.standin_frames(x, k, taps, D, longest) for x in iqs]
        z64, z32 = pfbbf_ref.beams(ys64, W), pfbbf_ref.beams_f32(ys32, W)
        for K in ks:
            ref_a, ref_c = pfbxc_ref.xc_sums([y[:n * K] for y in ys64], K)
            got_a, got_c = pfbxc_ref.sums_f32([y[:n * K] for y in ys32], k, K)
            rs = max(float((np.abs(got_a[:, a].astype(np.float64) - ref_a[:, a]).sum(axis=1)
                            / (pfbspec_ref.bound(k, K) * ref_a[:, a].sum(axis=1))).max()) for a in range(A))
            assert np.array_equal(ref_a[:, 0], pfbspec_ref.k_sums(ys64[0][:n * K], K))
            rc = pfbxc_ref.cross_ratio(got_c, ref_a, ref_c, k, K)
            assert pfbxc_ref.auto_ratio(got_a, ref_a, k, K) == rs
            rp = pfbbf_ref.power_ratio(pfbbf_ref.power_f32(z32[:, :n * K], k, K), pfbbf_ref.k_sums(z64[:, :n * K], K),
                                       [y[:n * K] for y in ys64], W, k, K)
            worst = [max(w, r) for w, r in zip(worst, (rs, rc, rp))]
            assert rs <= 1.0 and rc <= 1.0 and rp <= 1.0, (D, K, rs, rc, rp)
    print("M = %d: stand-in's worst ratios to the bounds at the new K: spectrometer %.4f, cross %.4f, beam power %.4f" % (M, *worst))
