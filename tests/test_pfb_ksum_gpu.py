"""GPU suite of the polyphase family's K-frame sums: the spectrometer, the cross-correlator and the beamformer's power
mode launched at a K of every class of tests/pfb_ksum_cases.py (every path of the kernels through (log2 M, K):
several spectra in a tile with one or several slices each, one spectrum over 1, 2 and 3 tile iterations with a last
iteration that is full, shorter than a slice, a whole number of slices or ragged across slices), at both hops.
At M = 16 every slice count 1 .. 8 of a spectrum that shares its tile is launched too.

Every sum is compared as uint32 with the documented order in numpy f32 -- pfbxc_ref.ordered_sums,
which tests/test_pfb_ksum_cpu.py pins to a second restatement -- of the f32 products of the channelizer's (the
beamformer: the voltage run's) own download of the same captures: no tolerance.  Beside that the derived bounds against
f64 (pfbspec_ref.bound, pfbxc_ref.bound, pfbbf_ref.power_bound) hold at every K.  Random bytes, random int16 taps,
T = 3 taps per branch (T does not enter the sums)."""
import functools

import numpy as np
import pytest

import pfb_ksum_cases as ksum
import pfb_ref
import pfbbf_ref
import pfbspec_ref
import pfbxc_ref
from test_pfbspec_gpu import worst_ratio

pytestmark = pytest.mark.gpu

T = 3
MULTI = (4, 6, 10)                                    # where the correlator also runs A = 2 and 4
BEAMS = ((2, 1), (3, 4))                              # (A, B)
DB_SCALE = 1e-9                                       # puts the rows of random bytes under random taps at 40 .. 90 dB
BIG = (4, ksum.MAX_K_AVG, 1, 2)                       # (log2 M, K, T, spectra) of the K = 65536 tests, hop M


def u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def u64(x):
    return np.ascontiguousarray(x).view(np.uint64)


@functools.lru_cache(maxsize=None)
def the_taps(k, taps_per_branch=T):
    return pfb_ref.random_taps(k, taps_per_branch, seed=100 * k + taps_per_branch)


@functools.lru_cache(maxsize=None)
def capture(k, a, nframes, taps_per_branch=T):
    """Capture a of log2 M = k, long enough for nframes frames at hop M (at hop M / 2 a prefix of it is read)."""
    M = 1 << k
    return pfb_ref.random_iq(pfb_ref.samples_needed(M, taps_per_branch, M, nframes), seed=1000 * a + k + 50)


@functools.lru_cache(maxsize=None)
def frames64(k, D, a, nframes, taps_per_branch=T):
    """The f64 restatement's frames of capture a, first_frame_index = 0, computed once for all three libraries' tests;
    nobody writes to it.  A shorter run is a prefix."""
    y = pfb_ref.pfb_ref(capture(k, a, nframes, taps_per_branch), k, the_taps(k, taps_per_branch), D, 0, nframes)
    y.setflags(write=False)
    return y


class Rig:
    """The captures of one log2 M on the device, uploaded once, the channelizer's and the spectrometer's plans and a
    buffer for the longest run of either."""

    def __init__(self, engine, built, k, ncaptures, nframes, taps_per_branch=T):
        self.eng, self.k, self.M, self.nframes = engine, k, 1 << k, nframes
        self.taps = the_taps(k, taps_per_branch)
        self.iqs = [capture(k, a, nframes, taps_per_branch) for a in range(ncaptures)]
        self.d_iqs = [engine.upload(x) for x in self.iqs]
        self.pfb_plan = built.PfbPlan.open(engine, k, self.taps)
        self.spec_plan = built.PfbSpecPlan.open(engine, k, self.taps)
        self.d_tmp = engine.alloc(nframes * self.M * 8)
        self.owned = [self.d_tmp] + self.d_iqs
        self.plans = [self.pfb_plan, self.spec_plan]

    def alloc(self, nbytes):
        self.owned.append(self.eng.alloc(nbytes))
        return self.owned[-1]

    def upload(self, x):
        self.owned.append(self.eng.upload(x))
        return self.owned[-1]

    def frames(self, a, n, D):
        """rtlws_pfb_run's time-major samples of capture a, first_frame_index = 0 -> complex64 [n, M]"""
        assert n <= self.nframes
        self.pfb_plan.run(self.d_iqs[a], n, self.d_tmp, hop=D, layout="time")
        self.eng.sync()
        return self.eng.download(self.d_tmp, np.complex64, (n, self.M))

    def spec(self, d_iq, K, n, D, shifted=False, output="power", scale=1.0):
        """rtlws_pfbspec_run's f32 rows of a capture on the device -> float32 [n, M]"""
        assert n * K <= self.nframes
        self.spec_plan.run(d_iq, n, K, self.d_tmp, hop=D, output=output, shifted=shifted, scale=scale)
        self.eng.sync()
        return self.eng.download(self.d_tmp, np.float32, (n, self.M))

    def close(self):
        for p in self.plans:
            p.close()
        for b in self.owned:
            b.free()


def runs(k, grid):
    """-> [(K, spectra)] of the matrix, spectra = 2 per + 1 with per from the library's own grid call"""
    return [(K, ksum.spectra(k, K, grid)) for K in ksum.cases(k)]


def spec_sums_f32(y, k, K):
    """complex64 [n K, M] -> float32 [n, M]: fl(fl(re re) + fl(im im)) summed in the documented order"""
    return pfbxc_ref.ordered_sums(pfbxc_ref.products_f32(y, y)[0], k, K)


def check_spectrometer(rig, k, D, todo, taps_per_branch=T):
    """The checks of one hop -> the worst ratio to pfbspec_ref.bound"""
    M = rig.M
    longest = max(K * n for K, n in todo)
    y = rig.frames(0, longest, D)
    ref64 = frames64(k, D, 0, rig.nframes, taps_per_branch)
    d_mid = rig.upload(np.full((pfb_ref.samples_needed(M, taps_per_branch, D, longest), 2), 128, dtype=np.uint8))
    worst = 0.0
    for K, n in todo:
        want = spec_sums_f32(y[:n * K], k, K)
        assert want.shape == (n, M) and np.all(want > 0)
        got = rig.spec(rig.d_iqs[0], K, n, D)
        assert np.array_equal(u32(got), u32(want)), (k, K, D, first_difference(got, want))
        shifted = rig.spec(rig.d_iqs[0], K, n, D, shifted=True)
        assert np.array_equal(u32(shifted), u32(np.fft.fftshift(want, axes=1))), (k, K, D, "shifted")
        r = worst_ratio(got, pfbspec_ref.k_sums(ref64[:n * K], K), k, K)       # pfbspec_ref.pfbspec_ref's rows
        worst = max(worst, r)
        assert r <= 1.0, (k, K, D, r)
        assert not u32(rig.spec(d_mid, K, n, D)).any(), (k, K, D, "all-128")
    return worst


def first_difference(got, want):
    """(spectrum, bin) of the first word that differs, for the message of a failed comparison"""
    bad = np.argwhere(u32(got) != u32(want))
    return tuple(int(v) for v in bad[0]) if bad.size else None


@pytest.mark.parametrize("k", ksum.LOG2_MS)
def test_spectrometer_at_every_sum_geometry(engine, built, k):
    """Raw sums as uint32 = the ordered f32 sums of rtlws_pfb_run's time-major download of the same capture, unshifted
    and shifted; under the f64 bound; all-128 input gives +0 in every word.  Every K of the matrix, both hops."""
    M = 1 << k
    todo = runs(k, lambda k, K: built.pfbspec_grid(k, T, M, K, 1)[4])
    rig = Rig(engine, built, k, 1, max(K * n for K, n in todo))
    try:
        worst = max(check_spectrometer(rig, k, D, todo) for D in (M, M // 2))
    finally:
        rig.close()
    print("pfbspec, M = %d: worst ||got - ref||_1 / bound = %.4f (K = %s)" % (M, worst, [K for K, _ in todo]))


def check_correlator(rig, k, D, plans, todo, d_auto, d_cross, taps_per_branch=T):
    """The checks of one hop for every (A, plan) of plans -> (the worst auto ratio, the worst cross ratio).  Every auto
    and every pair is summed once, for the largest A, and shared: the pairs of A inputs are rows of the largest A's."""
    M, most = rig.M, max(A for A, _ in plans)
    longest = max(K * n for K, n in todo)
    ys = [rig.frames(a, longest, D) for a in range(most)]
    refs = [frames64(k, D, a, rig.nframes, taps_per_branch) for a in range(most)]
    worst_a = worst_c = 0.0
    for K, n in todo:
        all_a, all_c = pfbxc_ref.sums_f32([y[:n * K] for y in ys], k, K)
        ref_all_a, ref_all_c = pfbxc_ref.xc_sums([y[:n * K] for y in refs], K)
        spec = [rig.spec(rig.d_iqs[a], K, n, D) for a in range(most)]
        for A, plan in plans:
            rows = [pfbxc_ref.pairs(most).index(p) for p in pfbxc_ref.pairs(A)]
            want_a, want_c, ref_a, ref_c = all_a[:, :A], all_c[:, rows], ref_all_a[:, :A], ref_all_c[:, rows]
            plan.run(rig.d_iqs[:A], n, K, d_auto, d_cross, hop=D)
            rig.eng.sync()
            autos = rig.eng.download(d_auto, np.float32, (n, A, M))
            cross = rig.eng.download(d_cross, np.complex64, (n, len(rows), M))
            assert np.array_equal(u32(autos), u32(want_a)), (k, K, D, A, first_difference(autos, want_a))
            assert np.array_equal(u64(cross), u64(want_c)), (k, K, D, A, first_difference(cross, want_c))
            for a in range(A):
                assert np.array_equal(u32(autos[:, a]), u32(spec[a])), (k, K, D, A, a)
            ra, rc = pfbxc_ref.auto_ratio(autos, ref_a, k, K), pfbxc_ref.cross_ratio(cross, ref_a, ref_c, k, K)
            worst_a, worst_c = max(worst_a, ra), max(worst_c, rc)
            assert ra <= 1.0 and rc <= 1.0, (k, K, D, A, ra, rc)
    return worst_a, worst_c


@pytest.mark.parametrize("k", ksum.LOG2_MS)
def test_correlator_at_every_sum_geometry(engine, built, k):
    """Autos as uint32 and crosses as uint64 = pfbxc_ref.sums_f32 of rtlws_pfb_run's frames of each capture; the auto
    rows are rtlws_pfbspec_run's; under the f64 bounds.  A = 3 at every log2 M, A = 2 and 4 at 4, 6 and 10."""
    M = 1 << k
    inputs = (2, 3, 4) if k in MULTI else (3,)
    todo = runs(k, lambda k, K: built.pfbxc_grid(k, T, M, K, 3, 1)[4])
    for A in inputs:
        assert runs(k, lambda k, K: built.pfbxc_grid(k, T, M // 2, K, A, 1)[4]) == todo
    nmax = max(n for _, n in todo)
    rig = Rig(engine, built, k, max(inputs), max(K * n for K, n in todo))
    worst_a = worst_c = 0.0
    try:
        d_auto = rig.alloc(nmax * max(inputs) * M * 4)
        d_cross = rig.alloc(nmax * 6 * M * 8)
        plans = []
        for A in inputs:
            plans.append((A, built.PfbXcPlan.open(engine, k, rig.taps, A)))
            rig.plans.append(plans[-1][1])
        for D in (M, M // 2):
            ra, rc = check_correlator(rig, k, D, plans, todo, d_auto, d_cross)
            worst_a, worst_c = max(worst_a, ra), max(worst_c, rc)
    finally:
        rig.close()
    print("pfbxc, M = %d, A = %s: worst cross ratio to the bound %.4f, worst auto ratio %.4f (K = %s)"
          % (M, list(inputs), worst_c, worst_a, [K for K, _ in todo]))


def check_beamformer(rig, k, D, A, B, todo, d_out, plan, taps_per_branch=T):
    """The checks of one (hop, A, B) -> the worst ratio to pfbbf_ref.power_bound"""
    M = rig.M
    longest = max(K * n for K, n in todo)
    ptrs = rig.d_iqs[:A]

    def power(d_w, K, n):
        plan.power(ptrs, d_w, n, K, d_out, hop=D)
        rig.eng.sync()
        return rig.eng.download(d_out, np.float32, (n, B, M))

    # random weights: the rows are the ordered sums of the voltage run's own download, and lie under the f64 bound
    W = pfbbf_ref.random_weights(B, A, M, seed=7 * k + A)
    d_w = rig.upload(W)
    plan.run(ptrs, d_w, longest, d_out, hop=D, first_frame_index=7 if D != M else 0, layout="time")
    rig.eng.sync()
    z = rig.eng.download(d_out, np.complex64, (B, longest, M))
    ys = [frames64(k, D, a, rig.nframes, taps_per_branch)[:longest] * pfbbf_ref.signs(M, D, 0, longest) for a in range(A)]
    zref = pfbbf_ref.beams(ys, W)
    worst = 0.0
    for K, n in todo:
        want = pfbbf_ref.power_f32(z[:, :n * K], k, K)
        assert want.shape == (n, B, M) and np.all(want > 0)
        got = power(d_w, K, n)
        assert np.array_equal(u32(got), u32(want)), (k, K, D, A, B, first_difference(got, want))
        r = pfbbf_ref.power_ratio(got, pfbbf_ref.k_sums(zref[:, :n * K], K), [y[:n * K] for y in ys], W, k, K)
        worst = max(worst, r)
        assert r <= 1.0, (k, K, D, A, B, r)
    # one-hot weights: beam b passes capture (b + 1) mod A alone, and its rows are the spectrometer's
    which = [(b + 1) % A for b in range(B)]
    d_hot = rig.upload(pfbbf_ref.one_hot(B, A, M, which))
    for K, n in todo:
        got = power(d_hot, K, n)
        for a in sorted(set(which)):
            want = rig.spec(rig.d_iqs[a], K, n, D)
            for b in range(B):
                if which[b] == a:
                    assert np.array_equal(u32(got[:, b]), u32(want)), (k, K, D, A, B, b)
    return worst


@pytest.mark.parametrize("k", ksum.LOG2_MS)
def test_beamformer_power_at_every_sum_geometry(engine, built, k):
    """Power rows as uint32 = pfbbf_ref.power_f32 of the voltage run's own download; with one-hot weights they are
    rtlws_pfbspec_run's rows of the passed capture; under the f64 bound with random weights.  (A, B) = (2, 1) and
    (3, 4): the K >= F and the K < F instantiation of both."""
    M = 1 << k
    todo = runs(k, lambda k, K: built.pfbbf_grid(k, T, M, K, 1)[4])
    longest = max(K * n for K, n in todo)
    rig = Rig(engine, built, k, max(A for A, _ in BEAMS), longest)
    worst = 0.0
    try:
        d_out = rig.alloc(max(B for _, B in BEAMS) * longest * M * 8)
        for A, B in BEAMS:
            plan = built.PfbBfPlan.open(engine, k, rig.taps, A, B)
            rig.plans.append(plan)
            for D in (M, M // 2):
                worst = max(worst, check_beamformer(rig, k, D, A, B, todo, d_out, plan))
    finally:
        rig.close()
    print("pfbbf, M = %d, (A, B) = %s: worst power ratio to the bound %.4f (K = %s)" % (M, list(BEAMS), worst, [K for K, _ in todo]))


@pytest.mark.parametrize("k", ksum.LOG2_MS)
def test_spectrometer_mean_db_at_the_new_geometries(engine, built, k):
    """RTLWS_OUT_MEAN_DB at K = 2 F (two full tile iterations) and, where it exists, at a K with several spectra per
    tile and several slices per spectrum: within 2e-4 dB (rtlws_hip.h's figure for this output kind, test_db_and_bytes'
    criterion) of 10 log10(S lin) in f64 of the device's own raw sums, unshifted and shifted."""
    M, F = 1 << k, ksum.tile_frames(k)
    ks = [K for K in (ksum.several_spectra_several_slices(k), 2 * F) if K is not None]
    assert len(ks) == (2 if k <= 6 else 1) and set(ks) <= set(ksum.cases(k))
    todo = [(K, ksum.spectra(k, K, lambda k, K: built.pfbspec_grid(k, T, M, K, 1)[4])) for K in ks]
    rig = Rig(engine, built, k, 1, max(K * n for K, n in todo))
    worst = 0.0
    try:
        for D in (M, M // 2):
            for K, n in todo:
                sums = rig.spec(rig.d_iqs[0], K, n, D)
                for shifted in (False, True):
                    want = pfbspec_ref.db(np.fft.fftshift(sums, axes=1) if shifted else sums, DB_SCALE, K)
                    assert 20.0 <= want.min() and want.max() <= 120.0
                    got = rig.spec(rig.d_iqs[0], K, n, D, shifted=shifted, output="db", scale=DB_SCALE)
                    err = float(np.abs(got.astype(np.float64) - want).max())
                    worst = max(worst, err)
                    assert err <= 2e-4, (k, K, D, shifted, err)
    finally:
        rig.close()
    print("pfbspec, M = %d: mean dB within %.2e dB of the f64 value of the device's sums (K = %s)" % (M, worst, ks))


# ---- K = 65536, the documented maximum: log2 M = 4, hop M, T = 1, two spectra -----------------------------------------

def big_rig(engine, built, ncaptures):
    k, K, taps_per_branch, n = BIG
    return Rig(engine, built, k, ncaptures, K * n, taps_per_branch)


def test_spectrometer_at_the_largest_k(engine, built):
    k, K, taps_per_branch, n = BIG
    assert built.pfbspec_supported(k, taps_per_branch, 1 << k, K) == 1 and built.pfbspec_supported(k, taps_per_branch, 1 << k, K + 1) == 0
    rig = big_rig(engine, built, 1)
    try:
        worst = check_spectrometer(rig, k, 1 << k, [(K, n)], taps_per_branch)
    finally:
        rig.close()
    print("pfbspec, M = %d, K = %d: ||got - ref||_1 / bound = %.2e" % (1 << k, K, worst))


def test_correlator_at_the_largest_k(engine, built):
    k, K, taps_per_branch, n = BIG
    M, A = 1 << k, 2
    rig = big_rig(engine, built, A)
    try:
        plan = built.PfbXcPlan.open(engine, k, rig.taps, A)
        rig.plans.append(plan)
        worst = check_correlator(rig, k, M, [(A, plan)], [(K, n)], rig.alloc(n * A * M * 4), rig.alloc(n * M * 8), taps_per_branch)
    finally:
        rig.close()
    print("pfbxc, M = %d, K = %d: auto ratio to the bound %.2e, cross ratio %.2e" % ((M, K) + worst))


def test_beamformer_power_at_the_largest_k(engine, built):
    k, K, taps_per_branch, n = BIG
    M, (A, B) = 1 << k, BEAMS[0]
    rig = big_rig(engine, built, A)
    try:
        plan = built.PfbBfPlan.open(engine, k, rig.taps, A, B)
        rig.plans.append(plan)
        worst = check_beamformer(rig, k, M, A, B, [(K, n)], rig.alloc(B * K * n * M * 8), plan, taps_per_branch)
    finally:
        rig.close()
    print("pfbbf, M = %d, K = %d: power ratio to the bound %.2e" % (M, K, worst))
