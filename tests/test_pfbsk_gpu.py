"""GPU suite of include/rtlws_pfbsk.h (librtlws_pfbsk.so), the spectrometer with spectral-kurtosis excision.

The two sums of a sub-integration are held to the bit: S1 to rtlws_pfbspec_run's rows of the short spectra, S2 to
pfbxc_ref.ordered_sums of fl(p p) formed in numpy f32 from rtlws_pfb_run's own download of the same capture.  The
decision, the clean sum and the counts are held to the bit to their restatement in numpy f32 (tests/pfbsk_ref.py) on the
device's own S1 and S2 rows.  Against the f64 definition stand the semantic case (flags away from the bounds, the
derived bound of the clean row) and the dB rows.  The walk of a row's L sub-integrations through its tiles is held to
the same bits at every step geometry of tests/pfbsk_walk_cases.py.  Random bytes and random int16 taps unless said
otherwise."""
import ctypes as C
import math

import numpy as np
import pytest

import pfb_ksum_cases as ksum
import pfb_ref
import pfbsk_ref
import pfbsk_walk_cases as walks
import pfbspec_ref
import pfbxc_ref
from test_pfb_ksum_gpu import Rig, first_difference, u32

pytestmark = pytest.mark.gpu

T, NSUB = 3, 3                                       # of the matrix
SK = (pfbsk_ref.SK_LO, pfbsk_ref.SK_HI)
OPEN = pfbsk_ref.OPEN


def sk_bounds(built, K):
    """The ratio bounds of SK: the library's own where it forms them (K >= 2), its formula at K = 1 (1, 1)."""
    got = built.pfbsk_bounds(K, *SK) if K >= 2 else tuple(float(x) for x in pfbsk_ref.bounds(K, *SK))
    assert tuple(np.float32(x) for x in got) == pfbsk_ref.bounds(K, *SK)
    return got


class SkRig(Rig):
    """tests/test_pfb_ksum_gpu.py's rig (capture 0 on the device, the channelizer's and the spectrometer's plans) with
    this library's plan and buffers for nrows clean rows and nsubs sub-integration rows."""

    def __init__(self, engine, built, k, nframes, nrows, nsubs, taps_per_branch=T):
        super().__init__(engine, built, k, 1, nframes, taps_per_branch)
        self.plan = built.PfbSkPlan.open(engine, k, self.taps)
        self.plans.append(self.plan)
        self.scale = built.pfbsk_power_scale(k, self.taps)
        assert self.scale == pfbsk_ref.power_scale(self.taps)
        self.nrows, self.nsubs = nrows, nsubs
        self.d_clean, self.d_kept = self.alloc(nrows * self.M * 4), self.alloc(nrows * self.M * 4)
        self.d_s1, self.d_s2 = self.alloc(nsubs * self.M * 4), self.alloc(nsubs * self.M * 4)

    def run(self, d_iq, K, L, n, D, bounds=OPEN, shifted=False, output="power", scale=1.0):
        """-> (clean rows [n, M], N uint32 [n, M], S1 and S2 float32 [n L, M])"""
        assert n <= self.nrows and n * L <= self.nsubs
        self.plan.run(d_iq, n, K, L, self.scale, self.d_clean, bounds[0], bounds[1], self.d_kept, self.d_s1, self.d_s2, hop=D,
                      output=output, shifted=shifted, scale=scale)
        self.eng.sync()
        dtype = np.uint8 if output == "payload" else np.float32
        return (self.eng.download(self.d_clean, dtype, (n, self.M)), self.eng.download(self.d_kept, np.uint32, (n, self.M)),
                self.eng.download(self.d_s1, np.float32, (n * L, self.M)), self.eng.download(self.d_s2, np.float32, (n * L, self.M)))


def scaled_squares_f32(y, scale):
    """complex64 [n, M] -> float32: fl(p p), p = fl(P scale), P = fl(fl(re re) + fl(im im))"""
    p = pfbxc_ref.products_f32(y, y)[0] * np.float32(scale)
    assert p.dtype == np.float32
    return p * p


def check_sums_and_decisions(rig, built, k, K, L, n, D, y, d_mid):
    """The bit checks of one (K, L, n rows, hop) -> (flagged, kept) counts under the SK bounds.  y: rtlws_pfb_run's
    frames of the capture, at least n L K of them."""
    M, nq = rig.M, n * L
    d_iq = rig.d_iqs[0]
    sk = sk_bounds(built, K)
    # the raw sums
    clean, kept, s1, s2 = rig.run(d_iq, K, L, n, D)
    want1 = rig.spec(d_iq, K, nq, D)
    assert np.array_equal(u32(s1), u32(want1)), (k, K, L, D, "S1", first_difference(s1, want1))
    want2 = pfbxc_ref.ordered_sums(scaled_squares_f32(y[:nq * K], rig.scale), k, K)
    assert np.array_equal(u32(s2), u32(want2)), (k, K, L, D, "S2", first_difference(s2, want2))
    assert np.all(s1 > 0) and np.all(s2 > 0) and np.all(np.isfinite(s2))
    # open bounds: nothing is flagged, C is the sequential f32 sum of the device's S1 rows
    none = np.zeros(s1.shape, dtype=bool)
    assert not pfbsk_ref.flagged_f32(s1, s2, K, rig.scale, *OPEN).any()
    assert np.all(kept == L), (k, K, L, D)
    want_c, _ = pfbsk_ref.clean_rows_f32(s1, none, L)
    assert np.array_equal(u32(clean), u32(want_c)), (k, K, L, D, "open", first_difference(clean, want_c))
    # the SK bounds: the decision and the sum restated in numpy f32 on the device's own rows
    clean, kept, s1b, s2b = rig.run(d_iq, K, L, n, D, sk)
    assert np.array_equal(u32(s1b), u32(s1)) and np.array_equal(u32(s2b), u32(s2))
    flags = pfbsk_ref.flagged_f32(s1, s2, K, rig.scale, *sk)
    want_c, want_n = pfbsk_ref.clean_rows_f32(s1, flags, L)
    assert np.array_equal(kept, want_n), (k, K, L, D, "N", first_difference(kept, want_n))
    assert np.array_equal(u32(clean), u32(want_c)), (k, K, L, D, "C", first_difference(clean, want_c))
    # shifted rows are the fftshift of unshifted ones, all four outputs
    for got, want in zip(rig.run(d_iq, K, L, n, D, sk, shifted=True), (clean, kept, s1, s2)):
        assert np.array_equal(u32(got), u32(np.fft.fftshift(want, axes=1))), (k, K, L, D, "shifted")
    # all-128 input: +0 in every word of C, S1 and S2, and everything kept
    clean, kept, s1, s2 = rig.run(d_mid, K, L, n, D, sk)
    assert not u32(clean).any() and not u32(s1).any() and not u32(s2).any() and np.all(kept == L), (k, K, L, D, "all-128")
    return int(flags.sum()), int((~flags).sum())


@pytest.mark.parametrize("k", ksum.LOG2_MS)
def test_every_sum_geometry_to_the_bit(engine, built, k):
    """Every K of tests/pfb_ksum_cases.py, both hops, T = 3, L = 3, 2 per + 1 rows with per from rtlws_pfbsk_grid."""
    M = 1 << k
    todo = []
    for K in ksum.cases(k):
        rc, blocks, _, _, per = built.pfbsk_grid(k, T, M, K, NSUB, 1)
        assert rc == 0 and per >= 1 and blocks == 1
        todo.append((K, 2 * per + 1))
    longest = max(K * n * NSUB for K, n in todo)
    rig = SkRig(engine, built, k, longest, max(n for _, n in todo), max(n * NSUB for _, n in todo))
    try:
        for D in (M, M // 2):
            y = rig.frames(0, longest, D)
            d_mid = rig.upload(np.full((pfb_ref.samples_needed(M, T, D, longest), 2), 128, dtype=np.uint8))
            flagged = keptn = 0
            for K, n in todo:
                f, g = check_sums_and_decisions(rig, built, k, K, NSUB, n, D, y, d_mid)
                flagged, keptn = flagged + f, keptn + g
            print("pfbsk, M = %d, hop %d: %d sub-integrations flagged, %d kept (K = %s)" % (M, D, flagged, keptn, [K for K, _ in todo]))
            assert flagged > 0 and keptn > 0, (k, D, flagged, keptn)              # both outcomes occur
    finally:
        rig.close()


@pytest.mark.parametrize("k", ksum.LOG2_MS)
def test_every_walk_geometry_to_the_bit(engine, built, k):
    """Every (K, L) of tests/pfbsk_walk_cases.py, both hops, T = 3, three rows: the same checks at every walk of a row's
    L sub-integrations through its tiles (one partial step up to the last item short of a full tile, a full step, two
    and three steps with a full and with a ragged last one; L = 1 and 2 where a step holds one sub-integration).  The
    capture is as long as the longest case needs at hop M, so that run reads it to its last sample."""
    M = 1 << k
    cases, n = walks.walk_cases(k), walks.ROWS
    for K, L in cases:
        rc, blocks, _, _, per = built.pfbsk_grid(k, T, M, K, L, 1)
        assert rc == 0 and per >= 1 and blocks == 1 and built.pfbsk_supported(k, T, M // 2, K, L) == 1
    longest = max(walks.frames(K, L) for K, L in cases)
    rig = SkRig(engine, built, k, longest, n, max(n * L for _, L in cases))
    try:
        assert any(len(rig.iqs[0]) == pfbsk_ref.samples_needed(M, T, M, K, L, n) for K, L in cases)
        for D in (M, M // 2):
            y = rig.frames(0, longest, D)
            d_mid = rig.upload(np.full((pfb_ref.samples_needed(M, T, D, longest), 2), 128, dtype=np.uint8))
            flagged = keptn = 0
            for K, L in cases:
                f, g = check_sums_and_decisions(rig, built, k, K, L, n, D, y, d_mid)
                flagged, keptn = flagged + f, keptn + g
            print("pfbsk walks, M = %d, hop %d: %d (K, L), %d sub-integrations flagged, %d kept" % (M, D, len(cases), flagged, keptn))
            assert flagged > 0 and keptn > 0, (k, D, flagged, keptn)              # both outcomes occur
    finally:
        rig.close()


@pytest.mark.parametrize("K,L", [(ksum.MAX_K_AVG, 2), (16, pfbsk_ref.MAX_NSUB)])
def test_the_largest_shapes_once(engine, built, K, L):
    """log2 M = 4, hop M, T = 1, one row: the largest K, and the largest L."""
    k, taps_per_branch = 4, 1
    M = 1 << k
    assert built.pfbsk_supported(k, taps_per_branch, M, K, L) == 1
    assert built.pfbsk_supported(k, taps_per_branch, M, K + 1, L) == 0 or built.pfbsk_supported(k, taps_per_branch, M, K, L + 1) == 0
    rig = SkRig(engine, built, k, K * L, 1, L, taps_per_branch)
    try:
        d_mid = rig.upload(np.full((pfb_ref.samples_needed(M, taps_per_branch, M, K * L), 2), 128, dtype=np.uint8))
        f, g = check_sums_and_decisions(rig, built, k, K, L, 1, M, rig.frames(0, K * L, M), d_mid)
    finally:
        rig.close()
    print("pfbsk, M = %d, K = %d, L = %d: %d sub-integrations flagged, %d kept" % (M, K, L, f, g))


def test_l1_and_k1_edges(engine, built):
    """L = 1 under open bounds is the spectrometer, at a K of each path; at K = 1 the ratio is exactly 1, so a ratio_lo
    just above 1 flags everything: the N = 0 rule through all three output kinds."""
    k = 6
    M, F = 1 << k, ksum.tile_frames(k)
    n = 5
    rig = SkRig(engine, built, k, (F + 1) * n, n, 3 * n)
    try:
        for D in (M, M // 2):
            for K in (3, F + 1):                                         # K < F and K >= F
                clean, kept, s1, _ = rig.run(rig.d_iqs[0], K, 1, n, D)
                want = rig.spec(rig.d_iqs[0], K, n, D)
                assert np.array_equal(u32(clean), u32(want)) and np.array_equal(u32(s1), u32(want)) and np.all(kept == 1), (K, D)
            above = (float(np.nextafter(np.float32(1), np.float32(2))), math.inf)
            for L in (1, 3):
                clean, kept, s1, s2 = rig.run(rig.d_iqs[0], 1, L, n, D, above)
                assert np.all(s1 > 0) and np.all(s2 > 0)
                assert not u32(clean).any() and not kept.any(), (L, D)
                assert np.all(rig.run(rig.d_iqs[0], 1, L, n, D, (1.0, 1.0))[1] == L)        # the ratio is exactly 1
                db = rig.run(rig.d_iqs[0], 1, L, n, D, above, output="db", scale=1e-9)[0]
                assert np.all(np.isneginf(db)), (L, D)
                assert not rig.run(rig.d_iqs[0], 1, L, n, D, above, output="payload", scale=1e20)[0].any(), (L, D)
    finally:
        rig.close()


@pytest.mark.parametrize("i", range(len(pfbsk_ref.SEMANTIC_SHAPES)))
def test_semantic_case(engine, built, i):
    """Noise, a steady tone and a gated tone through designed taps (tests/pfbsk_ref.py): the device's flags agree with
    the f64 reference's wherever the f64 ratio is more than 1 % from both bounds (at most 2 % are not), the steady
    tone's channel is flagged everywhere and the burst's where the bursts are; the clean row of the L-sub-integration
    run is the sum of the unflagged short rows, and the burst's channel lies under pfbspec_ref.bound(k, K N) of the f64
    sum over the same kept set."""
    k, T_, D, K, L, iq, taps, scale, lo, hi = pfbsk_ref.semantic_case(i)
    M, rows = 1 << k, pfbsk_ref.SEMANTIC_ROWS
    nq = rows * L
    assert built.pfbsk_power_scale(k, taps) == scale and built.pfbsk_bounds(K, *SK) == (float(lo), float(hi))
    _, _, s1_64, s2_64 = pfbsk_ref.pfbsk_ref(iq, k, taps, K, L, lo, hi, scale, D, nspectra=rows)
    r = pfbsk_ref.ratio(s1_64, s2_64, K, scale)
    flags64 = pfbsk_ref.flagged(s1_64, s2_64, K, scale, lo, hi)
    near = pfbsk_ref.near_a_bound(r, lo, hi)
    assert near.mean() <= 0.02, near.mean()
    # flags, read as N of L = 1 rows
    short, n1, s1, s2 = engine.pfbsk(iq, k, taps, K, 1, lo, hi, scale, hop=D, nspectra=nq, sub_rows=True)
    assert n1.shape == (nq, M) and n1.max() <= 1
    flags = n1 == 0
    assert np.array_equal(flags[~near], flags64[~near]), (i, np.argwhere((flags != flags64) & ~near)[:4])
    tone, burst, where = pfbsk_ref.tone_channel(M), pfbsk_ref.burst_channel(M), list(pfbsk_ref.burst_subs(L))
    assert flags[:, tone].all() and flags[where, burst].all()
    assert np.array_equal(u32(short), u32(np.where(flags, np.float32(0), s1)))
    # the long run: the sum of the unflagged short rows, in order
    clean, kept = engine.pfbsk(iq, k, taps, K, L, lo, hi, scale, hop=D, nspectra=rows)
    want_c, want_n = pfbsk_ref.clean_rows_f32(s1, flags, L)
    assert np.array_equal(kept, want_n) and np.array_equal(u32(clean), u32(want_c))
    assert np.all(kept[:, tone] == 0) and np.all(kept[:, burst] <= L - 1) and np.all(kept[:, burst] >= 1)
    ref = np.where(flags, 0.0, s1_64).reshape(rows, L, M).sum(axis=1)              # the f64 sum over the device's kept set
    worst = 0.0
    for j in range(rows):
        ratio = abs(float(clean[j, burst]) - ref[j, burst]) / (pfbspec_ref.bound(k, K * int(kept[j, burst])) * ref[j, burst])
        worst = max(worst, ratio)
    print("semantic case %d: %.2f %% of the ratios near a bound, %d flags differ there, burst channel at %.4f of its bound"
          % (i, 100 * near.mean(), int((flags != flags64).sum()), worst))
    assert worst <= 1.0, worst


@pytest.mark.parametrize("k,T_,hop_div", pfbspec_ref.DB_SHAPES)
def test_db_and_bytes(engine, built, k, T_, hop_div):
    """Tied to the device's own C and N: MEAN_DB within 2e-4 dB (rtlws_hip.h's figure for this output kind) of
    10 log10(C scale / (K N)) in f64; PAYLOAD_U8 equal to the truncated, clamped f64 value except +-1 where that value
    lies within 1e-3 of an integer; channels with N = 0 read -inf and 0."""
    M, L, n = 1 << k, pfbsk_ref.DB_NSUB, pfbsk_ref.DB_ROWS
    for K in (3, ksum.tile_frames(k) + 1):
        iq, taps, D, scale, pscale, lo, hi = pfbsk_ref.db_case(k, T_, hop_div, K)
        for shifted in (False, True):
            clean, kept = engine.pfbsk(iq, k, taps, K, L, lo, hi, pscale, hop=D, shifted=shifted, nspectra=n)
            assert (kept == 0).any() and (kept == L).any()
            want = pfbsk_ref.db(clean, kept, scale, K)
            got, kept_db = engine.pfbsk(iq, k, taps, K, L, lo, hi, pscale, hop=D, output="db", shifted=shifted, scale=scale, nspectra=n)
            assert got.shape == (n, M) and got.dtype == np.float32 and np.array_equal(kept_db, kept)
            assert np.all(np.isneginf(got[kept == 0])) and np.all(np.isfinite(got[kept > 0]))
            err = np.abs(got[kept > 0].astype(np.float64) - want[kept > 0]).max()
            assert err <= 2e-4, (K, shifted, err)
            assert 20.0 <= want[kept > 0].min() and want[kept > 0].max() <= 120.0
            byt, _ = engine.pfbsk(iq, k, taps, K, L, lo, hi, pscale, hop=D, output="payload", shifted=shifted, scale=scale, nspectra=n)
            assert byt.shape == (n, M) and byt.dtype == np.uint8 and not byt[kept == 0].any()
            exact = pfbspec_ref.payload(want)
            off = byt != exact
            assert np.all(np.abs(byt.astype(int) - exact.astype(int))[off] == 1), (K, shifted)
            assert np.all(pfbspec_ref.near_integer(want, 1e-3)[off]), (K, shifted)
            assert off.mean() <= 0.01, (K, shifted, off.mean())


def test_strides_and_nothing_outside_the_rows(engine, built):
    """Guard patterns at strides > M in all four buffers; d_kept, and d_s1 with d_s2, may be NULL."""
    k, K, L, n = 5, 3, 4, 3
    M = 1 << k
    taps = pfb_ref.random_taps(k, T, seed=21)
    scale = built.pfbsk_power_scale(k, taps)
    sk = sk_bounds(built, K)
    plan = built.PfbSkPlan.open(engine, k, taps)
    try:
        for D in (M, M // 2):
            iq = pfb_ref.random_iq(pfbsk_ref.samples_needed(M, T, D, K, L, n), seed=22)
            want = engine.pfbsk(iq, k, taps, K, L, sk[0], sk[1], scale, hop=D, sub_rows=True)
            d_iq = engine.upload(iq)
            for output, dtype, sentinel, cstride in (("power", np.float32, np.float32(-12345.5), M + 4),
                                                     ("payload", np.uint8, np.uint8(0xA5), M + 16)):
                kstride, sstride, tail = M + 8, M + 12, 64
                hosts = [np.full(n * cstride + tail, sentinel, dtype=dtype), np.full(n * kstride + tail, 0xDEADBEEF, dtype=np.uint32),
                         np.full(n * L * sstride + tail, np.float32(-777.25)), np.full(n * L * sstride + tail, np.float32(-888.25))]
                bufs = [engine.upload(h) for h in hosts]

                def run(kept, s1, s2):
                    plan.run(d_iq, n, K, L, scale, bufs[0], sk[0], sk[1], kept, s1, s2, hop=D, output=output, scale=1e-9,
                             clean_stride=cstride, kept_stride=kstride, sub_stride=sstride)
                    engine.sync()
                    return [engine.download(b, h.dtype, h.shape) for b, h in zip(bufs, hosts)]

                # the optional buffers left out: they keep their pattern
                out = run(None, None, None)
                assert all(np.array_equal(o, h) for o, h in zip(out[1:], hosts[1:]))
                first_clean = out[0]
                out = run(bufs[1], None, None)
                assert all(np.array_equal(o, h) for o, h in zip(out[2:], hosts[2:])) and np.array_equal(out[0], first_clean)
                out = run(bufs[1], bufs[2], bufs[3])
                assert np.array_equal(out[0], first_clean)
                for o, h, stride, rows, ref in zip(out, hosts, (cstride, kstride, sstride, sstride), (n, n, n * L, n * L), want):
                    body = o[:rows * stride].reshape(rows, stride)
                    assert np.all(body[:, M:] == h[0]) and np.all(o[rows * stride:] == h[0]), (D, output, stride)
                    if output == "power" or stride != cstride:
                        assert np.array_equal(u32(body[:, :M]), u32(ref)), (D, output, stride)
                if output == "payload":
                    want_b = engine.pfbsk(iq, k, taps, K, L, sk[0], sk[1], scale, hop=D, output="payload", scale=1e-9)[0]
                    assert np.array_equal(out[0][:n * cstride].reshape(n, cstride)[:, :M], want_b) and want_b.any()
                # with a device the refusals still hold and write nothing
                for kw, word in (({"hop": M // 4}, "hop"), ({"clean_stride": 16}, "clean_stride"), ({"kept_stride": 16}, "kept_stride"),
                                 ({"sub_stride": 16}, "sub_stride"), ({"shifted": 2}, "shifted")):
                    args = dict(hop=D, output=output, clean_stride=cstride, kept_stride=kstride, sub_stride=sstride)
                    args.update(kw)
                    rc = plan.run(d_iq, n, K, L, scale, bufs[0], sk[0], sk[1], bufs[1], bufs[2], bufs[3], check=False, **args)
                    assert rc == -1 and word in built.pfbsk_last_error(), kw
                assert plan.run(d_iq, 0, K, L, scale, bufs[0], hop=D, output=output, clean_stride=cstride) == 0
                engine.sync()
                assert all(np.array_equal(engine.download(b, h.dtype, h.shape).view(np.uint8), o.view(np.uint8)) for b, h, o in zip(bufs, hosts, out))
                for b in bufs:
                    b.free()
            d_iq.free()
    finally:
        plan.close()


@pytest.mark.parametrize("k,K,L", [(5, 3, 4), (8, 17, 3), (10, 2, 5)])
def test_two_runs_and_a_sub_capture_give_the_same_bits(engine, built, k, K, L):
    M, n, j0 = 1 << k, 5, 2
    taps = pfb_ref.random_taps(k, T, seed=k)
    scale = built.pfbsk_power_scale(k, taps)
    sk = sk_bounds(built, K)
    for D in (M, M // 2):
        iq = pfb_ref.random_iq(pfbsk_ref.samples_needed(M, T, D, K, L, n), seed=K + L)
        whole = engine.pfbsk(iq, k, taps, K, L, sk[0], sk[1], scale, hop=D, sub_rows=True)
        assert 0 < (whole[1] < L).sum() and 0 < (whole[1] > 0).sum()
        again = engine.pfbsk(iq, k, taps, K, L, sk[0], sk[1], scale, hop=D, sub_rows=True)
        part = engine.pfbsk(iq[j0 * L * K * D:], k, taps, K, L, sk[0], sk[1], scale, hop=D, sub_rows=True)
        for w, a, p, per in zip(whole, again, part, (1, 1, L, L)):
            assert np.array_equal(u32(a), u32(w)) and p.shape == w[j0 * per:].shape and np.array_equal(u32(p), u32(w[j0 * per:])), (k, D)


def _hip_runtime(built):
    """The HIP runtime the library itself launches with: its symbols are looked up through the library's own
    dependencies, so a second copy of the runtime in the process (one that torch brings) is not taken by mistake."""
    return C.CDLL(built.PFBSK_LIB)


def test_capture_into_a_graph_of_one_node(engine, built):
    """A run is one kernel launch and no other runtime call: captured into a hipGraph it is a single kernel node, and
    the replayed rows match the direct launch."""
    k, K, L, n = 6, 5, 3, 4
    M, D = 1 << k, 1 << (k - 1)
    taps = pfb_ref.random_taps(k, 4, seed=31)
    scale = built.pfbsk_power_scale(k, taps)
    sk = sk_bounds(built, K)
    iq = pfb_ref.random_iq(pfbsk_ref.samples_needed(M, 4, D, K, L, n), seed=32)
    want = engine.pfbsk(iq, k, taps, K, L, sk[0], sk[1], scale, hop=D, shifted=True, sub_rows=True)
    hip = _hip_runtime(built)
    plan = built.PfbSkPlan.open(engine, k, taps)
    d_iq = engine.upload(iq)
    shapes = ((n, M), (n, M), (n * L, M), (n * L, M))
    bufs = [engine.upload(np.zeros(s, np.uint32)) for s in shapes]
    stream, graph, exe, count = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t(0)
    try:
        assert hip.hipStreamCreate(C.byref(stream)) == 0
        assert hip.hipStreamBeginCapture(stream, 1) == 0                         # hipStreamCaptureModeThreadLocal
        rc = plan.run(d_iq, n, K, L, scale, bufs[0], sk[0], sk[1], bufs[1], bufs[2], bufs[3], hop=D, shifted=True,
                      stream=stream.value, check=False)
        assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0 and rc == 0, built.pfbsk_last_error()
        assert hip.hipGraphGetNodes(graph, None, C.byref(count)) == 0 and count.value == 1
        node, kind = C.c_void_p(), C.c_int(-1)
        assert hip.hipGraphGetNodes(graph, C.byref(node), C.byref(count)) == 0
        assert hip.hipGraphNodeGetType(node, C.byref(kind)) == 0 and kind.value == 0          # hipGraphNodeTypeKernel
        engine.sync()
        assert not any(engine.download(b, np.uint32, s).any() for b, s in zip(bufs, shapes))   # capture enqueued nothing
        assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, C.c_size_t(0)) == 0
        for _ in range(2):
            assert hip.hipGraphLaunch(exe, stream) == 0 and hip.hipStreamSynchronize(stream) == 0
            for b, s, w in zip(bufs, shapes, want):
                assert np.array_equal(engine.download(b, np.uint32, s), u32(w))
    finally:
        if exe:
            hip.hipGraphExecDestroy(exe)
        if graph:
            hip.hipGraphDestroy(graph)
        if stream:
            hip.hipStreamDestroy(stream)
        plan.close()
        for b in bufs + [d_iq]:
            b.free()
