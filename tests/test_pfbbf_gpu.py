"""GPU suite of include/rtlws_pfbbf.h, through the C ABI: the polyphase beamformer (every capture through one tile of
the filter bank in turn, the beams summed in registers, one launch) against the channelizer's own samples and the
spectrometer's rows bit for bit, and against the numpy restatement tests/pfbbf_ref.py.

The accuracy criteria are derived, not measured (pfbbf_ref.bound and power_bound): per (frame, beam)
||got - ref||_2 <= (8 (log2 M + 1) + A + 3) 2^-24 N with N = sum_a max_c |W[b][a][c]| ||Y_a[m]||_2, and per power row
||got - ref||_1 <= (16 (log2 M + 1) + 2 A + K + 10) 2^-24 sum_m N[m]^2."""
import numpy as np
import pytest

import pfb_ref
import pfbbf_ref

pytestmark = pytest.mark.gpu

NSPECTRA = (1, 2, 5)
MULTI_SHAPES = ((4, 7), (6, 8), (10, 4))                    # where (A, B) = (1, 1), (3, 2) and (8, 4) run
CASES = [(k, T, 2, 1) for k, T in pfb_ref.SHAPES] + [(k, T, A, B) for k, T in MULTI_SHAPES for A, B in ((1, 1), (3, 2), (8, 4))]
MULTI_CASES = [(k, T, A, B) for k, T in MULTI_SHAPES for A, B in ((3, 2), (8, 4))]
FIRSTS = (0, 7)                                             # first_frame_index: 0 and an odd value


def k_list(F):
    return sorted({K for K in (1, 2, 3, F - 1, F, F + 1, 2 * F + 3) if K >= 1})


def frame_counts(F):
    return (1, F - 1, F, F + 1, 2 * F + 3)


def u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


class Bank:
    """The captures of one (k, taps) on the device, uploaded once (a capture given twice: one buffer, its pointer
    twice), with the beamformer's plan for B beams, the channelizer's and the spectrometer's, and output buffers for
    max_frames frames of B beams."""

    def __init__(self, engine, built, k, taps, iqs, B, max_frames):
        self.eng, self.built, self.k, self.M, self.A, self.B, self.taps = engine, built, k, 1 << k, len(iqs), B, taps
        self.bufs = {}
        for x in iqs:
            if id(x) not in self.bufs:
                self.bufs[id(x)] = engine.upload(x)
        self.d_iqs = [self.bufs[id(x)] for x in iqs]
        self.plan = built.PfbBfPlan.open(engine, k, taps, self.A, B)
        self.spec_plan = built.PfbSpecPlan.open(engine, k, taps)
        self.pfb_plan = built.PfbPlan.open(engine, k, taps)
        self.d_out = engine.alloc(B * max_frames * self.M * 8)
        self.d_tmp = engine.alloc(max_frames * self.M * 8)
        self.d_w = None

    def weights(self, W):
        W = np.ascontiguousarray(W, dtype=np.complex64)
        assert W.shape == (self.B, self.A, self.M)
        if self.d_w is not None:
            self.d_w.free()
        self.d_w = self.eng.upload(W)
        return W

    def volts(self, n, D, first=0, layout="time", first_sample=0):
        """-> complex64 [B, n, M] ("time") or [B, M, n] ("channel"); the captures from sample first_sample on"""
        assert (2 * first_sample) % 16 == 0
        self.plan.run([b.ptr + 2 * first_sample for b in self.d_iqs], self.d_w, n, self.d_out, hop=D, first_frame_index=first, layout=layout)
        self.eng.sync()
        return self.eng.download(self.d_out, np.complex64, (self.B, n, self.M) if layout == "time" else (self.B, self.M, n))

    def power(self, K, n, D, shifted=False, first_sample=0):
        """-> float32 [n, B, M]"""
        assert (2 * first_sample) % 16 == 0
        self.plan.power([b.ptr + 2 * first_sample for b in self.d_iqs], self.d_w, n, K, self.d_out, hop=D, shifted=shifted)
        self.eng.sync()
        return self.eng.download(self.d_out, np.float32, (n, self.B, self.M))

    def spec(self, a, K, n, D, shifted=False):
        """rtlws_pfbspec_run's raw sums of capture a -> float32 [n, M]"""
        self.spec_plan.run(self.d_iqs[a], n, K, self.d_tmp, hop=D, shifted=shifted)
        self.eng.sync()
        return self.eng.download(self.d_tmp, np.float32, (n, self.M))

    def frames(self, a, n, D, first=0):
        """rtlws_pfb_run's time-major samples of capture a, the sign rule applied -> complex64 [n, M]"""
        self.pfb_plan.run(self.d_iqs[a], n, self.d_tmp, hop=D, first_frame_index=first, layout="time")
        self.eng.sync()
        return self.eng.download(self.d_tmp, np.complex64, (n, self.M))

    def raw_frames(self, n, D):
        """every capture's frames with the sign rule undone by the same bit flip -> A arrays complex64 [n, M]"""
        done = {}
        for a, b in enumerate(self.d_iqs):
            if id(b) not in done:
                done[id(b)] = pfbbf_ref.flip(self.frames(a, n, D), self.M, D, 0)
        return [done[id(b)] for b in self.d_iqs]

    def close(self):
        for p in (self.plan, self.spec_plan, self.pfb_plan):
            p.close()
        for b in list(self.bufs.values()) + [self.d_out, self.d_tmp] + ([self.d_w] if self.d_w is not None else []):
            b.free()


@pytest.mark.parametrize("k,T,A,B", CASES)
def test_voltages_are_the_channelizers_samples_weighted_bit_for_bit(engine, built, k, T, A, B):
    """rtlws_pfb_run's time-major samples of every capture, its sign rule undone by the bit flip, weighted and summed
    in numpy f32 in the definition's order from +0, the flip applied again: equal as uint32 to the device in both
    layouts, with first_frame_index 0 and odd, at both hops, for frame counts across the tile's borders."""
    M, F = 1 << k, 4096 >> k
    ns = frame_counts(F)
    taps = pfb_ref.random_taps(k, T, seed=100 * k + T)
    iqs = pfbbf_ref.random_captures(A, pfb_ref.samples_needed(M, T, M, max(ns)), seed=3 * k + T)
    bank = Bank(engine, built, k, taps, iqs, B, max(ns))
    W = bank.weights(pfbbf_ref.random_weights(B, A, M, seed=k + A))
    try:
        for D in (M, M // 2):
            for n in ns:
                z = pfbbf_ref.beams_f32(bank.raw_frames(n, D), W)
                assert z.dtype == np.complex64 and z.shape == (B, n, M) and np.any(z.real != 0) and np.any(z.imag != 0)
                for first in FIRSTS:
                    want = pfbbf_ref.flip(z, M, D, first)
                    got = bank.volts(n, D, first, "time")
                    assert np.array_equal(u32(got), u32(want)), (D, n, first, "time")
                    got = bank.volts(n, D, first, "channel")
                    assert np.array_equal(u32(got), u32(want.transpose(0, 2, 1))), (D, n, first, "channel")
    finally:
        bank.close()


@pytest.mark.parametrize("k,T,A,B", CASES)
def test_one_hot_beams_are_the_channelizer_and_the_spectrometer(engine, built, k, T, A, B):
    """Beam b passes capture (b + 1) mod A alone with weight 1 + 0i: its voltages equal rtlws_pfb_run's by value
    (the sign of a zero may differ) and its power rows are rtlws_pfbspec_run's RTLWS_OUT_POWER_SUM rows as uint32,
    shifted and unshifted, K across the tile's borders, nspectra that do and do not fill a workgroup."""
    M, F = 1 << k, 4096 >> k
    ks = k_list(F)
    longest = max(ks) * max(NSPECTRA)
    which = [(b + 1) % A for b in range(B)]
    taps = pfb_ref.random_taps(k, T, seed=100 * k + T)
    iqs = pfbbf_ref.random_captures(A, pfb_ref.samples_needed(M, T, M, longest), seed=k + T)
    bank = Bank(engine, built, k, taps, iqs, B, longest)
    bank.weights(pfbbf_ref.one_hot(B, A, M, which))
    try:
        for D in (M, M // 2):
            for n in frame_counts(F):
                for first in FIRSTS:
                    got = bank.volts(n, D, first, "time")
                    got_c = bank.volts(n, D, first, "channel")
                    for b, a in enumerate(which):
                        want = bank.frames(a, n, D, first)
                        assert np.any(want != 0) and np.array_equal(got[b], want), (D, n, first, b)
                        assert np.array_equal(got_c[b], want.T), (D, n, first, b)
            for shifted in (False, True):
                for K in ks:
                    for n in NSPECTRA:
                        got = bank.power(K, n, D, shifted)
                        for b, a in enumerate(which):
                            want = bank.spec(a, K, n, D, shifted)
                            assert np.all(want > 0)
                            assert np.array_equal(u32(got[:, b]), u32(want)), (D, shifted, K, n, b)
    finally:
        bank.close()


@pytest.mark.parametrize("k,T,A,B", CASES)
def test_power_is_the_ordered_sum_of_the_voltages(engine, built, k, T, A, B):
    """For every K the power rows equal pfbxc_ref.ordered_sums of the f32 products of the voltage run's own download,
    as uint32: the order of the sums is pinned with no tolerance (the sign rule does not reach a product)."""
    M, F = 1 << k, 4096 >> k
    ks = k_list(F)
    nmax = max(NSPECTRA)
    longest = max(ks) * nmax
    taps = pfb_ref.random_taps(k, T, seed=100 * k + T)
    iqs = pfbbf_ref.random_captures(A, pfb_ref.samples_needed(M, T, M, longest), seed=5 * k + T)
    bank = Bank(engine, built, k, taps, iqs, B, longest)
    bank.weights(pfbbf_ref.random_weights(B, A, M, seed=k + B))
    try:
        for D in (M, M // 2):
            z = bank.volts(longest, D, 7 if D != M else 0, "time")         # a shorter run is a prefix: the same frames
            for K in ks:
                want = pfbbf_ref.power_f32(z[:, :K * nmax], k, K)
                assert want.shape == (nmax, B, M) and np.all(want > 0)
                for n in NSPECTRA:
                    got = bank.power(K, n, D)
                    assert np.array_equal(u32(got), u32(want[:n])), (D, K, n)
                got = bank.power(K, nmax, D, shifted=True)
                assert np.array_equal(u32(got), u32(np.fft.fftshift(want, axes=2))), (D, K)
    finally:
        bank.close()


def worst_ratios(engine, built, k, T, A, B):
    """-> (the worst ratio of the voltages to pfbbf_ref.bound, of the power rows to pfbbf_ref.power_bound) over random
    bytes with random taps and 0/255 bytes with every tap 32767, random weights, both hops, K across the tile's
    borders; every single ratio is asserted."""
    M, F = 1 << k, 4096 >> k
    ks = k_list(F)
    nmax = max(NSPECTRA)
    longest = max(ks) * nmax
    ns = pfb_ref.samples_needed(M, T, M, longest)
    worst_v = worst_p = 0.0
    cases = (("random", pfbbf_ref.random_captures(A, ns, seed=k + T), pfb_ref.random_taps(k, T, seed=100 * k + T)),
             ("full scale", [pfb_ref.full_scale_iq(ns, seed=k * T + a) for a in range(A)], np.full(T * M, 32767, np.int16)))
    for kind, iqs, taps in cases:
        bank = Bank(engine, built, k, taps, iqs, B, longest)
        W = bank.weights(pfbbf_ref.random_weights(B, A, M, seed=7 * k + A))
        try:
            for D in (M, M // 2):
                ys = pfbbf_ref.frames_of(iqs, k, taps, D, longest)
                zref = pfbbf_ref.beams(ys, W)
                for n in frame_counts(F):
                    for first in FIRSTS:
                        got = bank.volts(n, D, first, "time")
                        rv = pfbbf_ref.voltage_ratio(got, zref[:, :n] * pfbbf_ref.signs(M, D, first, n)[None], [y[:n] for y in ys], W, k)
                        worst_v = max(worst_v, rv)
                        assert rv <= 1.0, (kind, D, n, first, rv)
                for K in ks:
                    ref = pfbbf_ref.k_sums(zref, K)
                    for n in NSPECTRA:
                        rp = pfbbf_ref.power_ratio(bank.power(K, n, D), ref[:n], ys, W, k, K)
                        worst_p = max(worst_p, rp)
                        assert rp <= 1.0, (kind, D, K, n, rp)
        finally:
            bank.close()
    return worst_v, worst_p


@pytest.mark.parametrize("k,T,A,B", CASES)
def test_voltages_and_powers_against_f64(engine, built, k, T, A, B):
    wv, wp = worst_ratios(engine, built, k, T, A, B)
    print("M = %d, T = %d, A = %d, B = %d: worst voltage ratio to the bound %.4f, worst power ratio %.4f" % (1 << k, T, A, B, wv, wp))


@pytest.mark.parametrize("k,T,A,B", MULTI_CASES)
def test_reproducible_and_independent_of_the_other_beams(engine, built, k, T, A, B):
    """Two runs give the same bits.  Beam b alone, through a plan for one beam, gives the bits it has among B beams:
    it does not depend on B or on the other beams' weights.  Voltage runs in chunks that pass first_frame_index
    concatenate to one run's bits.  A power run over the captures from sample j0 K D on gives rows j0 .. of the whole
    run; nspectra = 1 gives row 0."""
    M, F = 1 << k, 4096 >> k
    taps = pfb_ref.random_taps(k, T, seed=k)
    for K in (3, F + 1):
        per = built.pfbbf_grid(k, T, M, K, 1)[4]
        n = 2 * per + 3                                        # three workgroups, the last one partly filled
        j0 = per // 2 + 1                                      # rows that change their place in the tile and in the grid
        iqs = pfbbf_ref.random_captures(A, pfbbf_ref.samples_needed(M, T, M, K, n), seed=T + K)
        bank = Bank(engine, built, k, taps, iqs, B, n * K)
        solo = Bank(engine, built, k, taps, iqs, 1, n * K)
        W = bank.weights(pfbbf_ref.random_weights(B, A, M, seed=K))
        try:
            for D in (M, M // 2):
                nf = n * K
                cut = min(F + 1, nf - 1)                       # an odd number of frames into the run, across a tile
                for layout in ("time", "channel"):
                    z = bank.volts(nf, D, 5, layout)
                    assert np.array_equal(u32(bank.volts(nf, D, 5, layout)), u32(z)), (K, D, layout)
                    head = bank.volts(cut, D, 5, layout)
                    tail = bank.volts(nf - cut, D, 5 + cut, layout, first_sample=cut * D)
                    assert np.array_equal(u32(np.concatenate([head, tail], axis=1 if layout == "time" else 2)), u32(z)), (K, D, layout)
                rows = bank.power(K, n, D)
                assert rows.shape == (n, B, M) and np.all(rows > 0)
                assert np.array_equal(u32(bank.power(K, n, D)), u32(rows)), (K, D)
                for start in (j0, n - 1):
                    assert np.array_equal(u32(bank.power(K, n - start, D, first_sample=start * K * D)), u32(rows[start:])), (K, D, start)
                assert np.array_equal(u32(bank.power(K, 1, D)), u32(rows[:1])), (K, D)
                z = bank.volts(nf, D, 5, "time")
                for b in range(B):
                    solo.weights(W[b:b + 1])
                    assert np.array_equal(u32(solo.volts(nf, D, 5, "time")[0]), u32(z[b])), (K, D, b)
                    assert np.array_equal(u32(solo.power(K, n, D)[:, 0]), u32(rows[:, b])), (K, D, b)
        finally:
            solo.close()
            bank.close()


@pytest.mark.parametrize("k,T", MULTI_SHAPES)
def test_degenerate_inputs(engine, built, k, T):
    """All-128 captures: +0 power bits and zero voltages.  All-zero weights: the same.  One pointer given for every
    input with the weights (+1, -1): exactly zero in both modes, beside a beam that passes the capture."""
    M, F = 1 << k, 4096 >> k
    ks = (1, 3, F + 1)
    n = 3
    taps = pfb_ref.random_taps(k, T, seed=5 * k)
    nmax = pfb_ref.samples_needed(M, T, M, max(ks) * n)
    x = pfb_ref.random_iq(nmax, seed=k)
    mid = np.full((nmax, 2), 128, dtype=np.uint8)
    cancel = pfbbf_ref.one_hot(2, 2, M, (0, 0))
    cancel[0, 1] = -1.0
    dead = Bank(engine, built, k, taps, [mid, mid.copy(), mid], 2, max(ks) * n)
    mute = Bank(engine, built, k, taps, [x, mid, x], 2, max(ks) * n)
    same = Bank(engine, built, k, taps, [x, x], 2, max(ks) * n)
    dead.weights(pfbbf_ref.random_weights(2, 3, M, seed=1))
    mute.weights(np.zeros((2, 3, M), np.complex64))
    same.weights(cancel)
    try:
        assert same.d_iqs[0] is same.d_iqs[1]
        for D in (M, M // 2):
            for bank in (dead, mute):
                for layout in ("time", "channel"):
                    assert not bank.volts(max(ks) * n, D, 3, layout).any(), (D, layout)
                for K in ks:
                    for shifted in (False, True):
                        assert not u32(bank.power(K, n, D, shifted)).any(), (D, K)
            z = same.volts(max(ks) * n, D, 3, "time")
            assert not z[0].any() and np.array_equal(z[1], same.frames(0, max(ks) * n, D, 3))
            assert not same.volts(max(ks) * n, D, 3, "channel")[0].any()
            for K in ks:
                rows = same.power(K, n, D)
                assert not u32(rows[:, 0]).any(), (D, K)
                assert np.array_equal(u32(rows[:, 1]), u32(same.spec(0, K, n, D))), (D, K)
    finally:
        for bank in (dead, mute, same):
            bank.close()


def test_strides_and_nothing_outside(engine, built):
    """Sentinel-filled outputs with out_stride, beam_stride and row_stride above the least: the values lie under the
    bounds where they belong and every other byte is unchanged; with a device the refusals still hold and write
    nothing."""
    k, T, K, A, B = 5, 3, 3, 3, 2
    M, F = 1 << k, 4096 >> k
    nf = F + 5                                                 # two workgroups, the second partly filled
    per = built.pfbbf_grid(k, T, M, K, 1)[4]
    n = per + 3
    taps = pfb_ref.random_taps(k, T, seed=21)
    plan = built.PfbBfPlan.open(engine, k, taps, A, B)
    W = pfbbf_ref.random_weights(B, A, M, seed=22)
    d_w = engine.upload(W)
    sentinel = np.float32(-12345.5)
    tail = 64
    for D in (M, M // 2):
        iqs = pfbbf_ref.random_captures(A, pfbbf_ref.samples_needed(M, T, D, K, n), seed=23)
        assert n * K >= nf
        ys = pfbbf_ref.frames_of(iqs, k, taps, D, n * K)
        zref = pfbbf_ref.beams(ys, W)
        d_iqs = [engine.upload(x) for x in iqs]
        for layout, rows, cols in (("time", nf, M), ("channel", M, nf)):
            ostride = cols + 3
            bstride = rows * ostride + 5
            total = B * bstride + tail
            d_out = engine.upload(np.full(2 * total, sentinel, dtype=np.float32))
            plan.run(d_iqs, d_w, nf, d_out, hop=D, out_stride=ostride, beam_stride=bstride, first_frame_index=3, layout=layout)
            engine.sync()
            out = engine.download(d_out, np.float32, (total, 2))
            body = np.stack([out[b * bstride:b * bstride + rows * ostride].reshape(rows, ostride, 2) for b in range(B)])
            got = body[:, :, :cols, 0] + 1j * body[:, :, :cols, 1]
            got = got if layout == "time" else got.transpose(0, 2, 1)
            want = zref[:, :nf] * pfbbf_ref.signs(M, D, 3, nf)[None]
            assert pfbbf_ref.voltage_ratio(got, want, [y[:nf] for y in ys], W, k) <= 1.0, (D, layout)
            keep = np.ones(total, dtype=bool)
            for b in range(B):
                for r in range(rows):
                    keep[b * bstride + r * ostride:b * bstride + r * ostride + cols] = False
            assert np.all(out[keep] == sentinel) and not np.any(out[~keep] == sentinel), (D, layout)
            # the refusals with a device: nothing is written
            args = dict(hop=D, out_stride=ostride, beam_stride=bstride, first_frame_index=3, layout=layout)
            assert plan.run(d_iqs, d_w, 0, d_out, **args) == 0
            for kw, word in (({"hop": M // 4}, "hop"), ({"hop": 2 * M}, "hop"), ({"out_stride": cols - 1}, "out_stride"),
                             ({"beam_stride": (rows - 1) * ostride + cols - 1}, "beam_stride"), ({"first_frame_index": -1}, "first_frame_index"),
                             ({"layout": 2}, "layout"), ({"ninputs": A - 1}, "ninputs is not the plan's"), ({"nbeams": B - 1}, "nbeams is not the plan's"),
                             ({"nbeams": 5}, "nbeams")):
                a = dict(args)
                a.update(kw)
                assert plan.run(d_iqs, d_w, nf, d_out, check=False, **a) == -1 and word in built.pfbbf_last_error(), kw
            for bad, word in (([d_iqs[0], None, d_iqs[2]], "null pointer"), ([d_iqs[0], d_iqs[1], d_iqs[2].ptr + 8], "16-byte"), (None, "null pointer")):
                assert plan.run(bad, d_w, nf, d_out, check=False, **args) == -1 and word in built.pfbbf_last_error(), word
            assert plan.run(d_iqs, d_w.ptr + 8, nf, d_out, check=False, **args) == -1 and "d_weights" in built.pfbbf_last_error()
            assert plan.run(d_iqs, None, nf, d_out, check=False, **args) == -1 and "null pointer" in built.pfbbf_last_error()
            assert plan.run(d_iqs, d_w, nf, d_out.ptr + 4, check=False, **args) == -1 and "8-byte" in built.pfbbf_last_error()
            engine.sync()
            assert np.array_equal(u32(engine.download(d_out, np.float32, (total, 2))), u32(out))
            d_out.free()

        rstride = M + 4
        total = n * B * rstride + tail
        d_out = engine.upload(np.full(total, sentinel, dtype=np.float32))
        plan.power(d_iqs, d_w, n, K, d_out, hop=D, row_stride=rstride)
        engine.sync()
        out = engine.download(d_out, np.float32, (total,))
        body = out[:n * B * rstride].reshape(n, B, rstride)
        assert pfbbf_ref.power_ratio(body[:, :, :M], pfbbf_ref.k_sums(zref, K), ys, W, k, K) <= 1.0, D
        assert np.all(body[:, :, M:] == sentinel) and np.all(out[n * B * rstride:] == sentinel) and np.all(body[:, :, :M] > 0), D
        args = dict(hop=D, row_stride=rstride)
        assert plan.power(d_iqs, d_w, 0, K, d_out, **args) == 0
        for kw, word in (({"hop": M // 4}, "hop"), ({"row_stride": 16}, "row_stride must be >= M"), ({"row_stride": rstride + 2}, "row_stride must be a multiple of 4"),
                         ({"shifted": 2}, "shifted"), ({"ninputs": A + 1}, "ninputs is not the plan's"), ({"nbeams": B + 1}, "nbeams is not the plan's")):
            a = dict(args)
            a.update(kw)
            assert plan.power(d_iqs, d_w, n, K, d_out, check=False, **a) == -1 and word in built.pfbbf_last_error(), kw
        assert plan.power(d_iqs, d_w, n, 0, d_out, check=False, **args) == -1 and "k_avg" in built.pfbbf_last_error()
        assert plan.power(d_iqs, d_w, -1, K, d_out, check=False, **args) == -1 and "nspectra" in built.pfbbf_last_error()
        assert plan.power([d_iqs[0], None, d_iqs[2]], d_w, n, K, d_out, check=False, **args) == -1 and "null pointer" in built.pfbbf_last_error()
        assert plan.power(d_iqs, d_w.ptr + 8, n, K, d_out, check=False, **args) == -1 and "d_weights" in built.pfbbf_last_error()
        assert plan.power(d_iqs, d_w, n, K, d_out.ptr + 8, check=False, **args) == -1 and "16-byte" in built.pfbbf_last_error()
        engine.sync()
        assert np.array_equal(u32(engine.download(d_out, np.float32, (total,))), u32(out))
        for b in d_iqs + [d_out]:
            b.free()
    d_w.free()
    plan.close()


def test_capture_and_replay(built):
    """A run is one kernel launch: both modes captured on a side stream the way tests/test_pfbxc_gpu.py captures the
    correlator, replayed on the first weights and again after the weight buffer was overwritten: the replay gives the
    new weights' results, identical to eager launches."""
    import torch
    dev = torch.device("cuda", 0)
    eng = built.Engine(0)
    k, T, K, A, B = 6, 4, 5, 3, 2
    M, D = 1 << k, 1 << (k - 1)
    n = built.pfbbf_grid(k, T, D, K, 1)[4] + 5
    nf = n * K
    taps = pfb_ref.random_taps(k, T, seed=31)
    plan = built.PfbBfPlan.open(eng, k, taps, A, B)
    host = pfbbf_ref.random_captures(A, pfbbf_ref.samples_needed(M, T, D, K, n), seed=32)
    ys = pfbbf_ref.frames_of(host, k, taps, D, nf)
    iqs = [torch.from_numpy(x).to(dev) for x in host]
    weights = [pfbbf_ref.random_weights(B, A, M, seed=33), pfbbf_ref.random_weights(B, A, M, seed=34)]
    w = torch.zeros((B, A, M, 2), dtype=torch.float32, device=dev)
    volts = torch.zeros((B, nf, M, 2), dtype=torch.float32, device=dev)
    rows = torch.zeros((n, B, M), dtype=torch.float32, device=dev)

    def launch(v, r):
        st = built.torch_stream_handle()
        ptrs = [x.data_ptr() for x in iqs]
        plan.run(ptrs, w.data_ptr(), nf, v.data_ptr(), hop=D, first_frame_index=3, layout="time", stream=st)
        plan.power(ptrs, w.data_ptr(), n, K, r.data_ptr(), hop=D, shifted=True, stream=st)

    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            launch(volts, rows)
    torch.cuda.current_stream().wait_stream(side)
    assert float(volts.abs().sum()) == 0.0 and float(rows.abs().sum()) == 0.0      # capture enqueued nothing
    seen = []
    for W in weights:
        w.copy_(torch.from_numpy(np.ascontiguousarray(W).view(np.float32).reshape(B, A, M, 2)))
        volts.zero_()
        rows.zero_()
        g.replay()
        torch.cuda.synchronize()
        eager_v, eager_r = torch.zeros_like(volts), torch.zeros_like(rows)
        launch(eager_v, eager_r)
        torch.cuda.synchronize()
        assert torch.equal(volts, eager_v) and torch.equal(rows, eager_r)
        v = volts.cpu().numpy()
        zref = pfbbf_ref.beams(ys, W)
        assert pfbbf_ref.voltage_ratio(v[..., 0] + 1j * v[..., 1], zref * pfbbf_ref.signs(M, D, 3, nf)[None], ys, W, k) <= 1.0
        assert pfbbf_ref.power_ratio(rows.cpu().numpy(), pfbbf_ref.k_sums(zref, K, shifted=True), ys, W, k, K) <= 1.0
        seen.append(rows.cpu().numpy())
    assert not np.array_equal(seen[0], seen[1])
    plan.close()
    eng.close()


def test_the_delay_case_on_the_device(engine, built):
    """pfbbf_ref.delay_case() through the library: the steered beam over four captures that lag by 0, 1, 3, 6 samples
    and the nulled beam over the first two agree with the restatement under the bound, and show the restatement's
    gain and depth (tests/test_pfbbf_cpu.py holds the thresholds to the restatement's own figures)."""
    k, taps, D, K, iqs, w_steer, w_null = pfbbf_ref.delay_case()
    steer = engine.pfbbf_power(iqs, w_steer, k, taps, K, hop=D, nspectra=1)
    null = engine.pfbbf_power(iqs[:2], w_null, k, taps, K, hop=D, nspectra=1)
    assert steer.shape == (1, 2, 64) and null.shape == (1, 2, 64) and steer.dtype == np.float32
    ys = pfbbf_ref.frames_of(iqs, k, taps, D, K)
    rs = pfbbf_ref.power_ratio(steer, pfbbf_ref.k_sums(pfbbf_ref.beams(ys, w_steer), K), ys, w_steer, k, K)
    rn = pfbbf_ref.power_ratio(null, pfbbf_ref.k_sums(pfbbf_ref.beams(ys[:2], w_null), K), ys[:2], w_null, k, K)
    zs = engine.pfbbf(iqs, w_steer, k, taps, hop=D, layout="time", nframes=K)
    rv = pfbbf_ref.voltage_ratio(zs, pfbbf_ref.beams(ys, w_steer), ys, w_steer, k)
    gain, depth = pfbbf_ref.delay_figures(steer[0], null[0])
    print("steered gain over one element %.4f, null depth %.6f; ratios to the bounds: steered %.4f, nulled %.4f, voltages %.4f"
          % (gain, depth, rs, rn, rv))
    assert rs <= 1.0 and rn <= 1.0 and rv <= 1.0
    assert gain >= pfbbf_ref.STEER_GAIN_MIN
    assert depth <= pfbbf_ref.NULL_DEPTH_MAX
