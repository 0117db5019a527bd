"""GPU suite of include/rtlws_pfbxc.h, through the C ABI: the polyphase cross-correlator (every capture's tile of the
filter bank, multiplied and summed over K frames where the transform leaves it, one launch) against the spectrometer's
rows and the channelizer's own samples bit for bit, and against the numpy restatement tests/pfbxc_ref.py.

The accuracy criterion is derived, not measured (pfbxc_ref.bound): per cross row
sum_c |got - ref| <= (16 (log2 M + 1) + 2 K + 6) 2^-24 sqrt(||ref S_a||_1 ||ref S_b||_1); the auto rows keep
pfbspec_ref.bound."""
import numpy as np
import pytest

import pfb_ref
import pfbspec_ref
import pfbxc_ref

pytestmark = pytest.mark.gpu

NSPECTRA = (1, 2, 5)
MULTI_SHAPES = ((4, 7), (6, 8), (10, 4))                    # where A = 3 and 4 run
CASES = [(k, T, 2) for k, T in pfb_ref.SHAPES] + [(k, T, A) for k, T in MULTI_SHAPES for A in (3, 4)]
ORDER_SHAPES = [(4, 7), (6, 8), (8, 8), (10, 4)]


def k_list(F):
    return sorted({K for K in (1, 2, 3, F - 1, F, F + 1, 2 * F + 3) if K >= 1})


def u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


class Bank:
    """The captures of one (k, taps) on the device, uploaded once (a capture given twice: one buffer, its pointer
    twice), with the plans of the three libraries and output buffers for the longest run."""

    def __init__(self, engine, built, k, taps, iqs, max_frames, max_spectra):
        self.eng, self.k, self.M, self.A = engine, k, 1 << k, len(iqs)
        self.NX = self.A * (self.A - 1) // 2
        self.bufs = {}
        for x in iqs:
            if id(x) not in self.bufs:
                self.bufs[id(x)] = engine.upload(x)
        self.d_iqs = [self.bufs[id(x)] for x in iqs]
        self.xc_plan = built.PfbXcPlan.open(engine, k, taps, self.A)
        self.spec_plan = built.PfbSpecPlan.open(engine, k, taps)
        self.pfb_plan = built.PfbPlan.open(engine, k, taps)
        self.d_auto = engine.alloc(max_spectra * self.A * self.M * 4)
        self.d_cross = engine.alloc(max(max_spectra * self.NX, max_frames) * self.M * 8)

    def xc(self, K, n, D, shifted=False, first_sample=0, inputs=None, plan=None):
        """-> (float32 [n, A, M], complex64 [n, NX, M]); the captures from sample first_sample on."""
        d = self.d_iqs if inputs is None else [self.d_iqs[a] for a in inputs]
        A = len(d)
        NX = A * (A - 1) // 2
        assert (2 * first_sample) % 16 == 0
        (plan or self.xc_plan).run([b.ptr + 2 * first_sample for b in d], n, K, self.d_auto, self.d_cross, hop=D, shifted=shifted)
        self.eng.sync()
        return (self.eng.download(self.d_auto, np.float32, (n, A, self.M)),
                self.eng.download(self.d_cross, np.complex64, (n, NX, self.M)))

    def spec(self, a, K, n, D, shifted=False):
        """rtlws_pfbspec_run's raw sums of capture a -> float32 [n, M]"""
        self.spec_plan.run(self.d_iqs[a], n, K, self.d_cross, hop=D, shifted=shifted)
        self.eng.sync()
        return self.eng.download(self.d_cross, np.float32, (n, self.M))

    def frames(self, a, nframes, D):
        """rtlws_pfb_run's time-major samples of capture a, the sign rule applied -> complex64 [nframes, M]"""
        self.pfb_plan.run(self.d_iqs[a], nframes, self.d_cross, hop=D, layout="time")
        self.eng.sync()
        return self.eng.download(self.d_cross, np.complex64, (nframes, self.M))

    def close(self):
        for p in (self.xc_plan, self.spec_plan, self.pfb_plan):
            p.close()
        for b in list(self.bufs.values()) + [self.d_auto, self.d_cross]:
            b.free()


def random_captures(A, n, seed):
    return [pfb_ref.random_iq(n, seed=seed + 1000 * a) for a in range(A)]


@pytest.mark.parametrize("k,T,A", CASES)
def test_autos_are_the_spectrometer_bit_for_bit(engine, built, k, T, A):
    """Every auto row as uint32 against rtlws_pfbspec_run's RTLWS_OUT_POWER_SUM row of the same capture: both hops,
    both values of shifted, K across the tile's borders, nspectra that do and do not fill a workgroup."""
    M, F = 1 << k, 4096 >> k
    ks = k_list(F)
    longest = max(ks) * max(NSPECTRA)
    taps = pfb_ref.random_taps(k, T, seed=100 * k + T)
    iqs = random_captures(A, pfb_ref.samples_needed(M, T, M, longest), seed=k + T)
    bank = Bank(engine, built, k, taps, iqs, longest, max(NSPECTRA))
    try:
        for D in (M, M // 2):
            for shifted in (False, True):
                for K in ks:
                    for n in NSPECTRA:
                        autos, cross = bank.xc(K, n, D, shifted)
                        assert autos.shape == (n, A, M) and cross.shape == (n, A * (A - 1) // 2, M)
                        for a in range(A):
                            want = bank.spec(a, K, n, D, shifted)
                            assert np.all(want > 0)
                            assert np.array_equal(u32(autos[:, a]), u32(want)), (D, shifted, K, n, a)
    finally:
        bank.close()


@pytest.mark.parametrize("k,T,A", CASES)
def test_k1_crosses_are_the_channelizers_samples_multiplied_bit_for_bit(engine, built, k, T, A):
    """K = 1, unshifted: fl(+0 + fl(fl(ar br) + fl(ai bi))) and fl(+0 + fl(fl(ai br) - fl(ar bi))) of rtlws_pfb_run's
    time-major samples of the same captures (the sign rule applied: it reaches no product), formed in numpy f32 and
    compared as uint32: the transform, the table, the indexing and the conjugate are pinned with no tolerance."""
    M, F = 1 << k, 4096 >> k
    ns = (1, F - 1, F, F + 1, 2 * F + 3)
    taps = pfb_ref.random_taps(k, T, seed=100 * k + T)
    iqs = random_captures(A, pfb_ref.samples_needed(M, T, M, max(ns)), seed=3 * k + T)
    bank = Bank(engine, built, k, taps, iqs, max(ns), max(ns))
    zero = np.float32(0.0)
    try:
        for D in (M, M // 2):
            for n in ns:
                ys = [bank.frames(a, n, D) for a in range(A)]
                autos, cross = bank.xc(1, n, D)
                for x, (a, b) in enumerate(pfbxc_ref.pairs(A)):
                    re, im = pfbxc_ref.products_f32(ys[a], ys[b])
                    re, im = zero + re, zero + im
                    assert re.dtype == np.float32 and np.any(re != 0) and np.any(im != 0)
                    assert np.array_equal(u32(cross[:, x].real), u32(re)), (D, n, a, b)
                    assert np.array_equal(u32(cross[:, x].imag), u32(im)), (D, n, a, b)
                for a in range(A):
                    assert np.array_equal(u32(autos[:, a]), u32(zero + pfbxc_ref.products_f32(ys[a], ys[a])[0])), (D, n, a)
    finally:
        bank.close()


@pytest.mark.parametrize("k,T,A", CASES)
def test_k_sums_against_f64(engine, built, k, T, A):
    """Independent random bytes with random taps; 0/255 bytes with every tap 32767; copies of one noise capture
    delayed by 0, 1, 3, 6 samples plus noise of their own under the designed prototype, where every pair has a phase
    slope of its own kind: a wrong pair order, a swapped conjugate or a misplaced row falls far outside the bound
    (tests/test_pfbxc_cpu.py shows that on the restatement)."""
    M, F = 1 << k, 4096 >> k
    ks = k_list(F)
    longest = max(ks) * max(NSPECTRA)
    worst_c = worst_a = 0.0
    nmax = pfb_ref.samples_needed(M, T, M, longest)
    cases = (("random", random_captures(A, nmax, seed=k + T), pfb_ref.random_taps(k, T, seed=100 * k + T)),
             ("full scale", [pfb_ref.full_scale_iq(nmax, seed=k * T + a) for a in range(A)], np.full(T * M, 32767, np.int16)),
             ("delayed", pfbxc_ref.delayed_captures(A, nmax, seed=7 * k + T), pfbspec_ref.designed_taps(k, T)))
    for kind, iqs, taps in cases:
        bank = Bank(engine, built, k, taps, iqs, longest, max(NSPECTRA))
        try:
            for D in (M, M // 2):
                frames = pfbxc_ref.frames_of(iqs, k, taps, D, longest)      # a shorter run is a prefix: the same frames
                for K in ks:
                    ref_a, ref_c = pfbxc_ref.xc_sums(frames, K)
                    for n in NSPECTRA:
                        autos, cross = bank.xc(K, n, D)
                        ra = pfbxc_ref.auto_ratio(autos, ref_a[:n], k, K)
                        rc = pfbxc_ref.cross_ratio(cross, ref_a[:n], ref_c[:n], k, K)
                        worst_a, worst_c = max(worst_a, ra), max(worst_c, rc)
                        assert ra <= 1.0 and rc <= 1.0, (kind, D, K, n, ra, rc)
                # shifted rows are the same values in the other order
                K = ks[-1]
                autos, cross = bank.xc(K, 2, D)
                sh_a, sh_c = bank.xc(K, 2, D, shifted=True)
                assert np.array_equal(u32(sh_a), u32(np.fft.fftshift(autos, axes=2))), (kind, D)
                assert np.array_equal(sh_c.view(np.uint64), np.fft.fftshift(cross, axes=2).view(np.uint64)), (kind, D)
        finally:
            bank.close()
    print("M = %d, T = %d, A = %d: worst cross ratio to the bound %.4f, worst auto ratio %.4f (K = %s)" % (M, T, A, worst_c, worst_a, ks))


@pytest.mark.parametrize("k,T", ORDER_SHAPES)
def test_the_order_of_the_sum_knows_only_m_and_k(engine, built, k, T):
    """Two runs give the same bits; a run over the captures from sample j0 K D on gives rows j0 .. of the whole run;
    nspectra = 1 gives row 0 of a longer run; A = 2 against A = 3 with a third input added gives the same S_0, S_1 and
    V_01: the order does not know j, nspectra, the place in the grid or A."""
    M, F = 1 << k, 4096 >> k
    taps = pfb_ref.random_taps(k, T, seed=k)
    for K in (3, F + 1):
        per = built.pfbxc_grid(k, T, M, K, 2, 1)[4]
        n = 2 * per + 3                                        # three workgroups, the last one partly filled
        j0 = per // 2 + 1                                      # rows that change their place in the tile and in the grid
        iqs = random_captures(3, pfbxc_ref.samples_needed(M, T, M, K, n), seed=T + K)
        bank = Bank(engine, built, k, taps, iqs, n * K, n)
        two = built.PfbXcPlan.open(engine, k, taps, 2)
        try:
            for D in (M, M // 2):
                autos, cross = bank.xc(K, n, D)
                assert autos.shape == (n, 3, M) and np.all(autos > 0) and np.all(cross.real != 0) and np.all(cross.imag != 0)
                again_a, again_c = bank.xc(K, n, D)
                assert np.array_equal(u32(again_a), u32(autos)) and np.array_equal(again_c.view(np.uint64), cross.view(np.uint64)), (K, D)
                for start in (j0, n - 1):
                    part_a, part_c = bank.xc(K, n - start, D, first_sample=start * K * D)
                    assert np.array_equal(u32(part_a), u32(autos[start:])), (K, D, start)
                    assert np.array_equal(part_c.view(np.uint64), cross[start:].view(np.uint64)), (K, D, start)
                one_a, one_c = bank.xc(K, 1, D)
                assert np.array_equal(u32(one_a), u32(autos[:1])) and np.array_equal(one_c.view(np.uint64), cross[:1].view(np.uint64))
                for pair, x in (((0, 1), 0), ((0, 2), 1), ((1, 2), 2)):
                    a2, c2 = bank.xc(K, n, D, inputs=pair, plan=two)
                    assert a2.shape == (n, 2, M) and c2.shape == (n, 1, M)
                    assert np.array_equal(u32(a2), u32(autos[:, list(pair)])), (K, D, pair)
                    assert np.array_equal(c2[:, 0].view(np.uint64), np.ascontiguousarray(cross[:, x]).view(np.uint64)), (K, D, pair)
        finally:
            two.close()
            bank.close()


@pytest.mark.parametrize("k,T", MULTI_SHAPES)
def test_degenerate_inputs(engine, built, k, T):
    """The same pointer twice: the pair's re row is the auto row as uint32 and its im row is all +0 bits.  One input all
    128: its auto row and all its cross rows are +0 bits, the other autos and the other pair untouched."""
    M, F = 1 << k, 4096 >> k
    ks = (1, 3, F + 1)
    n = 3
    taps = pfb_ref.random_taps(k, T, seed=5 * k)
    nmax = pfb_ref.samples_needed(M, T, M, max(ks) * n)
    x, y = random_captures(2, nmax, seed=k)
    mid = np.full((nmax, 2), 128, dtype=np.uint8)
    same = Bank(engine, built, k, taps, [x, y, x], max(ks) * n, n)
    dead = Bank(engine, built, k, taps, [x, mid, y], max(ks) * n, n)
    try:
        assert same.d_iqs[0] is same.d_iqs[2]
        for D in (M, M // 2):
            for K in ks:
                for shifted in (False, True):
                    autos, cross = same.xc(K, n, D, shifted)
                    assert np.all(autos > 0)
                    assert np.array_equal(u32(cross[:, 1].real), u32(autos[:, 0])), (D, K)
                    assert np.array_equal(u32(autos[:, 2]), u32(autos[:, 0]))
                    assert not u32(cross[:, 1].imag).any(), (D, K)
                    assert np.any(cross[:, 0].imag != 0) and np.any(cross[:, 2].imag != 0)
                    # (0,1) and (1,2) = (y, x) are conjugates of each other, exactly
                    assert np.array_equal(u32(cross[:, 2].real), u32(cross[:, 0].real))
                    assert np.array_equal(cross[:, 2].imag, -cross[:, 0].imag)

                    d_a, d_c = dead.xc(K, n, D, shifted)
                    assert not u32(d_a[:, 1]).any() and not d_c[:, 0].view(np.uint64).any() and not d_c[:, 2].view(np.uint64).any(), (D, K)
                    assert np.array_equal(u32(d_a[:, 0]), u32(autos[:, 0])) and np.array_equal(u32(d_a[:, 2]), u32(autos[:, 1]))
                    assert np.array_equal(d_c[:, 1].view(np.uint64), np.ascontiguousarray(cross[:, 0]).view(np.uint64))
    finally:
        same.close()
        dead.close()


def test_strides_and_nothing_outside_the_rows(engine, built):
    k, T, K, A = 5, 3, 3, 3
    M, NX = 1 << k, 3
    per = built.pfbxc_grid(k, T, M, K, A, 1)[4]
    n = per + 3                                                # two workgroups, the second partly filled
    taps = pfb_ref.random_taps(k, T, seed=21)
    plan = built.PfbXcPlan.open(engine, k, taps, A)
    sentinel = np.float32(-12345.5)
    astride, cstride, tail = M + 4, M + 2, 64
    for D in (M, M // 2):
        iqs = random_captures(A, pfbxc_ref.samples_needed(M, T, D, K, n), seed=22)
        ref_a, ref_c = pfbxc_ref.pfbxc_ref(iqs, k, taps, K, D)
        d_iqs = [engine.upload(x) for x in iqs]
        na, nc = n * A * astride + tail, 2 * (n * NX * cstride + tail)
        d_auto = engine.upload(np.full(na, sentinel, dtype=np.float32))
        d_cross = engine.upload(np.full(nc, sentinel, dtype=np.float32))
        plan.run(d_iqs, n, K, d_auto, d_cross, hop=D, auto_stride=astride, cross_stride=cstride)
        engine.sync()
        out_a = engine.download(d_auto, np.float32, (na,))
        out_c = engine.download(d_cross, np.float32, (nc,))
        body_a = out_a[:n * A * astride].reshape(n, A, astride)
        body_c = out_c[:2 * n * NX * cstride].reshape(n, NX, cstride, 2)
        got_c = body_c[:, :, :M, 0] + 1j * body_c[:, :, :M, 1]
        assert pfbxc_ref.auto_ratio(body_a[:, :, :M], ref_a, k, K) <= 1.0, D
        assert pfbxc_ref.cross_ratio(got_c, ref_a, ref_c, k, K) <= 1.0, D
        assert np.all(body_a[:, :, M:] == sentinel) and np.all(out_a[n * A * astride:] == sentinel), D
        assert np.all(body_c[:, :, M:] == sentinel) and np.all(out_c[2 * n * NX * cstride:] == sentinel), D
        # no spectra: nothing happens; with a device the refusals still hold and write nothing
        args = dict(hop=D, auto_stride=astride, cross_stride=cstride)
        assert plan.run(d_iqs, 0, K, d_auto, d_cross, **args) == 0
        for kw, word in (({"hop": M // 4}, "hop"), ({"hop": 2 * M}, "hop"), ({"auto_stride": 16}, "auto_stride must be >= M"),
                         ({"auto_stride": astride + 2}, "auto_stride must be a multiple of 4"),
                         ({"cross_stride": 16}, "cross_stride must be >= M"),
                         ({"cross_stride": cstride + 1}, "cross_stride must be a multiple of 2"), ({"shifted": 2}, "shifted")):
            a = dict(args)
            a.update(kw)
            assert plan.run(d_iqs, n, K, d_auto, d_cross, check=False, **a) == -1 and word in built.pfbxc_last_error(), kw
        for bad_iqs, word in (([d_iqs[0], None, d_iqs[2]], "null pointer"), ([d_iqs[0], d_iqs[1], d_iqs[2].ptr + 8], "16-byte"),
                              (None, "null pointer")):
            assert plan.run(bad_iqs, n, K, d_auto, d_cross, check=False, **args) == -1 and word in built.pfbxc_last_error(), word
        assert plan.run(d_iqs, n, 0, d_auto, d_cross, check=False, **args) == -1 and "k_avg" in built.pfbxc_last_error()
        assert plan.run(d_iqs, n, K, d_auto.ptr + 8, d_cross, check=False, **args) == -1 and "16-byte" in built.pfbxc_last_error()
        assert plan.run(d_iqs, n, K, d_auto, d_cross.ptr + 8, check=False, **args) == -1 and "16-byte" in built.pfbxc_last_error()
        assert plan.run(d_iqs, -1, K, d_auto, d_cross, check=False, **args) == -1 and "nspectra" in built.pfbxc_last_error()
        engine.sync()
        assert np.array_equal(u32(engine.download(d_auto, np.float32, (na,))), u32(out_a))
        assert np.array_equal(u32(engine.download(d_cross, np.float32, (nc,))), u32(out_c))
        for b in d_iqs + [d_auto, d_cross]:
            b.free()
    plan.close()


def test_capture_and_replay(built):
    """A run is one kernel launch: captured on a side stream the way tests/test_pfbspec_gpu.py captures the
    spectrometer, replayed on the first inputs and again on fresh ones in the same buffers, identical to eager
    launches."""
    import torch
    dev = torch.device("cuda", 0)
    eng = built.Engine(0)
    k, T, K, A = 6, 4, 5, 2
    M, D = 1 << k, 1 << (k - 1)
    n = built.pfbxc_grid(k, T, D, K, A, 1)[4] + 5
    taps = pfb_ref.random_taps(k, T, seed=31)
    plan = built.PfbXcPlan.open(eng, k, taps, A)
    ns = pfbxc_ref.samples_needed(M, T, D, K, n)
    first_host, fresh_host = random_captures(A, ns, seed=32), random_captures(A, ns, seed=33)
    iqs = [torch.from_numpy(x).to(dev) for x in first_host]
    autos = torch.zeros((n, A, M), dtype=torch.float32, device=dev)
    cross = torch.zeros((n, 1, M, 2), dtype=torch.float32, device=dev)

    def launch(a, c):
        plan.run([x.data_ptr() for x in iqs], n, K, a.data_ptr(), c.data_ptr(), hop=D, shifted=True, stream=built.torch_stream_handle())

    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            launch(autos, cross)
    torch.cuda.current_stream().wait_stream(side)
    assert float(autos.abs().sum()) == 0.0 and float(cross.abs().sum()) == 0.0      # capture enqueued nothing
    for host in (first_host, fresh_host):
        for x, h in zip(iqs, host):
            x.copy_(torch.from_numpy(h))
        autos.zero_()
        cross.zero_()
        g.replay()
        torch.cuda.synchronize()
        eager_a, eager_c = torch.zeros_like(autos), torch.zeros_like(cross)
        launch(eager_a, eager_c)
        torch.cuda.synchronize()
        assert torch.equal(autos, eager_a) and torch.equal(cross, eager_c)
        ref_a, ref_c = pfbxc_ref.pfbxc_ref(host, k, taps, K, D, shifted=True)
        c = cross.cpu().numpy()
        assert pfbxc_ref.auto_ratio(autos.cpu().numpy(), ref_a, k, K) <= 1.0
        assert pfbxc_ref.cross_ratio(c[..., 0] + 1j * c[..., 1], ref_a, ref_c, k, K) <= 1.0
    plan.close()
    eng.close()


def test_the_delay_case_on_the_device(engine, built):
    """pfbxc_ref.delay_case() through the library: capture b lags capture a by one sample, so the phase of V_01[c] is
    +2 pi c_signed / 64 and the coherence near 1, at both hops."""
    for hop_div in (1, 2):
        k, taps, D, K, iqs = pfbxc_ref.delay_case(hop_div)
        autos, cross = engine.pfbxc(iqs, k, taps, K, hop=D, nspectra=1)
        assert autos.shape == (1, 2, 64) and cross.shape == (1, 1, 64) and cross.dtype == np.complex64
        dev, coh = pfbxc_ref.delay_figures(cross[0, 0], autos[0, 0], autos[0, 1])
        print("hop M / %d: phase within %.4f rad, coherence >= %.5f" % (hop_div, dev, coh))
        assert dev <= 0.02
        assert coh >= 0.99
