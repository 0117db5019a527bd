"""Every instantiation of the polyphase family's five libraries, launched through the C ABI.

tests/pfb_family_matrix.py lists one case per template instantiation (133); tests/test_pfb_family_matrix_cpu.py holds
that list to the libraries' code objects.  Here each case runs on random bytes under random int16 taps and is held
  - as uint32, without a tolerance, to the definition's f32 arithmetic in the definition's order (tests/pfbbf_ref.py,
    tests/pfbxc_ref.py, tests/pfbsk_ref.py) of the channelizer's or the voltage run's own download, and to the sibling
    library's rows where the family promises them equal;
  - to the f64 restatement under the bound the project derives for the library (pfb_ref.bound, pfbspec_ref.bound,
    pfbxc_ref.bound, pfbbf_ref.bound and power_bound): a ratio <= 1.
No tolerance is new.  With B > 1 every beam is also held to the run of a one-beam plan with that beam's weights, which
ties each B to the B = 1 kernels that tests/test_pfbbf_gpu.py pins at every shape.  The voltage kernels run 2 F + 3
frames (three workgroups, the last one partly filled), the sum kernels 2 per + 1 spectra with per from the library's
own grid call; both hops, the half hop from first_frame_index 7.  At the end one line per library gives the worst
ratio to each bound."""
import zlib

import numpy as np
import pytest

import pfb_family_matrix as fm
import pfb_ksum_cases as ksum
import pfb_ref
import pfbbf_ref
import pfbxc_ref
from test_pfb_ksum_gpu import Rig, check_correlator, check_spectrometer, first_difference, frames64, u32
from test_pfbbf_gpu import Bank
from test_pfbsk_gpu import SkRig, check_sums_and_decisions

pytestmark = pytest.mark.gpu

NSUB = 3                                              # L of the kurtosis spectrometer's cases
FIRST_AT_THE_HALF_HOP = 7                             # odd: the sign rule is live
WORST = {}                                            # (library, bound) -> the worst ratio of the cases that ran
DECISIONS = {"flagged": 0, "kept": 0}                 # the kurtosis spectrometer's sub-integrations under the SK bounds


def note(lib, what, ratio):
    WORST[lib, what] = max(WORST.get((lib, what), 0.0), ratio)


@pytest.fixture(scope="module", autouse=True)
def summary():
    """After the module's last case: one line per library, the worst ratio to each of its bounds."""
    yield
    for lib in fm.LIBRARIES:
        mine = sorted((what, r) for (name, what), r in WORST.items() if name == lib)
        if mine:
            print("\n%s, %d instantiations, worst ratio to the bound: %s" % (lib, fm.COUNTS[lib], ", ".join("%s %.4f" % wr for wr in mine)), end="")
    if DECISIONS["flagged"] + DECISIONS["kept"]:
        print("\npfbsk, %d instantiations, every comparison as uint32: %d sub-integrations flagged, %d kept"
              % (fm.COUNTS["pfbsk"], DECISIONS["flagged"], DECISIONS["kept"]))


def seed_of(c):
    return zlib.crc32(c.label().encode()) & 0xFFFFFF


def sum_frames(k):
    """The frames of the longest sum run at log2 M = k: K (2 per + 1) over both K of the matrix.  One figure per log2 M,
    so that the cases of a log2 M share test_pfb_ksum_gpu.frames64's f64 frames."""
    return max(K * (2 * ksum.geometry(k, K)[1] + 1) for K in (fm.sum_k(k, False), fm.sum_k(k, True)))


def spectra(c, K, per):
    assert per == ksum.geometry(c.k, K)[1], (c.label(), K, per)
    return 2 * per + 1


# ---- the beamformer ---------------------------------------------------------------------------------------------------

def beamformer_banks(engine, built, c, nframes):
    """-> (the case's bank with its random weights up, W, a one-beam bank over the same captures or None, the captures)"""
    M, seed = 1 << c.k, seed_of(c)
    taps = pfb_ref.random_taps(c.k, c.T, seed=seed)
    iqs = pfbbf_ref.random_captures(c.A, pfb_ref.samples_needed(M, c.T, M, nframes), seed=seed + 1)
    bank = Bank(engine, built, c.k, taps, iqs, c.B, nframes)
    try:
        W = bank.weights(pfbbf_ref.random_weights(c.B, c.A, M, seed=seed + 2))
        solo = Bank(engine, built, c.k, taps, iqs, 1, nframes) if c.B > 1 else None
    except Exception:
        bank.close()
        raise
    return bank, W, solo, iqs, taps


def check_voltage(engine, built, c):
    M, F = 1 << c.k, fm.tile_frames(c.k)
    n = 2 * F + 3
    assert built.pfbbf_grid(c.k, c.T, M, 0, n)[1:5:3] == (3, F)          # three workgroups of F frames
    bank, W, solo, iqs, taps = beamformer_banks(engine, built, c, n)
    try:
        for D in (M, M // 2):
            first = FIRST_AT_THE_HALF_HOP if D != M else 0
            z = pfbbf_ref.beams_f32(bank.raw_frames(n, D), W)
            assert z.dtype == np.complex64 and z.shape == (c.B, n, M)
            assert np.all(np.any(z.real != 0, axis=2)) and np.all(np.any(z.imag != 0, axis=2))       # every frame of every beam
            want = pfbbf_ref.flip(z, M, D, first)
            got = bank.volts(n, D, first, "time")
            assert np.array_equal(u32(got), u32(want)), (D, "time", first_difference(got, want))
            got_c = bank.volts(n, D, first, "channel")
            assert np.array_equal(u32(got_c), u32(want.transpose(0, 2, 1))), (D, "channel", first_difference(got_c, want.transpose(0, 2, 1)))
            ys = pfbbf_ref.frames_of(iqs, c.k, taps, D, n)
            r = pfbbf_ref.voltage_ratio(got, pfbbf_ref.beams(ys, W) * pfbbf_ref.signs(M, D, first, n)[None], ys, W, c.k)
            note("pfbbf", "voltages", r)
            assert r <= 1.0, (D, r)
            for b in range(c.B if solo else 0):
                solo.weights(W[b:b + 1])
                assert np.array_equal(u32(solo.volts(n, D, first, "time")[0]), u32(got[b])), (D, b, "time")
                assert np.array_equal(u32(solo.volts(n, D, first, "channel")[0]), u32(got_c[b])), (D, b, "channel")
    finally:
        for x in (solo, bank):
            if x is not None:
                x.close()


def check_power(engine, built, c):
    M, K = 1 << c.k, c.K
    n = spectra(c, K, built.pfbbf_grid(c.k, c.T, M, K, 1)[4])
    nf = n * K
    bank, W, solo, iqs, taps = beamformer_banks(engine, built, c, nf)
    try:
        for D in (M, M // 2):
            z = bank.volts(nf, D, FIRST_AT_THE_HALF_HOP if D != M else 0, "time")
            want = pfbbf_ref.power_f32(z, c.k, K)
            assert want.shape == (n, c.B, M) and np.all(want > 0)
            got = bank.power(K, n, D)
            assert np.array_equal(u32(got), u32(want)), (D, first_difference(got, want))
            shifted = bank.power(K, n, D, shifted=True)
            assert np.array_equal(u32(shifted), u32(np.fft.fftshift(want, axes=2))), (D, "shifted")
            ys = pfbbf_ref.frames_of(iqs, c.k, taps, D, nf)
            r = pfbbf_ref.power_ratio(got, pfbbf_ref.k_sums(pfbbf_ref.beams(ys, W), K), ys, W, c.k, K)
            note("pfbbf", "powers", r)
            assert r <= 1.0, (D, r)
            for b in range(c.B if solo else 0):
                solo.weights(W[b:b + 1])
                assert np.array_equal(u32(solo.power(K, n, D)[:, 0]), u32(got[:, b])), (D, b)
    finally:
        for x in (solo, bank):
            if x is not None:
                x.close()


# ---- the libraries on one capture each, and the correlator ------------------------------------------------------------------

def check_channelizer(engine, built, c):
    """2 F + 3 frames in both layouts at both hops under pfb_ref.bound against pfb_ref.pfb_ref."""
    M, F = 1 << c.k, fm.tile_frames(c.k)
    n = 2 * F + 3
    rig = Rig(engine, built, c.k, 1, sum_frames(c.k), c.T)
    assert n <= rig.nframes
    try:
        for D in (M, M // 2):
            ref = frames64(c.k, D, 0, rig.nframes, c.T)[:n]
            nrm = np.linalg.norm(ref, axis=1)
            assert np.all(nrm > 0)
            got = rig.frames(0, n, D)
            rig.pfb_plan.run(rig.d_iqs[0], n, rig.d_tmp, hop=D, layout="channel")
            engine.sync()
            got_c = engine.download(rig.d_tmp, np.complex64, (M, n))
            assert np.array_equal(u32(got_c), u32(got.T)), (D, "channel", first_difference(got_c, got.T))
            r = float((np.linalg.norm(got.astype(np.complex128) - ref, axis=1) / (pfb_ref.bound(c.k) * nrm)).max())
            note("pfb", "frames", r)
            assert r <= 1.0, (D, r)
    finally:
        rig.close()


def check_spectrometer_case(engine, built, c):
    M = 1 << c.k
    todo = [(K, spectra(c, K, built.pfbspec_grid(c.k, c.T, M, K, 1)[4])) for K in fm.run_ks(c)]
    rig = Rig(engine, built, c.k, 1, sum_frames(c.k), c.T)
    try:
        for D in (M, M // 2):
            r = check_spectrometer(rig, c.k, D, todo, c.T)               # bits, the f64 bound, all-128; its rows > 0
            note("pfbspec", "rows", r)
    finally:
        rig.close()


def check_correlator_case(engine, built, c):
    M, A = 1 << c.k, c.A
    NX = len(pfbxc_ref.pairs(A))
    todo = [(K, spectra(c, K, built.pfbxc_grid(c.k, c.T, M, K, A, 1)[4])) for K in fm.run_ks(c)]
    nmax = max(n for _, n in todo)
    rig = Rig(engine, built, c.k, A, sum_frames(c.k), c.T)
    try:
        d_auto, d_cross = rig.alloc(nmax * A * M * 4), rig.alloc(nmax * NX * M * 8)
        plan = built.PfbXcPlan.open(engine, c.k, rig.taps, A)
        rig.plans.append(plan)
        for D in (M, M // 2):
            for K, n in todo:
                # autos = the spectrometer's rows, autos and crosses = the ordered f32 sums, under the f64 bounds
                ra, rc = check_correlator(rig, c.k, D, [(A, plan)], [(K, n)], d_auto, d_cross, c.T)
                note("pfbxc", "autos", ra)
                note("pfbxc", "crosses", rc)
                autos = engine.download(d_auto, np.float32, (n, A, M))  # that run's rows: nowhere zero
                cross = engine.download(d_cross, np.complex64, (n, NX, M))
                assert np.all(autos > 0) and np.all(np.any(cross.real != 0, axis=2)) and np.all(np.any(cross.imag != 0, axis=2)), (D, K)
    finally:
        rig.close()


def check_kurtosis(engine, built, c):
    M, K = 1 << c.k, c.K
    rc, _, _, _, per = built.pfbsk_grid(c.k, c.T, M, K, NSUB, 1)
    assert rc == 0
    n = 2 * per + 1
    longest = K * n * NSUB
    rig = SkRig(engine, built, c.k, longest, n, n * NSUB, c.T)
    try:
        for D in (M, M // 2):
            y = rig.frames(0, longest, D)
            d_mid = rig.upload(np.full((pfb_ref.samples_needed(M, c.T, D, longest), 2), 128, dtype=np.uint8))
            flagged, kept = check_sums_and_decisions(rig, built, c.k, K, NSUB, n, D, y, d_mid)
            DECISIONS["flagged"] += flagged
            DECISIONS["kept"] += kept
    finally:
        rig.close()


CHECKS = {"pfb": check_channelizer, "pfbspec": check_spectrometer_case, "pfbxc": check_correlator_case, "pfbsk": check_kurtosis}


@pytest.mark.parametrize("c", fm.CASES, ids=[c.label() for c in fm.CASES])
def test_every_instantiation(engine, built, c):
    check = CHECKS.get(c.lib) or (check_power if c.K else check_voltage)
    try:
        check(engine, built, c)
    except AssertionError as e:
        raise AssertionError("%s [%s]: %s" % (fm.spell(fm.instantiation(c)), c.label(), e)) from e
