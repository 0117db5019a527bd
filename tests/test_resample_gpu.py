"""GPU parity for the decimators: bit-exact against the reference-object-code
goldens (tests/golden/*_ref.npz) and against the oracle on fresh inputs."""
import numpy as np
import pytest

import persistent_trips as pt
from conftest import golden

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("R", [8, 10, 12])
def test_cic_golden_chained_calls(built, R):
    g = golden("cic_ref.npz")
    src, cuts = g[f"R{R}_src"], g[f"R{R}_cuts"]
    st, outs = None, []
    for a, b in zip(cuts[:-1], cuts[1:]):
        rc, dst, st = built.cic_decimate(R, src[a:b], state=st)
        assert rc == 0
        outs.append(dst)
    assert np.array_equal(np.concatenate(outs), g[f"R{R}_dst"])
    assert np.array_equal(st, g[f"R{R}_state"])


def test_cic_golden_state_cases(built):
    g = golden("cic_ref.npz")
    rc, dst, st = built.cic_decimate(8, g["odd_src"], state=g["odd_state0"])
    assert rc == 0 and np.array_equal(dst, g["odd_dst"]) and np.array_equal(st, g["odd_state1"])
    rc, dst, st = built.cic_decimate(8, g["wrap_src"], state=g["wrap_state0"])
    assert rc == 0 and np.array_equal(dst, g["wrap_dst"]) and np.array_equal(st, g["wrap_state1"])
    rc, _, _ = built.cic_decimate(8, g["wrap_src"][:63], dst_len=8)
    assert rc == int(g["mismatch_rc"]) == -1


@pytest.mark.parametrize("R", [1, 2, 3, 7, 8, 10, 12, 16, 100])
def test_cic_vs_oracle(built, oracle, R):
    rng = np.random.default_rng(R)
    src = rng.integers(0, 256, size=(R * 1000 + 0, 2), dtype=np.uint8)
    rc, dst, st = built.cic_decimate(R, src)
    rc2, dst2, st2 = oracle.cic_decimate(R, src)
    assert rc == rc2 == 0
    assert np.array_equal(dst, dst2) and np.array_equal(st, st2)


def test_cic_large_block_sums(engine, oracle):
    """2^20 outputs at R=8 straight through the batch entry point."""
    rng = np.random.default_rng(0)
    n = 1 << 20
    src = rng.integers(0, 256, size=(n * 8, 2), dtype=np.uint8)
    d_src = engine.upload(src)
    d_dst = engine.alloc(n * 8)
    engine.cic_block_sums(8, d_src, n, d_dst)
    got = engine.download(d_dst, np.int32, (n, 2))
    want = (src.astype(np.int32) - 128).reshape(n, 8, 2).sum(axis=1)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("R", [1, 2, 3, 5, 9, 10, 12, 16, 25, 63, 64, 65, 127, 128])
def test_cic_block_sums_every_shape(engine, R):
    """Batch entry point: lengths around the 64-output piece and around a
    wavefront's round of pieces, every alignment class of R (odd R has a
    half-wavefront tail copy and masked half dwords; R > 64 the larger slice)."""
    rng = np.random.default_rng(1000 + R)
    per_round = 64 * max(1, (8192 if R <= 64 else 16384) // (128 * R))
    for n in (1, 63, 64, 65, per_round - 1, per_round + 64, 4 * per_round * 5 + 17, 40000):
        src = rng.integers(0, 256, size=(n * R, 2), dtype=np.uint8)
        d_src = engine.upload(src)
        d_dst = engine.alloc(n * 8)
        engine.cic_block_sums(R, d_src, n, d_dst)
        got = engine.download(d_dst, np.int32, (n, 2))
        want = (src.astype(np.int32) - 128).reshape(n, R, 2).sum(axis=1)
        assert np.array_equal(got, want), (R, n)


def _first_wrong_output(got, want, G):
    """Empty where got is want, else the first wrong output as (round, piece within the round, lane)."""
    neq = (got != want).any(axis=1)
    if not neq.any():
        return ""
    m = int(np.argmax(neq))
    piece, lane = divmod(m, 64)
    where = "round %d, piece %d, lane %d" % (piece // G, piece % G, lane) if piece < got.shape[0] // 64 else "tail lane %d" % lane
    return "%d outputs wrong, first %d (%s): %s, want %s" % (neq.sum(), m, where, got[m], want[m])


@pytest.mark.parametrize("R", [2, 3, 10, 12, 21, 64, 65, 128])
def test_cic_block_sums_past_the_grid_cap(engine, R):
    """cicr_kernel past its cap of workgroups (tests/persistent_trips.py, cic_len): every wavefront runs a second round
    in the LDS slice of its first, seven a third, then comes a round of fewer pieces than a slice holds (where it holds
    more than one) and a tail that fills no piece.  Random bytes; the piece in the first slot of a wavefront's slice
    is all 0 on the wavefront's first round and all 255 on its second, so a slice read before its copy has landed, or
    overwritten before it was read, shows in every lane."""
    cus = engine.get_option("cu_count")
    n = pt.cic_len(R, cus)
    L = pt.cic_launch(R, n, cus)
    per_wave = pt.cic_wave_rounds(R, n, cus)
    assert L.blocks == L.cap and min(per_wave) >= 2 and max(per_wave) == 3, (L, min(per_wave), max(per_wave))
    rng = np.random.default_rng(2000 + R)
    src = rng.integers(0, 256, size=(n * R, 2), dtype=np.uint8)
    pieces = src[:(n // 64) * 64 * R].reshape(n // 64, -1)               # a view: one row per piece
    first = np.arange(0, n // 64, L.G)                                    # the piece in slot 0 of every round
    trip = first // L.G // (4 * L.blocks)
    pieces[first[trip == 0]] = 0
    pieces[first[trip == 1]] = 255
    d_src = engine.upload(src)
    d_dst = engine.alloc(n * 8)
    engine.cic_block_sums(R, d_src, n, d_dst)
    got = engine.download(d_dst, np.int32, (n, 2))
    d_src.free()
    d_dst.free()
    want = (src.astype(np.int32) - 128).reshape(n, R, 2).sum(1)
    assert not _first_wrong_output(got, want, L.G), (R, n)


def test_cic8_block_sums_past_the_grid_cap(engine):
    """cic8_kernel's grid-stride loop: two whole trips of its capped grid, then a ragged third."""
    cus = engine.get_option("cu_count")
    n = pt.stride_len(cus)
    assert 2 * cus * 8 * 256 < n < 3 * cus * 8 * 256 and n % 256
    src = np.random.default_rng(2008).integers(0, 256, size=(n * 8, 2), dtype=np.uint8)
    d_src = engine.upload(src)
    d_dst = engine.alloc(n * 8)
    engine.cic_block_sums(8, d_src, n, d_dst)
    got = engine.download(d_dst, np.int32, (n, 2))
    want = (src.astype(np.int32) - 128).reshape(n, 8, 2).sum(1)
    assert not _first_wrong_output(got, want, 1), n


def test_cic_empty(built):
    rc, dst, st = built.cic_decimate(8, np.zeros((0, 2), dtype=np.uint8), state=[5, 6, 7, 8])
    assert rc == 0 and dst.shape[0] == 0 and list(st) == [5, 6, 7, 8]


def test_halfband_golden(built):
    g = golden("halfband_ref.npz")
    delay = np.zeros(10, dtype=np.float32)
    y1 = built.halfband_decimate(g["x"][:200], delay)
    assert np.array_equal(delay, g["delay_mid"])
    y2 = built.halfband_decimate(g["x"][200:], delay)
    assert np.array_equal(y1, g["y1"]) and np.array_equal(y2, g["y2"])      # bit-exact f32
    assert np.array_equal(delay, g["delay_end"])


def test_halfband_vs_oracle(built, oracle):
    rng = np.random.default_rng(4)
    x = rng.standard_normal(2 * 50000).astype(np.float32)
    d1 = rng.standard_normal(10).astype(np.float32)
    d2 = d1.copy()
    y = built.halfband_decimate(x, d1)
    y_ref = oracle.halfband_decimate(x, d2)
    assert np.array_equal(y, y_ref) and np.array_equal(d1, d2)


def test_halfband_past_the_grid_cap(engine, built, oracle):
    """halfband_kernel's grid-stride loop: two whole trips of its capped grid, then a ragged third; a non-zero delay
    line in, the delay line carried out."""
    cus = engine.get_option("cu_count")
    n = pt.stride_len(cus)
    assert 2 * cus * 8 * 256 < n < 3 * cus * 8 * 256 and n % 256
    rng = np.random.default_rng(44)
    x = rng.standard_normal(2 * n).astype(np.float32)
    d1 = rng.standard_normal(10).astype(np.float32)
    d2 = d1.copy()
    y = built.halfband_decimate(x, d1)
    y_ref = oracle.halfband_decimate(x, d2)
    bad = np.flatnonzero(y.view(np.uint32) != y_ref.view(np.uint32))
    assert bad.size == 0, "%d outputs differ, first %d (trip %d): %r, want %r" % (
        bad.size, bad[0], bad[0] // (cus * 8 * 256), y[bad[0]], y_ref[bad[0]])
    assert np.array_equal(d1, d2) and np.array_equal(d1, x[-10:])


def test_rf_decimator_golden(built):
    g = golden("rfdec_ref.npz")
    d = built.RfDecimator()
    rcs = [d.set_parameters(float(g["fs"]), int(g["R"]))]
    src, cuts = g["src"], g["cuts"]
    for a, b in zip(cuts[:-1], cuts[1:]):
        rcs.append(d.decimate(src[a:b]))
    assert rcs == list(g["rcs"])
    assert len(d.blocks) == g["blocks"].shape[0]
    assert np.array_equal(np.stack(d.blocks), g["blocks"])
    d.free()


def test_rf_decimator_unconfigured_and_bad_params(built):
    d = built.RfDecimator()
    assert d.decimate(np.zeros((10, 2), dtype=np.uint8)) == -1
    assert d.set_parameters(0.0, 8) == -1
    assert d.set_parameters(48000.0, 0) == -1
    assert d.set_parameters(48000.0, 8) == 0
    d.free()
