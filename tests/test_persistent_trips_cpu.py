"""tests/persistent_trips.py against its own conditions and against hand-computed launches (no GPU, no build)."""
import pytest

import kernel_matrix as km
import persistent_trips as pt


def test_pool_map_meets_its_conditions_for_every_grid():
    for blocks in range(1, 513):
        rows = pt.rows_for(blocks)
        assert rows == 2 * blocks + 19
        pm = pt.pool_map(blocks, rows)
        pt.check_pool_map(pm, blocks, rows, 4)              # (pool_map asserts this itself: here on its result)
        assert blocks % 4 or set(pm) == {0, 1, 2, 3}, blocks
        # three trips for the first 19 workgroups, two for the rest
        trips = [len(range(b, rows, blocks)) for b in range(blocks)]
        assert max(trips) >= 3 and min(trips) >= 2
        if blocks >= 19:
            assert trips == [3] * 19 + [2] * (blocks - 19)
    for blocks in range(4, 400, 4):                         # the closed form where it is promised
        rows = pt.rows_for(blocks)
        assert pt.pool_map(blocks, rows) == [(g + 2 * (g // blocks)) % 4 for g in range(rows)]
    for blocks in (1, 2, 3, 5, 7, 21, 41, 101, 255):        # five entries work as well
        pt.check_pool_map(pt.pool_map(blocks, pt.rows_for(blocks), 5), blocks, pt.rows_for(blocks), 5)


def test_check_pool_map_refuses_the_maps_that_would_hide_a_wrong_row():
    blocks, rows = 8, pt.rows_for(8)
    for bad in ([0] * rows,                                      # every row alike
                [g % 4 for g in range(rows)],                   # g + blocks looks like g
                [(g % blocks + g // blocks) % 4 for g in range(rows)]):   # g + blocks looks like g + 1
        with pytest.raises(AssertionError):
            pt.check_pool_map(bad, blocks, rows, 4)


@pytest.mark.parametrize("blocks", [64, 104, 256, 304])
def test_x8_pool_map_gives_a_workgroup_pairwise_different_rows(blocks):
    rows = pt.x8_rows_for(blocks)
    assert rows == 9 * blocks + 19
    pm, P = pt.x8_pool_map(blocks, rows)
    assert P == 10 and len(pm) == rows and set(pm) == set(range(P))
    for b in range(blocks):
        own = [pm[g] for g in range(b, rows, blocks)]
        assert len(own) > pt.X_STATIC_ROWS and len(set(own)) == len(own)
    assert all(pm[g] != pm[g + 1] for g in range(rows - 1))


# launch_cic_block_sums by hand, at cus = 256 and n = 1 000 000 outputs (15 625 pieces):
#   R     chunk   slice   G   rounds = ceil(15625 / G)   cap           blocks = min(ceil(rounds / 4), cap)
HAND = {
    2: (256, 8192, 32, 489, 1024, 123),
    3: (384, 8192, 21, 745, 1024, 187),
    10: (1280, 8192, 6, 2605, 1024, 652),
    12: (1536, 8192, 5, 3125, 1024, 782),
    21: (2688, 8192, 3, 5209, 1024, 1024),
    64: (8192, 8192, 1, 15625, 1024, 1024),
    65: (8320, 16384, 1, 15625, 512, 512),
    128: (16384, 16384, 1, 15625, 512, 512),
}


@pytest.mark.parametrize("R", sorted(HAND))
def test_cic_launch_agrees_with_the_hand_computed_launch(R):
    assert tuple(pt.cic_launch(R, 1000000, 256)) == HAND[R]
    L = pt.cic_launch(R, 1000000, 304)
    assert L.cap == 304 * (2 if R > 64 else 4) and L[:4] == HAND[R][:4]
    assert pt.cic_launch(R, 1, 256).blocks == 1              # no whole piece: one workgroup for the tail


@pytest.mark.parametrize("cus", [64, 104, 256, 304])
@pytest.mark.parametrize("R", sorted(HAND))
def test_cic_len_takes_every_wavefront_past_its_first_round(R, cus):
    n = pt.cic_len(R, cus)
    L = pt.cic_launch(R, n, cus)
    assert L.blocks == L.cap
    per_wave = pt.cic_wave_rounds(R, n, cus)
    assert len(per_wave) == 4 * L.cap and min(per_wave) >= 2 and max(per_wave) == 3
    pieces = n // 64
    full = pieces // L.G
    assert full == 2 * 4 * L.cap + 7
    assert pieces - full * L.G == (1 if L.G > 1 else 0) and n - 64 * pieces == 37
    # seven wavefronts reuse their slice twice; where G > 1 the eighth's third round is the short one
    assert per_wave.count(3) == (8 if L.G > 1 else 7)
    if cus == 256:
        assert 2 * R * n < 69e6                              # bytes of input: a slice per wavefront and trip at most


def test_stride_len():
    for cus in (64, 256, 304):
        n = pt.stride_len(cus)
        stride = cus * 8 * 256
        assert n == 2 * stride + 1317 and 2 * stride < n < 3 * stride and n % 256


def test_every_persistent_case_is_selected():
    names = {km.instantiation(c)[0] for c in km.CASES}
    assert names == set(pt.PERSISTENT) | {"spectra_direct", "spectra_f64"}
    # against the model: one case per persistent instantiation
    inst = {km.instantiation(c) for c in km.CASES if km.instantiation(c)[0] in pt.PERSISTENT}
    assert len(pt.CASES) == len(inst) == len({km.instantiation(c) for c in pt.CASES})
    assert len(pt.CASES) == len(km.CASES) - sum(1 for c in km.CASES
                                                 if km.instantiation(c)[0] in ("spectra_direct", "spectra_f64"))
    assert pt.FAMILIES == [f for f in km.FAMILIES if f.rsplit("-", 1)[0] in pt.PERSISTENT]
    assert sum(1 for c in pt.CASES if pt.is_x8(c)) == 7 and all(c.f64 for c in pt.CASES if pt.is_x8(c))
    for c in pt.CASES:
        assert pt.pin_option(c) == (("f64_blocks_per_cu", 1) if c.f64 else ("blocks_per_cu", 1))
        assert dict(c.opts).get(pt.pin_option(c)[0]) is None     # no case sets the option the test pins
