"""include/rtlws_dedisp.h restated in numpy: the sum in the header's order as f32 vectors, the same sum in f64 with the
bound that sequential f32 summation keeps against it, the delay formula in numpy.float64, and the inputs and tables the
two suites share (tests/test_dedisp_cpu.py, tests/test_dedisp_gpu.py).  Nothing here touches the library."""
import numpy as np

from helpers import hash_bytes

MIN_NCHAN, MAX_NCHAN, MAX_TRIALS, MAX_DELAY = 4, 4096, 4096, 65535
KDM = 4.148808e3          # s MHz^2 cm^3 / pc

# rtlws_dedisp_delays' arguments behind nchan: (nchan, shifted, f_centre_hz, bandwidth_hz, row_seconds, ntrials, dm0,
# dm_step) and the largest delay each gives
DELAY_SETS = ((1024, 1, 408e6, 2.4e6, 2048 / 2.4e6, 64, 0.0, 0.5),
              (16, 0, 1420.4e6, 2.0e6, 1e-4, 7, 10.0, 25.0),
              (64, 1, 151e6, 2.4e6, 512 / 2.4e6, 33, 0.0, 1.0),
              (4096, 0, 611e6, 20e6, 16384 / 20e6, 256, 0.0, 2.0))
LARGEST_DELAYS = (11, 9, 854, 453)


def rows_needed(delays, mask, nout):
    """nout + the largest delay over the positions the mask keeps; 0 for nout == 0"""
    delays = np.asarray(delays)
    keep = np.ones(delays.shape[1], bool) if mask is None else np.asarray(mask) != 0
    most = int(delays[:, keep].max()) if keep.any() else 0
    return nout + most if nout else 0


def dedisp_ref(rows, delays, mask=None, nout=None):
    """D[t][n] of the header, float32 [ntrials, nout]: one f32 accumulator per output, positions ascending, each step one
    f32 addition of a vector of delayed columns.  rows float32 [nrows, >= nchan]."""
    return _sums(np.asarray(rows, np.float32), delays, mask, nout, np.float32)


def dedisp_f64(rows, delays, mask=None, nout=None):
    """The same sums in f64"""
    return _sums(np.asarray(rows, np.float32), delays, mask, nout, np.float64)


def dedisp_both(rows, delays, mask=None, nout=None):
    """(dedisp_ref, dedisp_f64) of the same arguments, each term fetched once"""
    return _sums(np.asarray(rows, np.float32), delays, mask, nout, np.float32, np.float64)


def _sums(rows, delays, mask, nout, *dtypes):
    delays = np.asarray(delays, np.int64)
    ntrials, nchan = delays.shape
    if nout is None:
        nout = rows.shape[0] - (rows_needed(delays, mask, 1) - 1)
    accs = [np.zeros((ntrials, nout), dtype) for dtype in dtypes]
    n = np.arange(nout)[None, :]
    for i in range(nchan):
        if mask is not None and not mask[i]:
            continue
        term = rows[delays[:, i][:, None] + n, i]
        accs = [acc + term.astype(acc.dtype) for acc in accs]
    return accs[0] if len(accs) == 1 else tuple(accs)


def bound(rows, delays, mask=None, nout=None):
    """|D - D64| <= M 2^-24 sum |terms|: M - 1 additions, each within 2^-24 of its exact result, which the sum of the
    magnitudes bounds (sequential summation, first order; the factor M for M - 1 pays the second)"""
    return delays.shape[1] * 2.0 ** -24 * dedisp_f64(np.abs(rows), delays, mask, nout)


def frequencies_mhz(nchan, shifted, f_centre_hz, bandwidth_hz):
    """nu_i of the header in MHz, float64 [nchan]"""
    i = np.arange(nchan)
    c = (i + nchan // 2) % nchan if shifted else i
    return (np.float64(f_centre_hz) + np.where(c < nchan // 2, c, c - nchan).astype(np.float64) * np.float64(bandwidth_hz)
            / np.float64(nchan)) / np.float64(1e6)


def delay_quotients(nchan, shifted, f_centre_hz, bandwidth_hz, row_seconds, ntrials, dm0, dm_step):
    """What rtlws_dedisp_delays rounds, float64 [ntrials, nchan]"""
    nu = frequencies_mhz(nchan, shifted, f_centre_hz, bandwidth_hz)
    excess = 1.0 / (nu * nu) - 1.0 / (nu.max() * nu.max())
    dm = np.float64(dm0) + np.arange(ntrials, dtype=np.float64) * np.float64(dm_step)
    return np.float64(KDM) * dm[:, None] * excess[None, :] / np.float64(row_seconds)


def delays(*args):
    return np.rint(delay_quotients(*args)).astype(np.int32)


# ---- what the suites share ----

def _hashed_bits(nrows, width, seed):
    """(the bit patterns of hashed_rows, the one hash bit they leave unused), uint32 [nrows, width] each"""
    b = hash_bytes(4 * nrows * width, seed).astype(np.uint32).reshape(nrows, width, 4)
    mant = (b[..., 0] << np.uint32(15)) | (b[..., 1] << np.uint32(7)) | (b[..., 2] >> np.uint32(1))
    return ((np.uint32(117) + b[..., 3] % np.uint32(20)) << np.uint32(23)) | mant, b[..., 2] & np.uint32(1)


def hashed_rows(nrows, width, seed):
    """float32 [nrows, width], non-negative, from the counter hash: 23 bits of mantissa and one of 20 binades each, so
    that the order of a sum's additions shows in its bits"""
    return _hashed_bits(nrows, width, seed)[0].view(np.float32)


def signed_rows(nrows, width, seed):
    """hashed_rows with the sign from a further bit of the hash: terms cancel, and the f64 bound is on the magnitudes"""
    bits, sign = _hashed_bits(nrows, width, seed)
    return (bits | (sign << np.uint32(31))).view(np.float32)


NEG_ZERO, POS_INF, NEG_INF, QUIET_NAN = (np.uint32(x) for x in (0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000))


def special_rows(nrows, width, seed):
    """signed_rows (width even, at least 8) with what a sum of ordinary floats never meets, planted by the row: row j
    draws a hash h and two different even positions a < b, and by h % 16 becomes
      0   a cancelling row: every odd position holds the negative of the even one before it, so that the row's sum in
          the header's order is +0 exactly;
      1   subnormal throughout: every value keeps its sign and mantissa (bit patterns 1 .. 0x7FFFFF) and loses its exponent;
      2   a cancelling row before a and subnormal from a on: the row's sum is the sum of its subnormals;
      3   zeros throughout, -0.0 where the value was negative;
      4   a cancelling row whose pair at a is -0.0 twice;
      5   +Inf at a;    6  -Inf at b;    7  +Inf at a and -Inf at b;    8  a quiet NaN at a;
      9   -0.0 at a and a subnormal at b among ordinary values (neither shows in a sum: they must not);
      10 .. 15 as signed_rows left it.
    A table that delays one position further than the rest of the row mixes the rows: an output takes that position
    from another row than the rest, so that a subnormal row shows only where the other row is subnormal or zero there."""
    assert width % 2 == 0 and width >= 8
    bits = signed_rows(nrows, width, seed).view(np.uint32).copy()
    h = hashed_ints(2 * nrows, (1 << 24) - 1, seed + 4099).astype(np.int64).reshape(nrows, 2)
    kind = h[:, 0] % 16
    pa = 2 * (h[:, 1] % (width // 2 - 1))                                          # even, below width - 2
    pb = pa + 2 + 2 * ((h[:, 1] >> 12) % ((width - 2 - pa) // 2))                  # even, pa < pb <= width - 2
    i = np.arange(width)[None, :]
    subnormal = (bits & np.uint32(0x807FFFFF)) | np.uint32(1)
    pairs = bits.copy()
    pairs[:, 1::2] = pairs[:, 0::2] ^ NEG_ZERO
    at_a, at_b = i == pa[:, None], i == pb[:, None]
    for k, where, values in ((0, i >= 0, pairs), (1, i >= 0, subnormal), (2, i >= 0, np.where(i < pa[:, None], pairs, subnormal)),
                             (3, i >= 0, bits & NEG_ZERO), (4, i >= 0, pairs), (4, at_a | (i == pa[:, None] + 1), NEG_ZERO),
                             (5, at_a, POS_INF), (6, at_b, NEG_INF), (7, at_a, POS_INF), (7, at_b, NEG_INF), (8, at_a, QUIET_NAN),
                             (9, at_a, NEG_ZERO), (9, at_b, subnormal)):
        bits = np.where((kind == k)[:, None] & where, values, bits)
    return bits.view(np.float32)


_POOL = {}


def pooled_rows(nrows, width, seed):
    """float32 [nrows, width] cut from one pool of 2^20 hashed floats, begun at a place the seed picks: the inputs of the
    larger cases, which need more values than it pays to hash one by one"""
    if "rows" not in _POOL:
        _POOL["rows"] = hashed_rows(1, 1 << 20, seed=77).reshape(-1)
    return np.resize(np.roll(_POOL["rows"], -7919 * seed), (nrows, width))


def hashed_ints(n, top, seed):
    """n integers 0 .. top from the counter hash"""
    b = hash_bytes(4 * n, seed).astype(np.int64).reshape(n, 4)
    return ((b[:, 0] << 24 | b[:, 1] << 16 | b[:, 2] << 8 | b[:, 3]) % (top + 1)).astype(np.int32)


def random_table(ntrials, nchan, maxd, seed):
    """int32 [ntrials, nchan] uniform in 0 .. maxd with both ends present among the first four positions of trial 0: a
    spread of maxd inside one unit of any plan"""
    d = hashed_ints(ntrials * nchan, maxd, seed).reshape(ntrials, nchan)
    d[0, 0], d[0, 1] = 0, maxd
    return d


def mixed_table(ntrials, nchan, seed):
    """The first eight trials a smooth sweep, the ones behind them random to 5000"""
    d = random_table(ntrials, nchan, 5000, seed)
    smooth = np.arange(min(8, ntrials))[:, None] * (nchan - 1 - np.arange(nchan))[None, :] // max(nchan // 8, 1)
    d[:smooth.shape[0]] = smooth
    return d


def random_mask(nchan, seed):
    m = (hash_bytes(nchan, seed) % 3 != 0).astype(np.uint8)
    m[seed % nchan] = 1
    return m


def one_kept(nchan, i):
    m = np.zeros(nchan, np.uint8)
    m[i] = 1
    return m
