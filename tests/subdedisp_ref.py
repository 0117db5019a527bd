"""include/rtlws_subdedisp.h restated in numpy: the two chained sums in the header's order as f32 vectors, the same sums
in f64 with the bound that two chained sequential f32 sums keep against them, the sweep's tables in numpy.float64, and the
inputs the two suites share (tests/test_subdedisp_cpu.py, tests/test_subdedisp_gpu.py).  Nothing here touches the
library."""
import numpy as np

import dedisp_ref

MIN_NCHAN, MAX_NCHAN, MIN_PER_SUB, MAX_NOMINALS, MAX_TRIALS, MAX_DELAY = 4, 4096, 4, 4096, 4096, 65535
KDM = dedisp_ref.KDM

# rtlws_subdedisp_delays' arguments: (nchan, nsub, shifted, f_centre_hz, bandwidth_hz, row_seconds, ntrials, dm0, dm_step,
# per_nominal): both `shifted`, B = 1, a ragged last nominal, per_nominal = 1
DELAY_SETS = ((1024, 64, 1, 408e6, 2.4e6, 2048 / 2.4e6, 64, 0.0, 0.5, 16),
              (16, 1, 0, 1420.4e6, 2.0e6, 1e-4, 7, 10.0, 25.0, 3),
              (64, 4, 1, 151e6, 2.4e6, 512 / 2.4e6, 33, 0.0, 1.0, 8),
              (256, 16, 0, 611e6, 20e6, 1024 / 20e6, 40, 3.0, 2.0, 1),
              (64, 16, 0, 151e6, 2.4e6, 512 / 2.4e6, 21, 0.0, 1.5, 4))


def nominal_of(first, ntrials=None):
    """a(t), int [ntrials]"""
    first = np.asarray(first, np.int64)
    return np.searchsorted(first, np.arange(first[-1] if ntrials is None else ntrials), side="right") - 1


def kept_subbands(nchan, nsub, mask):
    """bool [nsub]: the subband keeps a position"""
    if mask is None:
        return np.ones(nsub, bool)
    return (np.asarray(mask).reshape(nsub, nchan // nsub) != 0).any(axis=1)


def maxima(d1, d2, mask=None):
    """(max_d1 over the kept positions, max_d2 over the subbands that keep one); 0 where nothing is kept"""
    d1, d2 = np.asarray(d1), np.asarray(d2)
    keep = np.ones(d1.shape[1], bool) if mask is None else np.asarray(mask) != 0
    keeps = kept_subbands(d1.shape[1], d2.shape[1], mask)
    return (int(d1[:, keep].max()) if keep.any() else 0), (int(d2[:, keeps].max()) if keeps.any() else 0)


def rows_needed(d1, d2, mask, nout):
    m1, m2 = maxima(d1, d2, mask)
    return nout + m2 + m1 if nout else 0


def mid_stride(d1, d2, mask, nout):
    return -(-(nout + maxima(d1, d2, mask)[1]) // 4) * 4 if nout else 0


def _stages(rows, first, d1, d2, mask, nout, *dtypes):
    """for each dtype (P [A, B, nmid], D [T, nout]) by the header's two recurrences"""
    d1, d2 = np.asarray(d1, np.int64), np.asarray(d2, np.int64)
    (A, M), (T, B) = d1.shape, d2.shape
    C = M // B
    m1, m2 = maxima(d1, d2, mask)
    if nout is None:
        nout = rows.shape[0] - m1 - m2
    nmid = nout + m2
    a_of = nominal_of(first, T)
    keeps = kept_subbands(M, B, mask)
    m = np.arange(nmid)[None, :]
    n = np.arange(nout)[None, :]
    got = []
    with np.errstate(invalid="ignore", over="ignore"):            # Inf - Inf and sums past the largest float are the definition's too
        for dtype in dtypes:
            P = np.zeros((A, B, nmid), dtype)
            for i in range(M):
                if mask is not None and not mask[i]:
                    continue
                P[:, i // C, :] = P[:, i // C, :] + rows[d1[:, i][:, None] + m, i].astype(dtype)
            D = np.zeros((T, nout), dtype)
            for s in range(B):
                if keeps[s]:
                    D = D + P[a_of[:, None], s, d2[:, s][:, None] + n]
            got.append((P, D))
    return got


def subdedisp_ref(rows, first, d1, d2, mask=None, nout=None, want_subbands=False):
    """D[t][n] of the header, float32 [ntrials, nout] (want_subbands: (D, P float32 [A, B, nmid])): one f32 accumulator per
    value, positions ascending inside a subband, then subbands ascending.  rows float32 [nrows, >= nchan]."""
    (P, D), = _stages(np.asarray(rows, np.float32), first, d1, d2, mask, nout, np.float32)
    return (D, P) if want_subbands else D


def subdedisp_both(rows, first, d1, d2, mask=None, nout=None):
    """(D in f32, P in f32, D in f64): the f64 sums are of the same terms"""
    (P, D), (_, D64) = _stages(np.asarray(rows, np.float32), first, d1, d2, mask, nout, np.float32, np.float64)
    return D, P, D64


def gamma(nchan, nsub):
    """gamma_k = k u / (1 - k u), u = 2^-24, k = C + B - 2: a term passes through at most C - 1 additions of its subband's
    sum and B - 1 of the trial's (the first addition of either, to +0.0, is exact), the standard bound of two chained
    recursive sums"""
    k, u = nchan // nsub + nsub - 2, 2.0 ** -24
    return k * u / (1.0 - k * u)


def bound(rows, first, d1, d2, mask=None, nout=None):
    """gamma * sum |terms|, float64 [ntrials, nout]"""
    d1, d2 = np.asarray(d1), np.asarray(d2)
    return gamma(d1.shape[1], d2.shape[1]) * _stages(np.abs(np.asarray(rows, np.float32)), first, d1, d2, mask, nout, np.float64)[0][1]


# ---- the sweep's tables ----

def sweep(nchan, nsub, shifted, f_centre_hz, bandwidth_hz, row_seconds, ntrials, dm0, dm_step, per_nominal):
    """What rtlws_subdedisp_delays rounds and gives, in numpy.float64: (first int32 [A + 1], the quotients of d1 [A, nchan],
    the quotients of d2 [ntrials, nsub], smear_rows)"""
    nu = dedisp_ref.frequencies_mhz(nchan, shifted, f_centre_hz, bandwidth_hz)
    x = 1.0 / (nu * nu) - 1.0 / (nu.max() * nu.max())
    C = nchan // nsub
    ref = np.array([s * C + int(np.argmin(x[s * C:(s + 1) * C])) for s in range(nsub)])
    A = -(-ntrials // per_nominal)
    first = np.minimum(np.arange(A + 1, dtype=np.int64) * per_nominal, ntrials)
    dm = np.float64(dm0) + np.arange(ntrials, dtype=np.float64) * np.float64(dm_step)
    dm_a = (dm[first[:-1]] + dm[first[1:] - 1]) / np.float64(2.0)
    dx = x - x[ref[np.arange(nchan) // C]]
    row = np.float64(row_seconds)
    q1 = np.float64(KDM) * dm_a[:, None] * dx[None, :] / row
    q2 = np.float64(KDM) * dm[:, None] * x[ref][None, :] / row
    a_of = nominal_of(first, ntrials)
    smear = (np.abs(dm - dm_a[a_of])[:, None] * np.float64(KDM) * dx[None, :] / row).max()
    return first.astype(np.int32), q1, q2, float(smear)


def tables(*args):
    """(first, d1, d2, smear_rows) of a sweep, as rtlws_subdedisp_delays gives them"""
    first, q1, q2, smear = sweep(*args)
    return first, np.rint(q1).astype(np.int32), np.rint(q2).astype(np.int32), smear


# ---- what the suites share ----

def even_first(ntrials, per):
    """first of nominals of `per` trials, the last one ragged"""
    return np.minimum(np.arange(-(-ntrials // per) + 1) * per, ntrials).astype(np.int32)


def random_tables(first, nchan, nsub, max1, max2, seed):
    """d1 int32 [A, nchan] uniform in 0 .. max1 and d2 int32 [T, nsub] uniform in 0 .. max2, both ends present in either:
    d1 inside the first quad under nominal 0, d2 in subband 0 under the first two trials (of one nominal where it has two)"""
    first = np.asarray(first)
    A, T = first.size - 1, int(first[-1])
    d1 = dedisp_ref.hashed_ints(A * nchan, max1, seed).reshape(A, nchan)
    d2 = dedisp_ref.hashed_ints(T * nsub, max2, seed + 1).reshape(T, nsub)
    d1[0, 0], d1[0, 1] = 0, max1
    d2[0, 0], d2[min(1, T - 1), 0] = (0, max2) if T > 1 else (max2, max2)
    return d1, d2


# A noise-free waterfall with a pulse of 3 rows swept by rtlws_dedisp_delays' formula at the DM of a nominal's middle
# trial: neighbouring trials' d2 differ by about 10 rows across the band and neighbouring nominals' d1 by about 6 across a
# subband, so that only the swept trial collects the pulse
PULSE = dict(nchan=256, nsub=16, shifted=1, f_centre_hz=150e6, bandwidth_hz=8e6, row_seconds=1e-3, ntrials=45, dm0=0.0, dm_step=0.5, per_nominal=9,
             nominal=2, row=40, width=3, nrows=700)


def pulse_sweep():
    """rtlws_subdedisp_delays' arguments"""
    return tuple(PULSE[n] for n in ("nchan", "nsub", "shifted", "f_centre_hz", "bandwidth_hz", "row_seconds", "ntrials", "dm0", "dm_step", "per_nominal"))


def pulse_waterfall():
    """(rows float32 [nrows, nchan], the trial the pulse is swept at, the row it is injected at)"""
    k = PULSE
    t0 = k["nominal"] * k["per_nominal"] + k["per_nominal"] // 2
    full = dedisp_ref.delays(k["nchan"], k["shifted"], k["f_centre_hz"], k["bandwidth_hz"], k["row_seconds"], k["ntrials"], k["dm0"], k["dm_step"])
    rows = np.zeros((k["nrows"], k["nchan"]), np.float32)
    for w in range(k["width"]):
        rows[k["row"] + w + full[t0], np.arange(k["nchan"])] = 1.0
    return rows, t0, k["row"]
