"""include/rtlws_cutout.h restated in numpy, word for word: the window of a candidate, the band-time plane (the rows of
a bin added in ascending row per channel, then the channels of a subband in ascending channel), the DM-time plane (the
samples of a bin in ascending n) and the info.  The loops over j and over c are plain loops, so that every addition is
one float32 rounding in the header's order; only the axes that no sum runs along are vectors.  No GPU, no library."""
import numpy as np

MIN_NCHAN, MAX_NCHAN, MAX_TRIALS, MAX_DELAY, MAX_WIDTHS, MAX_WIDTH, MAX_BIN = 4, 4096, 4096, 65535, 16, 1024, 1024
MIN_NX, MAX_NX, MAX_NF, MAX_RQ, MAX_DQ, MAX_NSAMP, MAX_CAND, CAND_WORDS, INFO_WORDS = 4, 256, 4096, 64, 64, 1 << 30, 4096, 8, 4


def window(at, width, b, nx, nsamp):
    """(n0, the number of n0 .. n0 + nx b - 1 inside 0 .. nsamp - 1)"""
    n0 = at + width // 2 - (nx // 2) * b
    return n0, max(min(n0 + nx * b, nsamp) - max(n0, 0), 0)


def _signed(word):
    return int(np.array([word], np.uint32).view(np.int32)[0])


def candidate(words, ntrials, widths, bins, nx, nsamp):
    """(t, b, n0, inside) of the candidate whose eight words these are, or None where it is not valid"""
    t, k, at = _signed(words[0]), _signed(words[2]), _signed(words[3])
    if not (0 <= t < ntrials and 0 <= k < len(widths) and 0 <= at < nsamp):
        return None
    n0, inside = window(at, int(widths[k]), int(bins[k]), nx, nsamp)
    return t, int(bins[k]), n0, inside


def band_time(rows, delays_t, mask, b, n0, nx, nf, nsamp):
    """F[f][x] of one candidate: rows float32 [nrows, >= nchan], delays_t int32 [nchan] the candidate's trial"""
    nchan = len(delays_t)
    cpb = nchan // nf
    keep = np.ones(nchan, bool) if mask is None else np.asarray(mask).astype(bool)
    x = np.arange(nx)
    R = np.zeros((nchan, nx), np.float32)
    for c in range(nchan):
        if not keep[c]:
            continue                                              # a masked channel's rows are never read
        acc = np.zeros(nx, np.float32)
        for j in range(b):
            n = n0 + x * b + j
            ok = (n >= 0) & (n < nsamp)
            acc[ok] = acc[ok] + rows[n[ok] + int(delays_t[c]), c]
        R[c] = acc
    F = np.zeros((nf, nx), np.float32)
    for f in range(nf):
        acc = np.zeros(nx, np.float32)
        for c in range(f * cpb, (f + 1) * cpb):
            if keep[c]:
                acc = acc + R[c]
        F[f] = acc
    return F


def dm_time(series, t, ntrials, b, n0, nx, rq, dq, nsamp):
    """G[r][x] of one candidate: series float32 [ntrials, >= nsamp]"""
    x = np.arange(nx)
    G = np.zeros((2 * rq + 1, nx), np.float32)
    for r in range(2 * rq + 1):
        q = t + (r - rq) * dq
        if not 0 <= q < ntrials:
            continue
        acc = np.zeros(nx, np.float32)
        for j in range(b):
            n = n0 + x * b + j
            ok = (n >= 0) & (n < nsamp)
            acc[ok] = acc[ok] + series[q, n[ok]]
        G[r] = acc
    return G


def cutout_ref(rows, series, cand, count, delays, mask, widths, bins, nx, nf, rq, dq, nsamp, max_cand):
    """-> (F float32 [m, nf, nx], G float32 [m, ndm, nx], info int32 [m, 4]), m = min(count[0], max_cand); rows or series
    None: that plane is None"""
    delays = np.asarray(delays, np.int32)
    ntrials = delays.shape[0]
    m = min(max(int(count[0]), 0), max_cand)
    F = None if rows is None else np.zeros((m, nf, nx), np.float32)
    G = None if series is None else np.zeros((m, 2 * rq + 1, nx), np.float32)
    info = np.zeros((m, INFO_WORDS), np.int32)
    with np.errstate(all="ignore"):
        for i in range(m):
            got = candidate(np.asarray(cand).reshape(-1, CAND_WORDS)[i], ntrials, widths, bins, nx, nsamp)
            if got is None:
                continue
            t, b, n0, inside = got
            info[i] = (n0, b, 1, inside)
            if F is not None:
                F[i] = band_time(rows, delays[t], mask, b, n0, nx, nf, nsamp)
            if G is not None:
                G[i] = dm_time(series, t, ntrials, b, n0, nx, rq, dq, nsamp)
    return F, G, info


def dedisp(rows, delays, mask, nsamp):
    """D[t][n] of include/rtlws_dedisp.h: float32 [ntrials, nsamp], the channels added in ascending position"""
    delays = np.asarray(delays, np.int32)
    out = np.zeros((delays.shape[0], nsamp), np.float32)
    n = np.arange(nsamp)
    with np.errstate(all="ignore"):
        for c in range(delays.shape[1]):
            if mask is None or mask[c]:
                out = out + rows[n[None, :] + delays[:, c][:, None], c]
    return out


def list_of(entries, room=0):
    """a list in the sift's form from (t, k, at) triples, at least `room` candidates long as the sift's d_cand is max_cand
    long; the words the cutouts do not read and the candidates behind the entries carry a pattern (no valid candidate)"""
    cand = np.full((max(len(entries), room, 1), CAND_WORDS), 0xDEADBEEF, np.uint32)
    for i, (t, k, at) in enumerate(entries):
        cand[i, [0, 2, 3]] = np.array([t, k, at], np.int64).astype(np.uint32)
    return cand


def waterfall(nrows, nchan, seed, delays=None, pulses=()):
    """seeded noise on a grid of 1/8 with a few dispersed pulses: (trial, row, amplitude) lights row + delays[trial][c] of
    every channel c"""
    rng = np.random.default_rng(seed)
    rows = (rng.integers(-64, 65, (nrows, nchan)) / 8.0 + rng.standard_normal((nrows, nchan))).astype(np.float32)
    for t, row, amp in pulses:
        for w in range(2):
            rows[row + w + np.asarray(delays[t]), np.arange(nchan)] += np.float32(amp)
    return rows
