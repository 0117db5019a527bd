"""include/rtlws_clean.h restated in numpy: the three stages in the header's order -- f64 sums by residue class and halving
tree, medians as elements of a sorted list, f32 arithmetic one rounding an operation (numpy.float32 arrays, so every
addition, subtraction, product and quotient below rounds once) -- the geometry's rule, the union mask, and the synthetic
waterfall the suites share (tests/test_clean_cpu.py, tests/test_clean_gpu.py).  Nothing here touches the library."""
import math

import numpy as np

MIN_NCHAN, MAX_NCHAN, MIN_BLOCK, MAX_BLOCK, MAX_NROWS, MAX_CELLS, ZERODM = 4, 4096, 32, 16384, 1 << 24, 1 << 22, 1
RES = 8
INF = float("inf")


def pow2_at_least(n):
    p = 1
    while p < n:
        p *= 2
    return p


def blocks_of(nrows, B):
    return -(-nrows // B)


def window_start(b, B, nrows):
    return min(b * B, nrows - B)


# ---- stage 1 ----

def sums_ref(window, residues=RES):
    """(s1, s2) float64 [M] of a window float32 [B, M]: per residue class of the row index the sums in ascending row from
    +0.0, then the halving tree over the classes.  residues must be a power of two."""
    x = window.astype(np.float64)
    q1, q2 = np.zeros((residues, x.shape[1])), np.zeros((residues, x.shape[1]))
    for k in range(x.shape[0]):
        q1[k % residues] = q1[k % residues] + x[k]
        q2[k % residues] = q2[k % residues] + x[k] * x[k]
    h = residues // 2
    while h >= 1:
        q1[:h], q2[:h] = q1[:h] + q1[h:2 * h], q2[:h] + q2[h:2 * h]
        h //= 2
    return q1[0], q2[0]


def stats_ref(window, mask=None):
    """(mu, sd float64 [M], m, r float32 [M], valid bool [M]) of one window"""
    B, M = window.shape
    with np.errstate(all="ignore"):
        s1, s2 = sums_ref(window)
        mu = s1 / np.float64(B)
        var = s2 / np.float64(B) - mu * mu
        sd = np.sqrt(var)
        m = mu.astype(np.float32)
        r = (np.float64(1.0) / sd).astype(np.float32)
    valid = np.isfinite(s1) & np.isfinite(s2) & (var > 0.0) & np.isfinite(r)
    if mask is not None:
        valid &= np.asarray(mask[:M]) != 0
    return mu, sd, m, r, valid


# ---- stage 2 ----

def med(values):
    """element floor((n - 1) / 2) of the values in ascending order"""
    ordered = sorted(float(v) for v in values)
    return ordered[(len(ordered) - 1) // 2]


def flags_ref(mu, sd, valid, t_mean, t_sigma):
    """keep bool [M] of one block"""
    keep = valid.copy()
    if not valid.any():
        return keep
    for x, t in ((mu, t_mean), (sd, t_sigma)):
        if t == INF:
            continue
        centre = med(x[valid])
        dev = np.abs(np.where(valid, x, 0.0) - np.float64(centre))
        mad = med(dev[valid])
        keep &= dev <= np.float64(t) * np.float64(mad)
    return keep


# ---- stage 3 ----

def row_tree(v, pairwise=True):
    """g[0] of the header for rows v float32 [rows, M]: the four of a lane left to right, zeros up to G, the halving tree.
    pairwise False: the plain left-to-right f32 sum of a row (what the tree is not)"""
    rows, M = v.shape
    if not pairwise:
        acc = np.zeros(rows, np.float32)
        for i in range(M):
            acc = acc + v[:, i]
        return acc
    G = pow2_at_least(M // 4)
    g = np.zeros((rows, G), np.float32)
    g[:, :M // 4] = ((v[:, 0::4] + v[:, 1::4]) + v[:, 2::4]) + v[:, 3::4]
    h = G // 2
    while h >= 1:
        g[:, :h] = g[:, :h] + g[:, h:2 * h]
        h //= 2
    return g[:, 0]


def apply_ref(rows, m, r, keep, zerodm):
    """the cleaned rows float32 [rows, M] of one block's rows"""
    with np.errstate(all="ignore"):
        v = np.where(keep[None, :], (rows - m[None, :]) * r[None, :], np.float32(0.0)).astype(np.float32)
        if not zerodm:
            return v
        nkept = int(keep.sum())
        if nkept == 0:
            return np.zeros_like(v)
        z = row_tree(v) / np.float32(nkept)
        return np.where(keep[None, :], v - z[:, None], np.float32(0.0)).astype(np.float32)


def clean_ref(rows, B, mask=None, t_mean=INF, t_sigma=INF, zerodm=True, nchan=None):
    """(out float32 [nrows, M], keep uint8 [nblocks, M], stats float32 [nblocks, M, 2], nkept int32 [nblocks]) of rows
    float32 [nrows, >= M]: what rtlws_clean_run writes"""
    rows = np.asarray(rows, np.float32)
    nrows = rows.shape[0]
    M = rows.shape[1] if nchan is None else nchan
    rows = rows[:, :M]
    nblocks = blocks_of(nrows, B)
    out = np.zeros((nrows, M), np.float32)
    keep, stats, nkept = np.zeros((nblocks, M), np.uint8), np.zeros((nblocks, M, 2), np.float32), np.zeros(nblocks, np.int32)
    for b in range(nblocks):
        j0 = window_start(b, B, nrows)
        mu, sd, m, r, valid = stats_ref(rows[j0:j0 + B], mask)
        kept = flags_ref(mu, sd, valid, t_mean, t_sigma)
        keep[b], nkept[b] = kept, kept.sum()
        stats[b, :, 0], stats[b, :, 1] = np.where(valid, m, np.float32(0.0)), np.where(valid, r, np.float32(0.0))
        mine = slice(b * B, min((b + 1) * B, nrows))
        out[mine] = apply_ref(rows[mine], m, r, kept, zerodm)
    return out, keep, stats, nkept


def zerodm_bound(v):
    """(6 + log2 G) 2^-24 sum |v_i| per row of v float32 [rows, M]"""
    G = pow2_at_least(v.shape[1] // 4)
    return (6 + math.log2(G)) * 2.0 ** -24 * np.abs(v.astype(np.float64)).sum(axis=1)


def union_mask(keep, min_share):
    keep = np.asarray(keep)
    return (keep.astype(bool).sum(axis=0).astype(np.float64) >= np.float64(min_share) * np.float64(keep.shape[0])).astype(np.uint8)


def geometry(nchan, B, nrows):
    """what rtlws_clean_geometry reports behind its return code"""
    nb = blocks_of(nrows, B)
    P, G = pow2_at_least(nchan), pow2_at_least(nchan // 4)
    T = max(256, G)
    at_once = 16 * T // G
    return ((nb * -(-nchan // 256), nb, nb * -(-B // at_once)), (512, min(max(P // 2, 64), 1024), T), (32768, 16 * P + 128, 8 * T if G > 64 else 0),
            nb, nb * (16 * nchan + 4), max_blocks(nchan, B))


def max_blocks(nchan, B):
    return min(-(-MAX_NROWS // B), MAX_CELLS // nchan)


# ---- the synthetic waterfall the issue's prototype ran on ----

SKY = dict(nchan=256, nrows=4196, B=512, shape=16.0, ripple=0.2, hot=(17, 101, 230), bursty=(60, 180), dead=3,
           pulse_amp=0.8, pulse_width=2, sweep=300, pulse_row=2000, burst_amp=1.0, burst_row=1500, burst_width=3)
PLANTED = SKY["hot"] + SKY["bursty"] + (SKY["dead"],)


def sky_delays(nchan=SKY["nchan"], sweep=SKY["sweep"]):
    """int32 [nchan]: a nu^-2 sweep over a band of ratio 1.25, 0 at the highest channel (the last), `sweep` rows at the first"""
    nu = np.linspace(1.0, 1.25, nchan)
    excess = nu ** -2.0 - nu[-1] ** -2.0
    return np.rint(sweep * excess / excess[0]).astype(np.int32)


def sky(seed, **changes):
    """float32 [nrows, nchan]: Gamma(shape) noise under a band-pass ripple of +-ripple, three channels at 5 x the mean, two
    with 60-row bursts at 6 x in every block, one dead (constant) channel, a dispersed pulse of pulse_amp sigma per channel
    and an undispersed burst of burst_amp sigma per channel -> (rows, delays)"""
    k = dict(SKY, **changes)
    M, N, B = k["nchan"], k["nrows"], k["B"]
    rng = np.random.default_rng(seed)
    gain = 1.0 + k["ripple"] * np.sin(2.0 * np.pi * (np.arange(M) / M * 3.0 + rng.random()))
    x = rng.gamma(k["shape"], 1.0, (N, M))
    sigma = math.sqrt(k["shape"])
    delays = sky_delays(M, k["sweep"])
    for w in range(k["pulse_width"]):
        x[k["pulse_row"] + w + delays, np.arange(M)] += k["pulse_amp"] * sigma
    x[k["burst_row"]:k["burst_row"] + k["burst_width"]] += k["burst_amp"] * sigma
    x *= gain[None, :]
    for i in k["hot"]:
        x[:, i] *= 5.0
    for i in k["bursty"]:
        for b in range(blocks_of(N, B)):
            j0 = window_start(b, B, N)
            at = j0 + int(rng.integers(0, B - 60))
            x[at:at + 60, i] *= 6.0
    x[:, k["dead"]] = 7.0
    return x.astype(np.float32), delays
