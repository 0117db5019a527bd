"""include/rtlws_sift.h restated in numpy, the yardstick of tests/test_sift_cpu.py and tests/test_sift_gpu.py: stage 1
(the score of every width in float64, one rounding an operation, once more to float32; the best width, ties to the
smaller k), stage 2 (the events at or above the threshold that no other event of their box beats, with the members of
their box and its extent in trials) and stage 3 (the list in ascending (s, t) order, eight words a candidate).  sift_slow
is the same definition event by event, for small planes: the two are held against each other."""
import numpy as np

MAX_WIDTHS, MAX_WIDTH, MIN_SEG, MAX_SEG, MAX_TRIALS, MAX_NOUT, MAX_RT, MAX_RS, MAX_CAND, CAND_WORDS = 16, 1024, 64, 1048576, 65536, 1 << 30, 32, 8, 1 << 24, 8
NEG_INF = np.float32(-np.inf)


def lengths(seg, nout):
    """the outputs of every segment: seg but for the last"""
    S = -(-nout // seg)
    return np.minimum(seg, nout - np.arange(S, dtype=np.int64) * seg)


def score_of_width(peak_k, w, mom, seg, nout):
    """peak_k float32 [T, S], mom float64 [T, S, 2] -> score_k float32 [T, S]"""
    ln = lengths(seg, nout)
    with np.errstate(all="ignore"):
        count = ln.astype(np.float64)[None, :]
        mean = mom[:, :, 0] / count
        var = mom[:, :, 1] / count - mean * mean
        snr = (peak_k.astype(np.float64) - np.float64(w) * mean) / np.sqrt(np.float64(w) * var)
        sc = snr.astype(np.float32)
    bad = (ln < 2)[None, :] | ~(var > 0.0) | np.isnan(peak_k) | (peak_k == NEG_INF) | np.isnan(sc)
    return np.where(bad, NEG_INF, sc).astype(np.float32)


def plane(peak, mom, widths, seg, nout):
    """stage 1: peak float32 [T, K, S], mom float64 [T, S, 2] -> (score float32 [T, S], k int32 [T, S])"""
    T, K, S = peak.shape
    assert S == -(-nout // seg) and mom.shape == (T, S, 2) and len(widths) == K
    best, k_of = np.full((T, S), NEG_INF, np.float32), np.zeros((T, S), np.int32)
    for k in range(K):
        sc = score_of_width(peak[:, k, :], widths[k], mom, seg, nout)
        take = sc > best
        best, k_of = np.where(take, sc, best), np.where(take, np.int32(k), k_of)
    return best, k_of


def maxima(score, threshold, rt, rs):
    """stage 2 -> (candidate bool [T, S], members, t_lo, t_hi int32 [T, S]; the three hold where candidate does)"""
    T, S = score.shape
    thr = np.float32(threshold)
    padded = np.full((T + 2 * rt, S + 2 * rs), np.nan, np.float32)
    padded[rt:rt + T, rs:rs + S] = score
    t_of = np.arange(T, dtype=np.int32)[:, None] + np.zeros((1, S), np.int32)
    beaten, members, lo, hi = np.zeros((T, S), bool), np.zeros((T, S), np.int32), t_of.copy(), t_of.copy()
    with np.errstate(invalid="ignore"):
        for dt in range(-rt, rt + 1):
            for ds in range(-rs, rs + 1):
                u = padded[rt + dt:rt + dt + T, rs + ds:rs + ds + S]
                member = u >= thr
                members += member
                lo, hi = np.where(member, np.minimum(lo, t_of + dt), lo), np.where(member, np.maximum(hi, t_of + dt), hi)
                beaten |= (u > score) | ((u == score) & (dt < 0 or (dt == 0 and ds < 0)))
        above = score >= thr
    return above & ~beaten, members, lo, hi


def sift_ref(peak, at, mom, widths, seg, nout, threshold, rt, rs):
    """-> (cand uint32 [found, 8] every candidate in ascending (s, t), count int32 [2], score float32 [T, S], k int32 [T, S]).
    A run with max_cand writes cand[:max_cand] and the same count."""
    peak, at, mom = np.asarray(peak, np.float32), np.asarray(at, np.int32), np.asarray(mom, np.float64)
    score, k_of = plane(peak, mom, widths, seg, nout)
    is_cand, members, lo, hi = maxima(score, threshold, rt, rs)
    s_idx, t_idx = np.nonzero(is_cand.T)                        # ascending s, then t
    k = k_of[t_idx, s_idx]
    cand = np.zeros((len(t_idx), CAND_WORDS), np.uint32)
    cand[:, 0], cand[:, 1], cand[:, 2] = t_idx, s_idx, k
    cand[:, 3] = np.where(score[t_idx, s_idx] > NEG_INF, at[t_idx, k, s_idx], np.int32(-1)).astype(np.int32).view(np.uint32)       # no width scored: (-Inf, 0, -1)
    cand[:, 4] = score[t_idx, s_idx].view(np.uint32)
    cand[:, 5] = np.ascontiguousarray(peak[t_idx, k, s_idx]).view(np.uint32)
    cand[:, 6] = members[t_idx, s_idx]
    cand[:, 7] = (hi[t_idx, s_idx].astype(np.uint32) << 16) | lo[t_idx, s_idx].astype(np.uint32)
    with np.errstate(invalid="ignore"):
        count = np.array([len(t_idx), int((score >= np.float32(threshold)).sum())], np.int32)
    return cand, count, score, k_of


def beats(a, b):
    """a, b: (score, t, s)"""
    return a[0] > b[0] or (a[0] == b[0] and (a[1] < b[1] or (a[1] == b[1] and a[2] < b[2])))


def sift_slow(score, threshold, rt, rs):
    """stages 2 and 3 event by event -> [(t, s, members, t_lo, t_hi)] in ascending (s, t)"""
    T, S = score.shape
    thr, out = np.float32(threshold), []
    for s in range(S):
        for t in range(T):
            if not score[t, s] >= thr:
                continue
            box = [(score[u, v], u, v) for u in range(max(t - rt, 0), min(t + rt, T - 1) + 1) for v in range(max(s - rs, 0), min(s + rs, S - 1) + 1)]
            if any(beats(b, (score[t, s], t, s)) for b in box if (b[1], b[2]) != (t, s)):
                continue
            inside = [b[1] for b in box if b[0] >= thr]
            out.append((t, s, len(inside), min(inside), max(inside)))
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------

def flat_moments(T, seg, nout, mean=3.0, var=4.0):
    """the moments of segments that all have the same mean and variance: equal peaks of a width then score equal bits
    in segments of equal length"""
    ln = lengths(seg, nout).astype(np.float64)
    mom = np.zeros((T, len(ln), 2), np.float64)
    mom[:, :, 0], mom[:, :, 1] = ln * mean, ln * (var + mean * mean)
    return mom


def random_case(T, K, S, seed, seg=64, tail=None, blobs=None, step=None):
    """(peak, at, mom, widths, seg, nout): noise scores around 0 +- 1 at every width, the moments of every segment
    different, and `blobs` pulses, each a peak spread over neighbouring trials and segments and falling off from its
    centre; step: the peaks rounded to multiples of it under flat moments, so that equal scores are common"""
    rng = np.random.default_rng(seed)
    nout = (S - 1) * seg + (seg if tail is None else tail)
    widths = np.sort(rng.choice(np.arange(1, 65), K, replace=False)).astype(np.int32)
    mu, sd = rng.uniform(1.0, 5.0, (T, S)), rng.uniform(0.5, 2.0, (T, S))
    if step is not None:
        mu[:], sd[:] = 3.0, 2.0
    ln = lengths(seg, nout).astype(np.float64)[None, :]
    mom = np.stack([ln * mu, ln * (sd * sd + mu * mu)], axis=2)
    z = rng.standard_normal((T, K, S))
    for _ in range(max(T * S // 40, 2) if blobs is None else blobs):
        t0, s0, amp = rng.integers(T), rng.integers(S), rng.uniform(5.0, 12.0)
        dt, ds = np.arange(T)[:, None] - t0, np.arange(S)[None, :] - s0
        z += amp * np.exp(-(dt / 2.5) ** 2 - (ds / 0.8) ** 2)[:, None, :] * rng.uniform(0.5, 1.0, K)[None, :, None]
    if step is not None:
        z = np.round(z / step) * step
    w = widths.astype(np.float64)[None, :, None]
    peak = (w * mu[:, None, :] + z * np.sqrt(w) * sd[:, None, :]).astype(np.float32)
    at = rng.integers(0, seg, (T, K, S)).astype(np.int32) + (np.arange(S, dtype=np.int32) * seg)[None, None, :]
    return peak, at, mom, widths, seg, nout


def richness(peak, at, mom, widths, seg, nout, threshold, rt, rs):
    """what keeps a random case from passing vacuously: (candidates, events at or above threshold that are no candidate,
    the most members of a candidate's box)"""
    cand, count, _, _ = sift_ref(peak, at, mom, widths, seg, nout, threshold, rt, rs)
    return len(cand), int(count[1]) - len(cand), int(cand[:, 6].max()) if len(cand) else 0
