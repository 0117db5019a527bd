"""include/rtlws_ffa.h restated in numpy: the fast folding transform in one go and in the plan's passes, the circular
boxcar sums in rtlws_pulse.h's order, the peaks per segment of rows with their tie rule, the plan as the header words it
-- the yardstick of tests/test_ffa_gpu.py, whose own properties tests/test_ffa_cpu.py holds.

  A_0[r][c] = D[r p + c];  stage j, blocks of 2^j rows from row g, s = 0 .. 2^j - 1:
  A_j[g + s][c] = fl(A_(j-1)[g + (s >> 1)][c] + A_(j-1)[g + 2^(j-1) + (s >> 1)][(c + ((s + 1) >> 1)) mod p])
  P_0 = a row;  P_(l+1)[c] = fl(P_l[c] + P_l[(c + 2^l) mod p]);  B_w: the pieces highest bit first, every index mod p
"""
import numpy as np

from pulse_ref import bits_of, signed_series            # noqa: F401  (signed_series: float32 [ntrials, n], both signs, exponents over 2^-6 .. 2^6)

MIN_P, MAX_P, MAX_L, MAX_CELLS, MAX_WIDTHS, MAX_WIDTH, MAX_TRIALS = 16, 1024, 12, 1 << 22, 16, 256, 65536
MAX_PASSES, MAX_STAGES, THREADS, WAVES, LDS_CAP, WORKSPACE_CAP = 3, 7, 512, 8, 160 * 1024, 1 << 30
SLOT_BYTES = MAX_WIDTHS * 8                              # a (best, at) pair per width


# ---- the transform -------------------------------------------------------------------------------------------------

def rows_of(x, p, m):
    """A_0 of x [.., >= m p]: [.., m, p]"""
    x = np.asarray(x, np.float32)
    return x[..., :m * p].reshape(x.shape[:-1] + (m, p))


def _roll(a, shift):
    """a[.., (c + shift) mod p] along the last axis"""
    return np.roll(a, -(shift % a.shape[-1]), axis=-1)


def stage(a, j):
    """A_j of A_(j-1) [.., m, p]"""
    out = np.empty_like(a)
    size, half = 1 << j, 1 << (j - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        for g in range(0, a.shape[-2], size):
            for s in range(size):
                out[..., g + s, :] = a[..., g + (s >> 1), :] + _roll(a[..., g + half + (s >> 1), :], (s + 1) >> 1)
    return out


def ffa(x, p, L):
    """prof [.., m, p] of x [.., >= m p], m = 2^L, every stage over all the rows in one go"""
    a = rows_of(x, p, 1 << L)
    for j in range(1, L + 1):
        a = stage(a, j)
    return a


def one_pass(rows_in, a, b, L):
    """stages a + 1 .. b over rows_in [.., m, p] whose blocks of 2^a rows are finished, as the pass kernel does them: a
    workgroup per superblock of 2^b rows from row B0 and q = 0 .. 2^a - 1 loads the rows B0 + i 2^a + q, runs a small
    transform whose shift at global stage j is ((s_j + 1) >> 1), s_j = (q << (j - a)) | u, and stores the rows
    B0 + q 2^(b-a) + u"""
    m, n = 1 << L, b - a
    out = np.empty_like(rows_in)
    with np.errstate(invalid="ignore", over="ignore"):
        for B0 in range(0, m, 1 << b):
            for q in range(1 << a):
                cur = np.stack([rows_in[..., B0 + (i << a) + q, :] for i in range(1 << n)], axis=-2)
                for jl in range(1, n + 1):
                    nxt = np.empty_like(cur)
                    for r in range(1 << n):
                        u = r & ((1 << jl) - 1)
                        g = r - u
                        sj = (q << jl) | u
                        nxt[..., r, :] = cur[..., g + (u >> 1), :] + _roll(cur[..., g + (1 << (jl - 1)) + (u >> 1), :], (sj + 1) >> 1)
                    cur = nxt
                out[..., B0 + (q << n):B0 + ((q + 1) << n), :] = cur
    return out


def ffa_passes(x, p, L, stages):
    """the transform in passes of `stages` stages each (they add to L)"""
    assert sum(stages) == L and all(n >= 1 for n in stages)
    a, rows = 0, rows_of(x, p, 1 << L)
    for n in stages:
        rows = one_pass(rows, a, a + n, L)
        a += n
    return rows


def splits_of(L):
    """every way to write L as an ordered sum of positive integers"""
    if L == 0:
        return [[]]
    return [[n] + rest for n in range(1, L + 1) for rest in splits_of(L - n)]


def sigma(r, s, L):
    """the shift at which input row r enters output row s: the sum over the stages j whose bit (j - 1) of r is set (r
    lies in the second half of its block there) of (s_j + 1) >> 1, s_j = s >> (L - j) the row's index at stage j"""
    return sum((((s >> (L - j)) + 1) >> 1) for j in range(1, L + 1) if r >> (j - 1) & 1)


def period(p, s, L):
    """p + s / (m - 1) in doubles; NaN where p is below 1, L outside 1 .. 12 or s outside 0 .. m - 1"""
    if p < 1 or not 1 <= L <= MAX_L or not 0 <= s < (1 << L):
        return np.nan
    return np.float64(p) + np.float64(s) / np.float64((1 << L) - 1)


def snr(peak, width, rows, sum1, sum2, count):
    """rtlws_ffa_snr's expression in numpy f64"""
    if count < 2 or width < 1 or rows < 1:
        return np.nan
    mean = np.float64(sum1) / np.float64(count)
    var = np.float64(sum2) / np.float64(count) - mean * mean
    if not var > 0:
        return np.nan
    n = np.float64(width) * np.float64(rows)
    return (np.float64(peak) - n * mean) / np.sqrt(n * var)


# ---- the widths and the peaks ---------------------------------------------------------------------------------------

def levels(prof, top):
    """[P_0 .. P_top] of prof [.., p], circular"""
    out = [prof]
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(top):
            out.append(out[-1] + _roll(out[-1], 1 << l))
    return out


def boxcar(prof, w, lv=None):
    """B_w of prof [.., p] -> [.., p]"""
    a = bits_of(w)
    lv = levels(prof, a[0]) if lv is None else lv
    b, off = lv[a[0]], 1 << a[0]
    with np.errstate(invalid="ignore", over="ignore"):
        for e in a[1:]:
            b = b + _roll(lv[e], off)
            off += 1 << e
    return b


def peaks(b, seg):
    """(peak float32 [.., nseg], at int32 [.., nseg]) of b [.., m, p]: per segment of seg rows the first, in (row,
    column) order, of the largest values that are not NaN, with its own bits and at = s p + c; (-Inf, -1) where nothing
    lies above -Inf"""
    m, p = b.shape[-2:]
    nseg = m // seg
    flat = b.reshape(-1, nseg, seg * p)
    v = np.where(np.isnan(flat), np.float32(-np.inf), flat)
    i = np.argmax(v, axis=2)                                     # the first occurrence; -0.0 == +0.0
    top = np.take_along_axis(v, i[..., None], axis=2)[..., 0]
    own = np.take_along_axis(flat, i[..., None], axis=2)[..., 0]
    won = top > -np.inf
    peak = np.where(won, own, np.float32(-np.inf)).astype(np.float32)
    at = np.where(won, i + np.arange(nseg)[None, :] * seg * p, -1).astype(np.int32)
    return peak.reshape(b.shape[:-2] + (nseg,)), at.reshape(b.shape[:-2] + (nseg,))


def samples_needed(p0, nper, L):
    return (p0 + nper - 1) << L


def ffa_ref(series, p0, nper, L, widths, seg):
    """(peak float32 [ntrials, nper, nseg, nwidths], at int32 of that shape, prof: a list of nper arrays float32
    [ntrials, m, p0 + i]) of series float32 [ntrials, >= samples_needed]; nothing at or beyond samples_needed is looked at"""
    series = np.asarray(series, np.float32)
    assert series.ndim == 2 and series.shape[1] >= samples_needed(p0, nper, L)
    m = 1 << L
    nseg, top = m // seg, int(max(widths)).bit_length() - 1
    peak = np.zeros((series.shape[0], nper, nseg, len(widths)), np.float32)
    at = np.zeros((series.shape[0], nper, nseg, len(widths)), np.int32)
    profs = []
    for i in range(nper):
        prof = ffa(series, p0 + i, L)
        profs.append(prof)
        lv = levels(prof, top)
        for k, w in enumerate(widths):
            peak[:, i, :, k], at[:, i, :, k] = peaks(boxcar(prof, int(w), lv), seg)
    return peak, at, profs


def peaks_by_the_letter(b, seg):
    """the header's loop over b [m, p], one comparison at a time"""
    m, p = b.shape
    peak, at = np.full(m // seg, -np.inf, np.float32), np.full(m // seg, -1, np.int32)
    for g in range(m // seg):
        best, where = np.float32(-np.inf), -1
        for s in range(g * seg, (g + 1) * seg):
            for c in range(p):
                if b[s, c] > best:
                    best, where = b[s, c], s * p + c
        peak[g], at[g] = best, where
    return peak, at


# ---- the plan, as the header words it ------------------------------------------------------------------------------

def supported(p0, nper, L, widths, seg):
    if p0 < MIN_P or nper < 1 or p0 + nper - 1 > MAX_P or not 1 <= L <= MAX_L or ((p0 + nper - 1) << L) > MAX_CELLS:
        return False
    if widths is None or not 1 <= len(widths) <= MAX_WIDTHS:
        return False
    if any(not 1 <= w <= min(MAX_WIDTH, p0) for w in widths) or any(b <= a for a, b in zip(widths, widths[1:])):
        return False
    return 1 <= seg <= (1 << L) and not seg & (seg - 1)


def max_stages(p_max):
    """the most stages of a pass: two copies of a tile of 2^n rows of p_max f32 and a pair of every width per row fit
    160 KiB; never more than 7"""
    n = 0
    while n < MAX_STAGES and (2 << (n + 1)) * p_max * 4 + (SLOT_BYTES << (n + 1)) <= LDS_CAP:
        n += 1
    return n


def split(L, p_max):
    """the stages of each pass: as few passes as max_stages allows, the stages dealt as evenly as they go, the larger
    shares first"""
    passes = -(-L // max_stages(p_max))
    out, left = [], L
    for k in range(passes, 0, -1):
        out.append(-(-left // k))
        left -= out[-1]
    return out


def eval_waves(n, p_max, top):
    """the wavefronts of the last pass (n stages) that evaluate a row each at a time: the largest power of two up to 8
    and 2^n whose `top` level rows each fit beside the tile"""
    e = min(WAVES, 1 << n)
    while e > 1 and ((1 << n) + max(1 << n, e * top)) * p_max * 4 + (SLOT_BYTES << n) > LDS_CAP:
        e //= 2
    return e


def plan(p0, nper, L, widths, seg, max_trials):
    """(passes, stages [3], workgroups per pair [3], threads, lds bytes [3], merge, workspace bytes, pairs in flight):
    rtlws_ffa_geometry's outputs; passes that a plan does not have are 0"""
    p_max, m, top = p0 + nper - 1, 1 << L, int(max(widths)).bit_length() - 1
    stages = split(L, p_max)
    last = stages[-1]
    blocks = [m >> n for n in stages]
    lds = [(2 << n) * p_max * 4 for n in stages[:-1]]
    e = eval_waves(last, p_max, top)
    lds.append(((1 << last) + max(1 << last, e * top)) * p_max * 4 + (SLOT_BYTES << last))
    merge = int(seg > (1 << last))
    per_pair = (len(stages) - 1) * m * p_max * 4 + (blocks[-1] * len(widths) * 8 if merge else 0)
    pairs = min(max_trials * nper, 65535)
    if per_pair:
        pairs = max(1, min(pairs, WORKSPACE_CAP // per_pair))
    pad = (0,) * (MAX_PASSES - len(stages))
    return len(stages), tuple(stages) + pad, tuple(blocks) + pad, THREADS, tuple(lds) + pad, merge, pairs * per_pair, pairs


# ---- data -----------------------------------------------------------------------------------------------------------

def train(n, period_samples, amplitude, seed):
    """float32 [n]: unit Gaussian noise plus `amplitude` at the samples nearest to the multiples of period_samples"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n)
    at = np.rint(np.arange(0, n / period_samples) * period_samples).astype(np.int64)
    x[at[at < n]] += amplitude
    return x.astype(np.float32)
