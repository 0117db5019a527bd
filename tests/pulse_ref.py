"""include/rtlws_pulse.h restated in numpy: the levels, the boxcar sums in their fixed order, the peaks with their tie
rule, the moments in their residue classes and halving tree -- the yardstick of tests/test_pulse_gpu.py, whose own
properties tests/test_pulse_cpu.py holds.  Everything works on [ntrials, n] arrays, a trial a row.

  P_0 = D;  P_(l+1)[n] = fl(P_l[n] + P_l[n + 2^l])
  B_w[n] = the pieces P_a[n + (the sum of w's higher bits)], highest bit first, added from the left, one f32 rounding each
"""
import numpy as np

MAX_WIDTHS, MAX_WIDTH, MIN_SEG, MAX_SEG, MAX_TRIALS, MAX_NOUT = 16, 1024, 64, 1 << 20, 65536, 1 << 30
LDS_WORDS = (4096, 8192, 16384)                  # f32 of LDS a workgroup takes: 16, 32, 64 KiB
LADDER = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024)
MIXED16 = (1, 2, 3, 5, 7, 12, 20, 33, 60, 100, 180, 255, 257, 511, 1000, 1023)


def bits_of(w):
    """the exponents of w's binary form, highest first"""
    return [a for a in range(int(w).bit_length() - 1, -1, -1) if w >> a & 1]


def depth(w):
    """additions on the longest path from a sample to B_w: floor(log2 w) + popcount(w) - 1"""
    return int(w).bit_length() - 1 + bin(int(w)).count("1") - 1


def levels(x, top):
    """[P_0, .., P_top] of x [.., n], in x's precision; P_l is 2^l - 1 entries shorter than x"""
    out = [x]
    for l in range(top):
        p = out[-1]
        out.append(p[..., :p.shape[-1] - (1 << l)] + p[..., 1 << l:])
    return out


def boxcar(x, w, lv=None):
    """B_w of x [.., n] -> [.., n - w + 1], in x's precision (float32: the definition; float64: the sum to compare with)"""
    a = bits_of(w)
    lv = levels(x, a[0]) if lv is None else lv
    n = x.shape[-1] - w + 1
    b, off = lv[a[0]][..., :n], 1 << a[0]
    for e in a[1:]:
        b = b + lv[e][..., off:off + n]
        off += 1 << e
    return b


def boxcars(x, widths):
    """[B_w for w in widths], the levels built once"""
    lv = levels(x, int(max(widths)).bit_length() - 1)
    return [boxcar(x, int(w), lv) for w in widths]


def sequential(x, w):
    """the ascending sum D[n] + D[n + 1] + .. in x's precision: what B_w is NOT from w = 5 on"""
    n = x.shape[-1] - w + 1
    b = x[..., :n].copy()
    for j in range(1, w):
        b = b + x[..., j:j + n]
    return b


def bound(x, w):
    """depth 2^-24 sum|terms| of every B_w[n], in f64"""
    return depth(w) * 2.0 ** -24 * boxcar(np.abs(x.astype(np.float64)), w)


def samples_needed(widths, nout):
    return nout + int(max(widths)) - 1 if nout else 0


def segments(nout, seg):
    return -(-nout // seg)


def peaks(b, seg, nout):
    """(peak float32 [ntrials, nseg], at int32 [ntrials, nseg]) of b [ntrials, >= nout]: the first of the largest values
    that are not NaN, with its own bits; (-Inf, -1) where nothing lies above -Inf"""
    nseg = segments(nout, seg)
    peak, at = np.full((b.shape[0], nseg), -np.inf, np.float32), np.full((b.shape[0], nseg), -1, np.int32)
    rows = np.arange(b.shape[0])
    for s in range(nseg):
        part = b[:, s * seg:min((s + 1) * seg, nout)]
        v = np.where(np.isnan(part), np.float32(-np.inf), part)
        i = np.argmax(v, axis=1)                                # the first occurrence of the maximum; -0.0 == +0.0
        won = v[rows, i] > -np.inf
        peak[won, s] = part[rows, i][won]
        at[won, s] = (s * seg + i)[won]
    return peak, at


def peaks_by_the_letter(b, seg, nout):
    """the header's loop, one comparison at a time (slow: for the restatement's own tests)"""
    nseg = segments(nout, seg)
    peak, at = np.full((b.shape[0], nseg), -np.inf, np.float32), np.full((b.shape[0], nseg), -1, np.int32)
    for t in range(b.shape[0]):
        for s in range(nseg):
            best, where = np.float32(-np.inf), -1
            for n in range(s * seg, min((s + 1) * seg, nout)):
                if b[t, n] > best:
                    best, where = b[t, n], n
            peak[t, s], at[t, s] = best, where
    return peak, at


def moments(x, seg, nout):
    """float64 [ntrials, nseg, 2] of x [ntrials, >= nout]: 256 residue classes summed in ascending j, then the halving tree"""
    nseg = segments(nout, seg)
    out = np.zeros((x.shape[0], nseg, 2), np.float64)
    for s in range(nseg):
        part = x[:, s * seg:min((s + 1) * seg, nout)].astype(np.float64)
        rows = -(-part.shape[1] // 256)
        padded = np.zeros((x.shape[0], rows * 256), np.float64)      # a class never holds -0.0: adding +0.0 changes no bit
        padded[:, :part.shape[1]] = part
        padded = padded.reshape(x.shape[0], rows, 256)
        for j, y in enumerate((padded, padded * padded)):
            q = np.zeros((x.shape[0], 256), np.float64)
            for r in range(rows):
                q = q + y[:, r]
            h = 128
            while h >= 1:
                q = q[:, :h] + q[:, h:2 * h]
                h //= 2
            out[:, s, j] = q[:, 0]
    return out


def pulse_ref(series, widths, seg, nout):
    """(peak float32 [ntrials, nwidths, nseg], at int32 of that shape, mom float64 [ntrials, nseg, 2]) of series float32
    [ntrials, >= samples_needed]; nothing at or beyond samples_needed is looked at"""
    series = np.asarray(series, np.float32)
    need = samples_needed(widths, nout)
    assert series.ndim == 2 and series.shape[1] >= need
    x = series[:, :need]
    nseg = segments(nout, seg)
    peak = np.zeros((x.shape[0], len(widths), nseg), np.float32)
    at = np.zeros((x.shape[0], len(widths), nseg), np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k, b in enumerate(boxcars(x, widths)):
            peak[:, k], at[:, k] = peaks(b[:, :nout], seg, nout)
        mom = moments(x, seg, nout)
    return peak, at, mom


def worst_ratio(series, widths, nout):
    """the largest |B_w - its f64 sum| / bound over the finite outputs of every width"""
    x = np.asarray(series, np.float32)[:, :samples_needed(widths, nout)]
    x64 = x.astype(np.float64)
    worst = 0.0
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for w, b, b64 in zip(widths, boxcars(x, widths), boxcars(x64, widths)):
            lim = bound(x, int(w))
            ok = np.isfinite(b64) & np.isfinite(lim) & (lim > 0)
            if ok.any():
                worst = max(worst, float((np.abs(b.astype(np.float64) - b64)[ok] / lim[ok]).max()))
    return worst


def snr(peak, width, sum1, sum2, count):
    """rtlws_pulse_snr's expression in numpy f64"""
    if count < 2 or width < 1:
        return np.nan
    mean = np.float64(sum1) / np.float64(count)
    var = np.float64(sum2) / np.float64(count) - mean * mean
    if not var > 0:
        return np.nan
    return (np.float64(peak) - np.float64(width) * mean) / np.sqrt(np.float64(width) * var)


# ---- the plan, as the header words it ----------------------------------------------------------------------------

def plan(widths):
    """(tile_out, lds_bytes, levels_kept, rows, row) of a table: one row of roundup4(tile_out + w_max - 1) f32 for every
    bit set over the table and at most two for the levels in between; the largest tile of 1024, 512, 256 whose rows fit
    in 64 KiB; the smallest of 16, 32, 64 KiB that holds them"""
    bits = 0
    for w in widths:
        bits |= int(w)
    w_max = int(max(widths))
    kept = bin(bits).count("1")
    rows = kept + min(2, w_max.bit_length() - kept)
    for tile in (1024, 512, 256):
        row = (tile + w_max - 1 + 3) // 4 * 4
        if rows * row <= LDS_WORDS[-1]:
            break
    lds = min(words for words in LDS_WORDS if words >= rows * row)
    return tile, lds * 4, kept, rows, row


# ---- data ---------------------------------------------------------------------------------------------------------

def signed_series(ntrials, n, seed):
    """float32 [ntrials, n]: both signs, exponents spread over 2^-6 .. 2^6, finite, none zero"""
    rng = np.random.default_rng(seed)
    x = (1.0 + rng.random((ntrials, n))) * np.exp2(rng.integers(-6, 7, (ntrials, n))) * rng.choice([-1.0, 1.0], (ntrials, n))
    return x.astype(np.float32)
