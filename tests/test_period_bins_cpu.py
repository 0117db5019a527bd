"""CPU suite of the per-bin bound of the periodicity family's power spectra (period_ref.bound_bin, periodlong_ref.bound_bin;
DESIGN.md 4.22a, 4.23a): evidence, without a GPU, that the bound and the inputs of tests/period_bins_cases.py fit each
other and that the check is not idle.

model() is a plain numpy float32 / complex64 restatement of stage 1 of period.hip (the row transform of row_fft.h in
LDS) and of periodlong.hip (columns, twist, rows, untangling): the same tables as arrays (period_plan.h's host_tables
restated in tables(): tw, twist, tw_row, tw256; the short frames' one table tw), the same index maps (the radix-16
passes' exponents j q 2 M / L through the half table, pos(k), j = j1 M2 + j2, k = k1 + M1 k2, the 256-point columns' j1 =
a + 16 n, k1 = q + 16 q2), 16-point transforms as plain matrix products.  It does not reproduce the device's bits.

  the clean model is within the per-bin bound on every input of period_bins_cases and on the GPU suites' noise
  entries of every table are mutated -- zeroed, negated, replaced by the entry at the other end (the gross kinds),
      conjugated, displaced by D places of phase -- and each mutation puts at least one bin of at least one case
      outside the bound.  D(log2n) is the smallest displacement whose phase error 2 pi D / size exceeds four times b1;
      smaller ones are inside worst-case rounding and not claimed, a conjugation that moves an entry by less neither.
      The gross kinds take the first and last entry the kernels read, each side of the M1 and M2 borders and 64 seeded
      entries of all that are read (tw's upper half in the long frames, the odd entries of tw_row, row 0 of the twist
      with M1 = 16 and most of tw256 are never read; a mutation there changes nothing and is not listed).  A phase error
      of 4 b1 in ONE term shows only where that term is a large share of ||y||_1 and another term, which keeps its
      phase, stands beside it (the power does not see a bin that turns as a whole), so the two small kinds take their
      entries, the same borders and 64 seeded ones, from those that one impulse of a pair drives at full weight while the
      other stays away; every such pair is a probe
  two adjacent bins swapped, and a tile of bins swapped with their mirrors M - k, are outside the bound on the noise
  from log2n 17 on a zeroed entry of tw passes the aggregate bound on pairs of impulses that it puts outside the per-bin
      one, from 18 on on every one of them: the reason for the per-bin check
  (at log2n 20 the mutations are of twist and tw256, what M1 = 256 reads otherwise than M1 = 16, 8 seeded entries each)

Worst per-bin share of the bound, the clean model (printed by test_the_clean_model), on the cases: 0.0293, 0.0266,
0.0256, 0.0295, 0.0316, 0.0334 at log2n 10 .. 15, 0.0314, 0.0332, 0.0328, 0.0316 at 16, 19, 20, 22; on the suites' noise
0.0062, 0.0030, 0.0061, 0.0071, 0.0059, 0.0084 and 0.0059, 0.0079, 0.0023, 0.0013.  D is 1 place for every table up to
log2n 17, 9 places of tw and twist at 20.  With tw[24280] zeroed at log2n 17, 4 of the 8 pairs a, -a pass the aggregate
bound; with tw[233898] zeroed at 20, all 8."""
import math

import numpy as np
import pytest

import period_bins_cases as cases
import period_ref
import periodlong_ref
from period_family import noise

LOG2NS = cases.SHORT_LOG2NS + cases.LONG_LOG2NS
MUTATED_LOG2NS = (10, 12, 16, 17, 20)            # 16 . 16 . 2 and three radix-16 passes; M1 = 16 twice; M1 = 256


def _long(log2n):
    return log2n >= periodlong_ref.MIN_LOG2N


def bounds(log2n):
    ref = periodlong_ref if _long(log2n) else period_ref
    return ref.bound(log2n), ref.bound_bin(log2n)


# ---- the tables: period_plan.h's host_tables in a few lines ------------------------------------------------------

def root(n, k):
    """e^(-2 pi i k / n) rounded once to complex64"""
    a = (np.asarray(k, np.int64) % n) * (2.0 * np.pi / n)
    return (np.cos(a) - 1j * np.sin(a)).astype(np.complex64)


def tables(log2n):
    """tw [M]; for the long frames twist [M1 M2], tw_row [M2], tw256 [256] too"""
    n = 1 << log2n
    m = n // 2
    t = {"tw": root(n, np.arange(m))}
    if _long(log2n):
        l1, l2 = periodlong_ref.split(log2n)
        m1, m2 = 1 << l1, 1 << l2
        t["twist"] = root(n, 2 * np.outer(np.arange(m1), np.arange(m2)).reshape(-1))
        t["tw_row"] = root(n, np.arange(m2) * m1)
        t["tw256"] = root(n, np.arange(256) * (n // 256))
    return t


def phase(log2n, table, i):
    """(p, size): entry i of a table is the root p of `size`"""
    n = 1 << log2n
    if table == "tw":
        return i, n
    l1, l2 = periodlong_ref.split(log2n)
    if table == "twist":
        return 2 * (i >> l2) * (i & ((1 << l2) - 1)), n
    return (i, 2 << l2) if table == "tw_row" else (i, 256)


D16 = root(16, np.outer(np.arange(16), np.arange(16)))


# ---- the model ------------------------------------------------------------------------------------------------------

def _note(rec, table, idx, mag):
    """the largest |operand| that met each entry, per trial: rec[table] float32 [trials, size]"""
    if rec is not None:
        for t in range(mag.shape[0]):
            np.maximum.at(rec[table][t], idx.ravel(), mag[t].ravel())


def row_fft(a, tw, table, rec):
    """row_fft.h's forward over the last axis of complex64 [trials, .., M]: radix-16 passes over blocks of L points with
    W_L^(j q) = root<M>(tw, j q 2 M / L), a last pass of radix R, bin k from place pos(k)"""
    m = a.shape[-1]
    log2m = m.bit_length() - 1
    three = log2m >= 12
    r = 1 << (log2m - 12 if three else log2m - 8)
    lead = a.shape[:-1]
    for l in (m, m // 16, m // 256)[:3 if three else 2]:
        stride = l // 16
        v = np.matmul(D16, a.reshape(lead + (m // l, 16, stride)))           # [.., block, q, j]
        if l > 16:
            e = np.outer(np.arange(16), np.arange(stride)) * (2 * m // l)
            idx = e & (m - 1)
            _note(rec, table, idx, np.abs(v).reshape((lead[0], -1, 16, stride)).max(axis=1))
            v = v * np.where(e < m, tw[idx], -tw[idx])
        a = v.reshape(lead + (m,))
    if r > 1:
        a = np.matmul(a.reshape(lead + (m // r, r)), root(r, np.outer(np.arange(r), np.arange(r)))).reshape(lead + (m,))
    k = np.arange(m)
    pos = (k & 15) * (m // 16) + ((k >> 4) & 15) * (m // 256) + (((k >> 8) & 15) * (m // 4096) + (k >> 12) if three else k >> 8)
    assert a.dtype == np.complex64
    return a[..., pos]


def packed(x, nsamp, log2n):
    """z [trials, M] complex64 of float32 [trials, >= nsamp]: the f64 mean removed, zeros behind nsamp"""
    n = 1 << log2n
    x64 = x[:, :nsamp].astype(np.float64)
    y = np.zeros((x.shape[0], n), np.float32)
    y[:, :nsamp] = (x64 - x64.mean(axis=1, keepdims=True)).astype(np.float32)
    return (y[:, 0::2] + 1j * y[:, 1::2]).astype(np.complex64)


def transform(z, log2n, t, rec):
    """Z [trials, M] in natural order"""
    if not _long(log2n):
        return row_fft(z, t["tw"], "tw", rec)
    l1, l2 = periodlong_ref.split(log2n)
    m1, m2 = 1 << l1, 1 << l2
    trials = z.shape[0]
    if l1 == 4:
        a = np.matmul(D16, z.reshape(trials, 16, m2))                        # [k1, j2]
    else:
        v = np.matmul(D16, z.reshape(trials, 16, 16 * m2)).reshape(trials, 16, 16, m2)      # [q, a, j2] over j1 = a + 16 n
        idx = np.outer(np.arange(16), np.arange(16))
        _note(rec, "tw256", idx, np.abs(v).max(axis=3))
        v = v * t["tw256"][idx][:, :, None]
        a = np.matmul(D16, v).reshape(trials, 256, m2)                       # [q, q2, j2] -> over a: [q, q2]; k1 = q + 16 q2
        a = a.reshape(trials, 16, 16, m2).transpose(0, 2, 1, 3).reshape(trials, 256, m2)
    first = 1 if l1 == 4 else 0                                              # cols16 leaves row 0 alone
    idx = np.arange(first * m2, m1 * m2).reshape(m1 - first, m2)
    _note(rec, "twist", idx, np.abs(a[:, first:]))
    a[:, first:] = a[:, first:] * t["twist"][idx]
    b = row_fft(a, t["tw_row"], "tw_row", rec)                               # [k1, k2]
    return np.ascontiguousarray(b.transpose(0, 2, 1)).reshape(trials, m1 * m2)


def model(x, nsamp, log2n, t, rec=None):
    """P float32 [trials, M] of float32 [trials, >= nsamp]"""
    m = 1 << (log2n - 1)
    zz = transform(packed(x, nsamp, log2n), log2n, t, rec)
    k = np.arange(1, m // 2 + 1)
    za, zb = zz[:, k], np.conj(zz[:, m - k])
    e, o = np.complex64(0.5) * (za + zb), np.complex64(0.5) * (za - zb)
    _note(rec, "tw", k, np.abs(o))
    w = o * t["tw"][k]
    xa, xb = e - np.complex64(1j) * w, e + np.complex64(1j) * w
    p = np.empty((x.shape[0], m), np.float32)
    p[:, 0] = (zz[:, 0].real + zz[:, 0].imag) ** 2
    p[:, m - k] = xb.real * xb.real + xb.imag * xb.imag
    p[:, k] = xa.real * xa.real + xa.imag * xa.imag
    assert zz.dtype == np.complex64 and xa.dtype == np.complex64
    return p


def read_entries(log2n):
    """the entries of each table that the kernels read at all, sorted"""
    m = 1 << (log2n - 1)
    out = {"tw": set(range(1, m // 2 + 1))}

    def passes(mm, name):
        log2m = mm.bit_length() - 1
        for l in (mm, mm // 16, mm // 256)[:3 if log2m >= 12 else 2]:
            if l > 16:
                e = np.outer(np.arange(16), np.arange(l // 16)) * (2 * mm // l)
                out.setdefault(name, set()).update((e & (mm - 1)).ravel().tolist())
    if not _long(log2n):
        passes(m, "tw")
    else:
        l1, l2 = periodlong_ref.split(log2n)
        passes(1 << l2, "tw_row")
        out["twist"] = set(range((1 << l2) if l1 == 4 else 0, m))
        if l1 == 8:
            out["tw256"] = set(np.outer(np.arange(16), np.arange(16)).ravel().tolist())
    return {name: np.array(sorted(s), np.int64) for name, s in out.items()}


# ---- the checks ---------------------------------------------------------------------------------------------------

_REF = {}


def reference(case, log2n):
    """(x float32 [nsamp], the f64 spectrum, the per-bin allowance) of a case, computed once"""
    key = (log2n, case[0])
    if key not in _REF:
        x = cases.series(case)
        ref = periodlong_ref.power(x, log2n)
        _REF[key] = (x, ref, period_ref.bin_allowance(x, ref, bounds(log2n)[1]))
    return _REF[key]


def shares(p, some, log2n):
    """the worst per-bin share of each trial of p, the model's rows of the cases `some`"""
    out = []
    for row, case in zip(p, some):
        _, ref, allow = reference(case, log2n)
        out.append(float((np.abs(np.sqrt(row.astype(np.float64)) - np.sqrt(ref)) / allow).max()))
    return out


def aggregate_share(row, case, log2n):
    _, ref, _ = reference(case, log2n)
    return float(np.abs(row.astype(np.float64) - ref).sum() / (bounds(log2n)[0] * ref.sum()))


def run(some, log2n, t, rec=None):
    """the model over cases of any nsamp -> P [len(some), M]"""
    out = np.empty((len(some), 1 << (log2n - 1)), np.float32)
    for nsamp in sorted({c[1] for c in some}):
        which = [i for i, c in enumerate(some) if c[1] == nsamp]
        sub = None if rec is None else {name: r[which] for name, r in rec.items()}
        out[which] = model(cases.stacked([some[i] for i in which], nsamp), nsamp, log2n, t, sub)
        if rec is not None:
            for name in rec:
                rec[name][which] = sub[name]
    return out


def suite_noise(log2n):
    """the series of the GPU suites' test_every_frame_length"""
    n = 1 << log2n
    if _long(log2n):
        x = noise(2 if log2n <= 19 else 1, n, seed=log2n)
    else:
        x = noise(2, n, seed=log2n, draw=np.float64)
    x[-1] += (3.0 * np.cos(2.0 * np.pi * np.arange(n) / 37.5)).astype(np.float32)
    return x


def test_the_bound_is_the_derivation():
    """bound_bin from bound()'s constants: b_fft as bound() has it, sqrt 2 of it through the untangling, twice b_u behind;
    between one and two times t eta, growing with log2n, the twist's tau on top in the long frames"""
    u = 2.0 ** -24
    eta = u + 4 * u / (1 - 4 * u) * (math.sqrt(2.0) + u)
    for log2n in range(10, 23):
        b1 = bounds(log2n)[1]
        t = log2n - 1
        assert math.sqrt(2.0) * t * eta < b1 < 2.0 * t * eta
        if log2n > 10:
            assert b1 > bounds(log2n - 1)[1]
    tau = u + math.sqrt(2.0) * 3 * u / (1 - 3 * u)
    gap = periodlong_ref.bound_bin(16) - period_ref.bound_bin(16)
    assert math.sqrt(2.0) * tau < gap < 1.5 * tau
    x = np.float32([3.0, -1.0, 2.5])
    assert period_ref.mean_term(x) == pytest.approx(4 * 2.0 ** -53 * 6.5, rel=1e-9)
    allow = period_ref.bin_allowance(x, np.zeros(8), 1e-5)
    assert allow.shape == (8,) and np.all(allow > 1e-5 * np.abs(x - x.mean()).sum())
    assert period_ref.bin_share(np.zeros(8, np.float32), x, np.zeros(8), 1e-5) == (0.0, 0)
    assert period_ref.bin_share(np.full(8, np.nan, np.float32), x, np.zeros(8), 1e-5)[0] == np.inf


def test_the_cases_are_what_they_say():
    for log2n in LOG2NS:
        l1, l2 = cases.split(log2n)
        n, m1, m2 = 1 << log2n, 1 << l1, 1 << l2
        ps = cases.pairs(log2n)
        places = [[cases.place(log2n, int(v)) for v in c[2]] for c in ps]
        assert {p[2] for pl in places for p in pl} == {0, 1}
        assert any(a[1] == b[1] for a, b in places) and any(a[1] != b[1] for a, b in places)
        flat = [p for pl in places for p in pl]
        assert {0, m2 - 1} <= {p[1] for p in flat} and {0, m1 - 1} <= {p[0] for p in flat}
        assert any(c[1] < n and int(c[2].max()) == c[1] - 1 for c in ps) and any(int(c[2].max()) == n - 1 for c in ps)
        assert {int(c[2].max()) & 1 for c in ps if c[1] < n} == {0, 1}
        row, col = cases.combs(log2n)
        assert sorted(cases.place(log2n, int(v))[1] for v in row[2]) == list(range(m2)) and len({cases.place(log2n, int(v))[0] for v in row[2]}) == 1
        assert sorted(cases.place(log2n, int(v))[0] for v in col[2]) == list(range(m1)) and len({cases.place(log2n, int(v))[1] for v in col[2]}) == 1
        assert np.abs(row[3]).sum() == m2 and len(set(row[3].tolist())) == 2 and len(set(col[3].tolist())) > 2
        for c in cases.cases(log2n):
            assert set(np.abs(c[3]).tolist()) <= set(cases.SIZES.tolist()) and len(set(c[2].tolist())) == c[2].size
            assert c[0] == "unequal" or c[3].astype(np.float64).sum() == 0.0
        assert len(cases.eights(log2n)) >= 4 and all(c[2].size == 8 for c in cases.eights(log2n))


def test_the_model_is_the_transform():
    """against numpy's own FFT, far inside any bound: the index maps are the kernels'"""
    for log2n in (10, 11, 12, 13, 14, 15, 16, 20):
        x = suite_noise(log2n)[:1]
        p = model(x, x.shape[1] - 3, log2n, tables(log2n))[0]
        ref = periodlong_ref.power(x[0, :x.shape[1] - 3], log2n)
        assert np.abs(p - ref).max() <= 1e-4 * ref.max(), log2n


@pytest.mark.parametrize("log2n", LOG2NS)
def test_the_clean_model(log2n):
    """every case and the suites' noise within the per-bin bound (and the aggregate one); two adjacent bins swapped and
    a tile of bins swapped with their mirrors are not"""
    t = tables(log2n)
    some = cases.cases(log2n)
    worst = 0.0
    for first in range(0, len(some), 4):
        part = some[first:first + 4]
        p = run(part, log2n, t)
        got = shares(p, part, log2n)
        assert max(got) <= 1.0, (log2n, [c[0] for c in part], got)
        assert max(aggregate_share(row, c, log2n) for row, c in zip(p, part)) <= 1.0
        worst = max(worst, max(got))
        if log2n >= 20:
            for c in part:
                _REF.pop((log2n, c[0]))
    x = suite_noise(log2n)
    m, b1 = 1 << (log2n - 1), bounds(log2n)[1]
    l1, _ = cases.split(log2n)
    tile = min((1 << l1) * (64 if l1 == 4 else 16), m // 4)                  # untangle_kernel's L
    p = model(x, x.shape[1], log2n, t)
    rng = np.random.default_rng(log2n)
    worst_noise = 0.0
    for row, xs in zip(p, x):
        ref = periodlong_ref.power(xs, log2n)
        share = period_ref.bin_share(row, xs, ref, b1)[0]
        assert share <= 1.0, (log2n, share)
        worst_noise = max(worst_noise, share)
        # a swap of two bins whose true amplitudes agree within the allowance is no fault any check can see: the seeded
        # swaps are of neighbours that differ by more than twice the allowance.  At 2^22 the allowance is 0.03 of the
        # Rayleigh scale sqrt(N / 2) sigma of a bin of noise, four allowances cover about 0.13 of the differences of two
        # such amplitudes; shorter frames leave fewer out
        amp = np.sqrt(ref)
        apart = np.abs(amp[1:m - 1] - amp[2:m]) > 2.0 * period_ref.bin_allowance(xs, ref, b1)[1:m - 1]
        assert apart.mean() >= 0.8, (log2n, apart.mean())
        for k in 1 + rng.choice(np.flatnonzero(apart), 8, replace=False):
            bad = row.copy()
            bad[k], bad[k + 1] = row[k + 1], row[k]
            assert period_ref.bin_share(bad, xs, ref, b1)[0] > 1.0, (log2n, "adjacent", k)
        k0 = tile * int(rng.integers(0, m // 2 // tile))
        k = np.arange(max(k0, 1), k0 + tile)
        bad = row.copy()
        bad[k], bad[m - k] = row[m - k], row[k]
        assert period_ref.bin_share(bad, xs, ref, b1)[0] > 1.0, (log2n, "mirrors", k0)
    print("log2n %d: the clean model's worst bin %.3g of bound_bin %.3g on the cases, %.3g on the noise" % (log2n, worst, b1, worst_noise))


# ---- mutated tables -------------------------------------------------------------------------------------------------

def displacement(log2n, size):
    """D: the smallest displacement whose phase error 2 pi D / size exceeds four times b1"""
    return int(math.floor(4.0 * bounds(log2n)[1] * size / (2.0 * math.pi))) + 1


def listed(log2n, entries, rng, count=64):
    """of the sorted `entries`: the first and last, those on each side of the M1 and M2 borders, and `count` seeded others"""
    l1, l2 = cases.split(log2n)
    near = {int(entries[0]), int(entries[-1])}
    for border in (1 << l1, 1 << l2):
        at = int(np.searchsorted(entries, border))
        near.update(int(entries[i]) for i in (at - 1, at) if 0 <= i < entries.size)
    rest = np.setdiff1d(entries, np.array(sorted(near)))
    return sorted(near) + sorted(int(v) for v in rng.choice(rest, min(count, rest.size), replace=False))


def detected(log2n, t, table, i, value, probes):
    """does the model with t[table][i] = value put a bin of one of the probes (lists of cases, tried in turn) outside?
    One mutation is no fault: in the long frames tw[M / 2] = -i serves the bin that is its own mirror alone, and its
    negative (which is its conjugate) gives conj X[M / 2], the same power"""
    if _long(log2n) and table == "tw" and i == 1 << (log2n - 2) and abs(value + t[table][i]) < 1e-6:
        return True
    keep = t[table][i]
    t[table][i] = value
    try:
        return any(max(shares(run(some, log2n, t), some, log2n)) > 1.0 for some in probes if some)
    finally:
        t[table][i] = keep


@pytest.mark.parametrize("log2n", MUTATED_LOG2NS)
def test_every_mutation_is_seen(log2n):
    t = tables(log2n)
    read = read_entries(log2n)
    ps, combs, eights = cases.pairs(log2n), cases.combs(log2n), cases.eights(log2n)
    rec = {name: np.zeros((len(ps), tab.size), np.float32) for name, tab in t.items()}
    assert max(shares(run(ps, log2n, t, rec), ps, log2n)) <= 1.0
    # which entries one impulse of a pair a, -a drives at full weight while the other stays away: the impulses alone
    equal = [c for c in ps if c[0] != "unequal"]
    alone = [(c[0], c[1], c[2][h:h + 1], c[3][h:h + 1]) for c in equal for h in (0, 1)]
    met = {name: np.zeros((len(alone), tab.size), np.float32) for name, tab in t.items()}
    run(alone, log2n, t, met)
    full = np.array([abs(c[3][0]) for c in equal], np.float32)[:, None]
    rng = np.random.default_rng(3000 + log2n)
    counts = {}
    # the long pole: at 2^20 the two tables that M1 = 256 reads otherwise than M1 = 16 does, and 8 seeded entries each
    count = 64 if log2n < 20 else 8
    for name in sorted(read) if log2n < 20 else ("tw256", "twist"):          # tw256 is read with M1 = 256 alone
        assert set(np.flatnonzero(rec[name].max(axis=0)).tolist()) <= set(read[name].tolist()), name
        size = t[name].size
        # the gross kinds, on what is read
        gross = listed(log2n, read[name], rng, count)
        for i in gross:
            for kind, value in (("zeroed", 0.0), ("negated", -t[name][i]), ("other end", t[name][size - 1 - i])):
                if abs(value - t[name][i]) < 0.5:
                    continue                                 # an other end this near (the twist's first column: the same 1) is not gross
                assert detected(log2n, t, name, i, value, (combs, ps, eights)), (log2n, name, i, kind)
                counts[name, kind] = counts.get((name, kind), 0) + 1
        # the small kinds, on what one impulse of a pair drives at full weight and the other does not: those pairs are the probes
        one, other = met[name][0::2], met[name][1::2]
        driven = ((one >= 0.99 * full) & (other <= 0.01 * full)) | ((other >= 0.99 * full) & (one <= 0.01 * full))
        entries = np.flatnonzero(driven.any(axis=0))
        assert entries.size >= 4, (name, entries.size)
        p0, psize = phase(log2n, name, 0)
        d = displacement(log2n, psize)
        chord = abs(np.exp(2j * np.pi * d / psize) - 1.0)
        for i in listed(log2n, entries, rng, count):
            probes = tuple([ps[j]] for j in np.flatnonzero(driven[:, i]))    # in turn: in a bin where a pair's two terms are
            p, _ = phase(log2n, name, i)
            moved = root(psize, p + d)
            # in phase, |1 - W| = |1 - conj W| hides a conjugated W from that pair
            assert detected(log2n, t, name, i, moved, probes), (log2n, name, i, "displaced", d)
            assert not np.isclose(abs(moved - t[name][i]), 0.0)
            counts[name, "displaced"] = counts.get((name, "displaced"), 0) + 1
            if abs(np.conj(t[name][i]) - t[name][i]) >= chord:
                assert detected(log2n, t, name, i, np.conj(t[name][i]), probes), (log2n, name, i, "conjugated")
                counts[name, "conjugated"] = counts.get((name, "conjugated"), 0) + 1
    print("log2n %d: D = %s; mutations seen: %s" % (log2n, {n: displacement(log2n, phase(log2n, n, 0)[1]) for n in sorted(read)},
                                                    ", ".join("%s %s %d" % (k[0], k[1], v) for k, v in sorted(counts.items()))))


@pytest.mark.parametrize("log2n", [17, 20])
def test_the_aggregate_bound_lets_a_gross_fault_pass(log2n):
    """a zeroed entry W of the untangling's table: X[k] = E - i W O loses its odd part.  Every pair a, -a (one impulse is
    E, the other O: the two bins k, M - k are wrong by 2 a^2 to 4 a^2 together) misses the per-bin bound.  The aggregate
    bound allows c M 2 a^2: at log2n 17 (c M = 1.7) it lets some of these very pairs pass, from c M >= 2 on (log2n 18)
    every one of them"""
    t = tables(log2n)
    some = cases.pairs(log2n)[:-1]                           # a, -a
    c_m = bounds(log2n)[0] * (1 << (log2n - 1))
    assert c_m >= (2.0 if log2n >= 18 else 1.0)
    k = int(np.random.default_rng(log2n).integers(1, 1 << (log2n - 2)))
    t["tw"][k] = 0.0
    p = run(some, log2n, t)
    assert all(s > 1.0 for s in shares(p, some, log2n))
    within = [aggregate_share(row, c, log2n) <= 1.0 for row, c in zip(p, some)]
    assert all(within) if log2n >= 18 else any(within), within
    print("log2n %d: tw[%d] zeroed: every pair outside the per-bin bound, %d of %d inside the aggregate one" % (log2n, k, sum(within), len(within)))
