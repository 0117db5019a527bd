"""What the GPU suites of the periodicity-search family (test_period_gpu.py, test_periodlong_gpu.py, test_accel_gpu.py,
test_period_family_digest_gpu.py) say the same way: the comparison by bits, the seeded noise, the padded series, the
unpacking of a run's flat buffers with their guards, the loop of the stage-1 bound and the check of everything behind
the power row against tests/period_ref.py.  A plain module, like period_ref.py beside it."""
import numpy as np

import period_ref

FILL = np.float32(-12345.678)
FILL_BITS = FILL.view(np.uint32)


def same_bits(got, want, what=None, nan_by_place=True):
    """bit for bit on uint32 views; with nan_by_place a NaN only has to lie where the other has one (the default NaN of
    the host's division and the device's may differ), without it (device against device) a NaN's bits count too"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)      # a slice's last axis need not be contiguous
    nan = np.isnan(want) if nan_by_place and got.dtype.kind == "f" else np.zeros(want.shape, bool)
    gnan = np.isnan(got) if nan_by_place and got.dtype.kind == "f" else nan
    bad = (gnan != nan) | (~nan & (got.view(np.uint32) != want.view(np.uint32)))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])


def noise(ntrials, nsamp, seed, mean=10.0, draw=np.float32):
    """mean + standard normal draws as float32; `draw` is the type the generator draws in (the short frames' suite has
    drawn in float64 since its first day, and its recorded figures are of those series)"""
    rng = np.random.default_rng(seed)
    return (mean + rng.standard_normal((ntrials, nsamp), dtype=draw)).astype(np.float32)


def padded(x, nsamp, wide):
    """x[:, :nsamp] in rows of nsamp rounded up to a multiple of 4 (12 more with `wide`), NaN behind nsamp -> (rows, stride)"""
    stride = (nsamp + 3) // 4 * 4 + (12 if wide else 0)
    out = np.full((x.shape[0], stride), np.nan, np.float32)
    out[:, :nsamp] = x[:, :nsamp]
    return out, stride


def unpack(outs, ntrials, levels, nseg, m, guard, name=None):
    """the four flat buffers of a run with `fill`: each as long as its output and the guard, the guard untouched ->
    (best, at, power, white) in their shapes"""
    n1, n2 = ntrials * levels * nseg, ntrials * m
    for o, n in zip(outs, (n1, n1, n2, n2)):
        assert o.shape == (n + guard,) and np.all(o[n:].view(np.uint32) == FILL_BITS), name
    best, at = outs[0][:n1].reshape(ntrials, levels, nseg), outs[1][:n1].reshape(ntrials, levels, nseg)
    assert at.dtype == np.int32
    return best, at, outs[2][:n2].reshape(ntrials, m), outs[3][:n2].reshape(ntrials, m)


def check_bare(bare, best, at, name=None):
    """the run with NULL rows: the rows' buffers as they were, the peaks those of the run with rows"""
    assert np.all(bare[2].view(np.uint32) == FILL_BITS) and np.all(bare[3].view(np.uint32) == FILL_BITS), name
    same_bits(bare[0][:best.size].reshape(best.shape), best, (name, "best without rows"))
    assert np.array_equal(bare[1][:at.size].reshape(at.shape), at), (name, "at without rows")


def check_bins(power_row, xs, ref, b1, name):
    """every bin of one trial within period_ref.bound_bin's allowance of the f64 spectrum `ref` -> the worst share"""
    share, k = period_ref.bin_share(power_row, xs, ref, b1)
    assert share <= 1.0, (name, "bin", k, share, float(power_row[k]), float(ref[k]))
    return share


def check_stage1(power, x, nsamp, c, b1, reference, worst_of, worst_bin_of, key, name, finite=None):
    """per trial sum |P^ - P| <= c sum P against reference(trial's samples, name) -> the f64 spectrum (which asserts the
    premises of that bound itself), and every bin within bound_bin's allowance (b1; no premise); the worst shares of the two
    bounds go into worst_of[key] and worst_bin_of[key], the aggregate one comes back"""
    worst, worst_bin = 0.0, 0.0
    for t in range(x.shape[0]):
        if finite is not None and not finite[t]:
            continue
        ref = reference(x[t, :nsamp], name)
        err = np.abs(power[t].astype(np.float64) - ref).sum()
        assert err <= c * ref.sum(), (name, t, err, c * ref.sum())
        if ref.sum() > 0:
            worst = max(worst, err / (c * ref.sum()))
        worst_bin = max(worst_bin, check_bins(power[t], x[t, :nsamp], ref, b1, (name, t)))
    worst_of[key] = max(worst_of.get(key, 0.0), worst)
    worst_bin_of[key] = max(worst_bin_of.get(key, 0.0), worst_bin)
    return worst


def check_behind(power, white, best, at, levels, norm, seg, klo, name):
    """stages 2 - 4 from the device's own rows"""
    same_bits(white, period_ref.whiten(power, norm), (name, "white"))
    want_best, want_at = period_ref.peaks(period_ref.sums(white, levels), seg, klo)
    same_bits(best, want_best, (name, "best"))
    assert np.array_equal(at, want_at), (name, "at", np.argwhere(at != want_at)[:5])
