"""include/rtlws_cand.h restated in numpy as plain loops -- the yardstick of tests/test_cand_gpu.py, whose own properties
tests/test_cand_cpu.py holds.

  phase_c(n) = (phi0_c + n step_c) mod 2^64;  bin_c(n) = (((phase_c(n) >> 32) nbins) >> 32)          (fold_ref's)
  cube[c][s][i][b] = the f32 sum, ascending n, of S[n + delays[c][i]][i] over the n of sub-integration s that fall in bin b
  T[c][q][s][b]    = the f32 sum, ascending i, of cube[c][s][i][(b + a[c][q][i]) mod nbins]
  P[c][q][r][b]    = the f32 sum, ascending s, of T[c][q][s][(b + g[c][r][s]) mod nbins]
  stat, total      = the f64 sums, ascending b, of P_b^2 and of P_b

cube_ref and search_ref walk the index the order is defined over (n, then i, then s, then b) in a Python loop and add
one numpy vector per step over the indices the order does not depend on: every element sees its own additions one at a
time, each rounded once.  The *_by_the_letter forms are the same in scalars, for the small cases that hold the two to
each other.
"""
import numpy as np

from fold_ref import TWO64, bins_of, phase_at, step_of, subints          # noqa: F401  (the phase arithmetic is rtlws_fold.h's)

MAX_CANDS, MIN_NCHAN, MAX_NCHAN, MAX_DELAY, MIN_BINS, MAX_BINS = 64, 4, 4096, 65535, 2, 256
MIN_SUB, MAX_SUB, MAX_NSAMP, MAX_NSUB, MAX_NDM, MAX_NTR, MAX_WORKSPACE = 16, 1 << 24, 1 << 30, 1024, 256, 4096, 1 << 30
WAVES, CHUNK = 8, 32       # trials a workgroup and rows a chunk of the refinement's stages
KDM = 4.148808e3           # s MHz^2 cm^3 / pc


def waves_per_block(nbins):
    return 4 if nbins <= 64 else 2 if nbins <= 128 else 1


def fold_plan(ncand, nchan, nbins, sub, nsamp):
    """(workgroups, threads, lds_bytes, waves_per_block, nsub) as the header words it"""
    wpb, nsub = waves_per_block(nbins), subints(nsamp, sub)
    return ncand * nsub * -(-nchan // (64 * wpb)), 64 * wpb, wpb * nbins * 256, wpb, nsub


def search_plan(ncand, nsub, nchan, nbins, ndm, ntr):
    """(workgroups of stage 1, of stage 2, threads, lds_bytes of stage 1, of stage 2, workspace bytes)"""
    return (ncand * nsub * -(-ndm // WAVES), ncand * ndm * -(-ntr // WAVES), 64 * WAVES, CHUNK * nbins * 4, (CHUNK + WAVES) * nbins * 4,
            ncand * ndm * nsub * nbins * 4)


def _kept(nchan, mask):
    return np.ones(nchan, bool) if mask is None else np.asarray(mask)[:nchan] != 0


def _delays(ncand, nchan, delays):
    return np.zeros((ncand, nchan), np.int64) if delays is None else np.asarray(delays, np.int64).reshape(ncand, nchan)


def rows_needed(ncand, nchan, delays, mask, nsamp):
    """nsamp + the largest delay over the channels the mask keeps and all candidates; 0 for nsamp == 0"""
    keep = _kept(nchan, mask)
    most = int(_delays(ncand, nchan, delays)[:, keep].max()) if keep.any() else 0
    return nsamp + most if nsamp else 0


def cube_ref(rows, steps, phases, nchan, nbins, sub, nsamp, delays=None, mask=None):
    """(cube float32 [ncand, nsub, nchan, nbins], hits uint32 [ncand, nsub, nbins]) of rows float32 [nrows, >= nchan]: a loop
    over n, one vector of the kept channels' delayed samples added to the row of bin_c(n).  Nothing of a masked channel,
    nothing at or beyond nchan and no row behind rows_needed is looked at"""
    rows = np.asarray(rows, np.float32)
    ncand, nsub = len(steps), subints(nsamp, sub)
    d, keep = _delays(ncand, nchan, delays), _kept(nchan, mask)
    chans = np.flatnonzero(keep)
    cube = np.zeros((ncand, nsub, nchan, nbins), np.float32)
    hits = np.zeros((ncand, nsub, nbins), np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(ncand):
            for s in range(nsub):
                n0, n1 = s * sub, min((s + 1) * sub, nsamp)
                b = bins_of(steps[c], phases[c], nbins, n0, n1)
                acc = np.zeros((nbins, chans.size), np.float32)
                for n in range(n0, n1):
                    acc[b[n - n0]] = acc[b[n - n0]] + rows[n + d[c, chans], chans]
                cube[c, s, chans] = acc.T
                hits[c, s] = np.bincount(b, minlength=nbins)
    return cube, hits


def cube_by_the_letter(rows, step, phi0, nchan, nbins, n0, n1, delays=None, mask=None, order=None):
    """one candidate, one sub-integration (samples n0 .. n1 - 1) in scalars: float32 [nchan, nbins] and the hits; order: the
    n in the order they are added (None: ascending)"""
    d, keep = _delays(1, nchan, delays)[0], _kept(nchan, mask)
    acc = [[np.float32(0.0)] * nbins for _ in range(nchan)]
    count = [0] * nbins
    with np.errstate(invalid="ignore", over="ignore"):
        for n in (range(n0, n1) if order is None else order):
            b = ((((int(phi0) + n * int(step)) % TWO64) >> 32) * nbins) >> 32
            count[b] += 1
            for i in range(nchan):
                if keep[i]:
                    acc[i][b] = np.float32(acc[i][b] + np.float32(rows[n + d[i]][i]))
    return np.array(acc, np.float32), np.array(count, np.uint32)


def search_ref(cube, a, g):
    """(stat, total float64 [ncand, ndm, ntr], P float32 [ncand, ndm, ntr, nbins], T float32 [ncand, ndm, nsub, nbins]) of
    cube float32 [ncand, nsub, nchan, nbins], a int [ncand, ndm, nchan], g int [ncand, ntr, nsub]: loops over i, then s,
    then b; the vectors run over (s, b), (r, b) and the trials"""
    cube = np.asarray(cube, np.float32)
    ncand, nsub, nchan, nbins = cube.shape
    a, g = np.asarray(a, np.int64), np.asarray(g, np.int64)
    ndm, ntr = a.shape[1], g.shape[1]
    b = np.arange(nbins)
    T = np.zeros((ncand, ndm, nsub, nbins), np.float32)
    P = np.zeros((ncand, ndm, ntr, nbins), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(ncand):
            for q in range(ndm):
                acc = np.zeros((nsub, nbins), np.float32)
                for i in range(nchan):
                    acc = acc + cube[c, :, i][:, (b + a[c, q, i]) % nbins]
                T[c, q] = acc
                acc = np.zeros((ntr, nbins), np.float32)
                for s in range(nsub):
                    acc = acc + T[c, q, s, (b[None, :] + g[c, :, s, None]) % nbins]
                P[c, q] = acc
        stat, total = np.zeros((ncand, ndm, ntr)), np.zeros((ncand, ndm, ntr))
        P64 = P.astype(np.float64)
        for k in range(nbins):
            stat = stat + P64[..., k] * P64[..., k]
            total = total + P64[..., k]
    return stat, total, P, T


def search_by_the_letter(cube, a, g, chan_order=None, sub_order=None):
    """one candidate, one DM trial, one period trial in scalars: cube float32 [nsub, nchan, nbins], a int [nchan], g int
    [nsub] -> (stat, total, P float32 [nbins], T float32 [nsub, nbins]); the orders: the i and the s in the order they are
    added (None: ascending)"""
    nsub, nchan, nbins = cube.shape
    T = np.zeros((nsub, nbins), np.float32)
    P = np.zeros(nbins, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(nsub):
            for b in range(nbins):
                acc = np.float32(0.0)
                for i in (range(nchan) if chan_order is None else chan_order):
                    acc = np.float32(acc + cube[s][i][(b + int(a[i])) % nbins])
                T[s][b] = acc
        for b in range(nbins):
            acc = np.float32(0.0)
            for s in (range(nsub) if sub_order is None else sub_order):
                acc = np.float32(acc + T[s][(b + int(g[s])) % nbins])
            P[b] = acc
        stat, total = np.float64(0.0), np.float64(0.0)
        for b in range(nbins):
            stat = stat + np.float64(P[b]) * np.float64(P[b])
            total = total + np.float64(P[b])
    return stat, total, P, T


def chi2(stat, total, nbins, bin_variance):
    if nbins < 2 or not bin_variance > 0:
        return np.nan
    return (np.float64(stat) - np.float64(total) * np.float64(total) / nbins) / ((nbins - 1) * np.float64(bin_variance))


# ---- the helpers in extended precision: what is rounded, before the rint ----

def frequencies_mhz(nchan, shifted, f_centre_hz, bandwidth_hz):
    L = np.longdouble
    i = np.arange(nchan)
    c = (i + nchan // 2) % nchan if shifted else i
    return (L(f_centre_hz) + np.where(c < nchan // 2, c, c - nchan).astype(L) * L(bandwidth_hz) / L(nchan)) / L(1e6)


def dm_delay_rows(nchan, shifted, f_centre_hz, bandwidth_hz, row_seconds, ddm):
    """dt_i(dDM) in rows against the highest channel, longdouble [nchan]"""
    L = np.longdouble
    nu = frequencies_mhz(nchan, shifted, f_centre_hz, bandwidth_hz)
    return L(KDM) * L(ddm) * (1 / (nu * nu) - 1 / (nu.max() * nu.max())) / L(row_seconds)


def dm_shift_quotients(nchan, shifted, f_centre_hz, bandwidth_hz, row_seconds, period_rows, nbins, ndm, ddm0, ddm_step):
    """nbins dt_i(dDM_q) / period, longdouble [ndm, nchan]"""
    L = np.longdouble
    return np.stack([L(nbins) * dm_delay_rows(nchan, shifted, f_centre_hz, bandwidth_hz, row_seconds, L(ddm0) + L(q) * L(ddm_step)) / L(period_rows)
                     for q in range(ndm)])


def drift_shift_quotients(nbins, sub, nsub, nf, df0, df_step, nfd=1, dfd0=0.0, dfd_step=0.0):
    """nbins (df t_s + dfd t_s^2 / 2) at t_s = (s + 1/2) sub, longdouble [nfd * nf, nsub], the frequency index fastest"""
    L = np.longdouble
    t = (np.arange(nsub).astype(L) + L(0.5)) * L(sub)
    out = np.zeros((nfd * nf, nsub), L)
    for k in range(nfd):
        for j in range(nf):
            out[k * nf + j] = L(nbins) * ((L(df0) + L(j) * L(df_step)) * t + (L(dfd0) + L(k) * L(dfd_step)) * t * t / L(2))
    return out


def reduced(quotients, nbins):
    """rint(v) mod nbins into 0 .. nbins - 1, and whether v is safely away from a tie (a double's error cannot turn it)"""
    r = np.rint(quotients)
    away = np.abs(np.abs(quotients - np.floor(quotients)) - 0.5) > 1e-6 * np.maximum(1.0, np.abs(quotients).astype(np.float64))
    return (r.astype(np.int64) % nbins).astype(np.int32), away


# ---- what the suites share ----

def gaussian_cube(ncand, nsub, nchan, nbins, seed):
    """float32, both signs, exponents over 2^-6 .. 2^6: another order of a sum's additions shows in its bits"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((ncand, nsub, nchan, nbins)) * np.exp2(rng.integers(-6, 7, (ncand, nsub, nchan, nbins)))).astype(np.float32)


def shift_table(shape, nbins, seed):
    """int32 shifts 0 .. nbins - 1 with both ends present"""
    t = np.random.default_rng(seed).integers(0, nbins, shape).astype(np.int32)
    t.reshape(-1)[0], t.reshape(-1)[-1] = 0, nbins - 1
    return t


# The synthetic pulsar of the recovery tests: 64 channels, 4096 samples, folded a little off in DM and in frequency
PULSAR = dict(nchan=64, shifted=1, f_centre_hz=400e6, bandwidth_hz=100e6, row_seconds=1e-3, nsamp=4096, sub=256, nbins=32,
              period=50.3, dm_fold=20.0, ndm=9, ddm0=-2.0, ddm_step=0.5, q_true=7, nf=9, r_true=6, amplitude=3.0, seed=2027)
PULSAR["df_step"] = 0.25 / PULSAR["nsamp"]                    # a quarter of a turn over the run per step
PULSAR["df0"] = -4 * PULSAR["df_step"]


def pulsar_rows(delays_fold):
    """(rows float32 [nsamp + max delay, nchan], the step the cube is folded at): unit noise and a pulse one row wide every
    1 / f_true rows, f_true = 1 / period - (df0 + r_true df_step) (the fold is that much too fast: the pulse drifts forward
    through the folded phase at df turns per row), dispersed at dm_fold + ddm0 + q_true ddm_step; the fold is
    at `period` and at delays_fold (rtlws_dedisp_delays at dm_fold)"""
    p = PULSAR
    rng = np.random.default_rng(p["seed"])
    nrows = p["nsamp"] + int(np.max(delays_fold))
    rows = rng.standard_normal((nrows, p["nchan"])).astype(np.float32)
    f_true = 1.0 / p["period"] - (p["df0"] + p["r_true"] * p["df_step"])
    dm_true = p["dm_fold"] + p["ddm0"] + p["q_true"] * p["ddm_step"]
    late = dm_delay_rows(p["nchan"], p["shifted"], p["f_centre_hz"], p["bandwidth_hz"], p["row_seconds"], dm_true).astype(np.float64)
    for i in range(p["nchan"]):
        at = np.rint(np.arange(0.25 / f_true, nrows - late[i] - 1, 1.0 / f_true) + late[i]).astype(np.int64)
        rows[at[at < nrows], i] += np.float32(p["amplitude"])
    return rows, step_of(p["period"])
