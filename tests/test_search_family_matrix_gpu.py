"""Every instantiation of the waterfall-and-series family's nine libraries, every form its kernels choose among at run
time and every geometry class of the cleaning and of the refinement, launched once.

tests/search_family_matrix.py lists the cases; tests/test_search_family_matrix_cpu.py holds that list to the libraries'
code objects.  Here each case runs through its own suite's checked path -- the helper that suite's tests call, with its NaN
padding and its preset guards -- so every output word is bit for bit the numpy restatement's (tests/*_ref.py); the coherent
dedispersion's voltages keep their two derived bounds (cdd_ref.shares), and its power rows are the bits of those voltages
squared and summed.  No comparison and no tolerance is new."""
import zlib

import numpy as np
import pytest

import cand_ref
import cdd_ref
import dedisp_ref
import ffa_ref
import fold_ref
import pulse_ref
import search_family_matrix as fm
import sift_ref
from test_cand_gpu import _fold as cand_fold, _search as cand_search, cand  # noqa: F401  (the fixtures of the suites)
from test_cdd_gpu import _gauss, _power as cdd_power, _tables, _volts, cdd  # noqa: F401
from test_clean_gpu import _check as clean_check, clean  # noqa: F401
from test_dedisp_gpu import _border_case as dedisp_case
from test_ffa_gpu import _run as ffa_run, ffa  # noqa: F401
from test_fold_gpu import _run as fold_run
from test_pulse_gpu import _run as pulse_run
from test_sift_gpu import _check as sift_check, sf  # noqa: F401
from test_subdedisp_gpu import _stage1_case, _stage2_case, sd  # noqa: F401

pytestmark = pytest.mark.gpu


def seed_of(c):
    return zlib.crc32(c.label().encode()) & 0xFFFF


def check_dedisp(c, request):
    dedisp_case(request.getfixturevalue("built"), request.getfixturevalue("engine"), c.plan)


def check_subdedisp(c, request):
    (_stage1_case if c.kernel == "subdedisp_subband_kernel" else _stage2_case)(request.getfixturevalue("sd"), request.getfixturevalue("engine"), c.plan)


def check_pulse(c, request):
    """two trials over two tiles and five outputs, segments of a tile and four: a partial last tile in the first segment,
    a last segment of one output and a little"""
    built = request.getfixturevalue("built")
    tile = pulse_ref.plan(c.plan)[0]
    assert built.pulse_geometry(c.plan, 64)[4] == tile
    nout = 2 * tile + 5
    x = pulse_ref.signed_series(2, pulse_ref.samples_needed(c.plan, nout), seed_of(c))
    pulse_run(built, request.getfixturevalue("engine"), x, c.plan, tile + 4, nout, name=c.label())


def check_fold(c, request):
    """two trials at 65 periods (a second group of wavefronts with one live lane), two tiles and five samples in
    sub-integrations of 68"""
    nbins, = c.plan
    steps, phases = fold_ref.table(65, seed_of(c))
    x = fold_ref.signed_series(2, 2 * fold_ref.TILE + 5, seed_of(c))
    fold_run(request.getfixturevalue("built"), request.getfixturevalue("engine"), x, steps, phases, nbins, 68, want_hits=c.form == "hits", name=c.label())


def check_cand(c, request):
    mod, engine = request.getfixturevalue("cand"), request.getfixturevalue("engine")
    if c.kernel == "cand_fold_kernel":
        # two candidates over 68 channels (a second wavefront of four live lanes), 230 samples in sub-integrations of 100
        nbins, = c.plan
        steps, phases = fold_ref.table(2, seed=seed_of(c), first=2.7 + nbins / 3.0, spread=11.3)
        delays = dedisp_ref.random_table(2, 68, 40, seed=nbins)
        x = dedisp_ref.signed_rows(230 + int(delays.max()), 68, seed=seed_of(c))
        cand_fold(mod, engine, x, steps, phases, nbins, 100, 230, delays, want_hits=c.form == "hits", name=c.label())
        return
    nbins, nsub, ndm, ntr, nchan = c.plan
    cube = cand_ref.gaussian_cube(2, nsub, nchan, nbins, seed_of(c))
    a, g = cand_ref.shift_table((2, ndm, nchan), nbins, seed_of(c) + 1), cand_ref.shift_table((2, ntr, nsub), nbins, seed_of(c) + 2)
    # stage 1's copy is the caller's T; stage 2's out the caller's P, which the case that is there for stage 2 asks for
    cand_search(mod, engine, cube, a, g, want_prof=c.form == "stage 2", want_tphase=c.form != "stage 1, no copy", name=c.label())


def check_ffa(c, request):
    """one base period; two trials but for the plan of three passes (320 000 samples a trial: one)"""
    p0, L, seg = c.plan
    x = ffa_ref.signed_series(1 if p0 << L > 1 << 16 else 2, p0 << L, seed_of(c))
    ffa_run(request.getfixturevalue("ffa"), request.getfixturevalue("engine"), x, p0, 1, L, fm.FFA_WIDTHS, seg, name=c.label())


def check_cdd(c, request):
    mod, engine = request.getfixturevalue("cdd"), request.getfixturevalue("engine")
    log2n, = c.plan
    if c.form != "voltages":
        cdd_power(mod, engine, log2n, "3", c.form)            # against the bits of that suite's own voltages of this N
        return
    n, nchan, nseg, lead, trail = 1 << log2n, 2, 2, 5, 11
    tables = _tables(mod, log2n, nchan, seed=seed_of(c), chirp_at=1)
    x = _gauss(nchan, cdd_ref.samples_needed(n, lead, trail, nseg), seed=seed_of(c) + 1)
    per_sample, per_segment = cdd_ref.shares(_volts(mod, engine, x, tables, lead, trail, nseg), x, tables, lead, trail, nseg)
    assert per_sample <= 1.0 and per_segment <= 1.0, (per_sample, per_segment)


def check_clean(c, request):
    """blocks of 32 rows over 80: two whole blocks and one of sixteen rows that looks back"""
    nchan, = c.plan
    x = dedisp_ref.pooled_rows(80, nchan, seed=seed_of(c))
    clean_check(request.getfixturevalue("clean"), request.getfixturevalue("engine"), x, 32, zerodm=c.form != "no zero-DM", name=c.label())


def check_sift(c, request):
    mod, engine = request.getfixturevalue("sf"), request.getfixturevalue("engine")
    if c.kernel == "sift_score_kernel":
        case = (np.full((1, 1, 1), 20.0, np.float32), np.full((1, 1, 1), 17, np.int32), sift_ref.flat_moments(1, 64, 64), np.array([2], np.int32), 64, 64)
        assert len(sift_check(mod, engine, case, 1.0, 0, 0, name=c.label())[0]) == 1
    elif c.kernel == "sift_box_kernel":
        sift_check(mod, engine, sift_ref.random_case(5, 3, 7, 1), 1.0, 32, 8, name=c.label())
    else:
        case = sift_ref.random_case(65, 2, 65, 2, blobs=25)
        want = sift_check(mod, engine, case, 2.0, 1, 1, name=c.label())[0]
        assert len(want) >= 4
        sift_check(mod, engine, case, 2.0, 1, 1, max_cand=len(want) // 2, name=c.label() + ", half")


CHECKS = {"dedisp": check_dedisp, "subdedisp": check_subdedisp, "pulse": check_pulse, "fold": check_fold, "ffa": check_ffa, "cdd": check_cdd,
          "cand": check_cand, "clean": check_clean, "sift": check_sift}


@pytest.mark.parametrize("c", fm.CASES, ids=[c.label() for c in fm.CASES])
def test_every_case(request, c):
    try:
        CHECKS[c.lib](c, request)
    except AssertionError as e:
        raise AssertionError("%s [%s]: %s" % (fm.spell(fm.instantiation(c)), c.label(), e)) from e
