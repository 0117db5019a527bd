"""CPU suite of include/rtlws_dedisp.h (librtlws_dedisp.so): the ABI, the kernels' resources from the code-object
metadata, the form a table gets, the refusals and the delay helper -- and the numpy restatement's own properties
(tests/dedisp_ref.py), which hold the yardstick of tests/test_dedisp_gpu.py rather than the code under test.  No GPU is
used."""
import os
import re
import subprocess

import numpy as np
import pytest

import dedisp_ref
from dedisp_ref import DELAY_SETS, LARGEST_DELAYS
from test_abi_cpu import INCLUDE, _declared_functions, _exported

TILE = 256
SMALL_LDS, BIG_LDS = 36 * 1024, 64 * 1024


def _cap(ntrials):
    """the most trials a workgroup takes for a table of ntrials: 8 from five on, 4 for three and four"""
    return 8 if ntrials >= 5 else 4 if ntrials >= 3 else ntrials


def test_dedisp_library_exports_its_header_and_nothing_else(built):
    built.dedisp_lib()
    declared = _declared_functions("rtlws_dedisp.h")
    assert len(declared) == 8
    assert _exported(built.DEDISP_LIB) == set(declared) == set(built.DEDISP_SYMBOLS)
    dyn = subprocess.run(["readelf", "-d", built.DEDISP_LIB], capture_output=True, text=True, check=True).stdout
    assert "librtlws_hip.so" in dyn and "$ORIGIN" in dyn
    txt = open(os.path.join(INCLUDE, "rtlws_dedisp.h")).read()
    for name, value in (("MIN_NCHAN", 4), ("MAX_NCHAN", 4096), ("MAX_TRIALS", 4096), ("MAX_DELAY", 65535)):
        assert re.search(r"#define RTLWS_DEDISP_%s %d\b" % (name, value), txt) and getattr(built, "DEDISP_" + name) == value
        assert getattr(dedisp_ref, name) == value


def _kernels(built):
    """{(trials, lone, big): metadata} of every kernel of the library"""
    from rtlws import codeobj
    built.dedisp_lib()
    names = {}
    for k in codeobj.kernels(built.DEDISP_LIB):
        d = k.get("demangled", k["name"])
        m = re.search(r"rtlws::dedisp::dedisp_kernel<(\d+), (false|true), (false|true)>", d)
        assert m, d
        names[(int(m.group(1)), m.group(2) == "true", m.group(3) == "true")] = k
    return names


def test_dedisp_kernels_do_not_spill(built):
    """Every kernel of the library: no scratch, no spilled register, 256 threads, at most 64 KiB of LDS and no more
    VGPRs and AGPRs than the workgroups its LDS admits per compute unit can have (128 at four, 256 at two); the kernel
    names are exactly the instantiations the launch table reaches."""
    names = _kernels(built)
    for key, k in names.items():
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, key
        assert not k.get("sgpr_spill_count", 0), key
        # four workgroups a compute unit in 36 KiB of LDS, two in 64 KiB: the registers must not be what holds fewer
        assert k["vgpr_count"] + (k.get("agpr_count") or 0) <= (256 if key[2] else 128), (key, k["vgpr_count"], k.get("agpr_count"))
        assert k["max_flat_workgroup_size"] == 256
        assert k["group_segment_fixed_size"] == (BIG_LDS if key[2] else SMALL_LDS) <= 65536, key
    assert set(names) == {(t, False, big) for t in (8, 4, 2, 1) for big in (False, True)} | {(1, True, False)}


def test_geometry_reports_the_code_objects_resources(built):
    """rtlws_dedisp_geometry's LDS and threads for tables of every form are those of a kernel of that many trials"""
    names = _kernels(built)
    seen = set()
    for ntrials, nchan, maxd in ((9, 64, 0), (9, 64, 5), (9, 64, 100), (9, 64, 240), (3, 64, 100), (2, 64, 0), (2, 20, 200), (1, 16, 0),
                                 (9, 64, 300), (9, 64, 1000), (1, 64, 3000), (9, 64, 5000), (2, 4, 65535)):
        d = dedisp_ref.random_table(ntrials, nchan, maxd, seed=maxd + 1) if maxd else np.zeros((ntrials, nchan), np.int32)
        rc, blocks, threads, lds, tile, per, most = built.dedisp_geometry(d, None, 1000)
        assert rc == 0 and tile == TILE and most == maxd and lds <= 65536, (ntrials, nchan, maxd)
        fits = [k for key, k in names.items() if key[0] == per and k["group_segment_fixed_size"] == lds]
        assert fits and all(k["max_flat_workgroup_size"] == threads == 256 for k in fits), (ntrials, nchan, maxd, per, lds)
        assert blocks == -(-1000 // tile) * -(-ntrials // per)
        seen.add((per, lds))
    assert seen >= {(8, SMALL_LDS), (8, BIG_LDS), (4, BIG_LDS), (2, SMALL_LDS), (2, BIG_LDS), (1, SMALL_LDS), (1, BIG_LDS)}, seen


def test_geometry_of_tables(built):
    geo = built.dedisp_geometry
    # all zero: the most trials a workgroup takes, nothing beyond nout read
    for nchan in (4, 16, 20, 64, 1024, 4096):
        for ntrials in (1, 2, 3, 4, 5, 7, 8, 9, 33, 4096 if nchan == 4 else 64):
            z = np.zeros((ntrials, nchan), np.int32)
            rc, blocks, threads, lds, tile, per, most = geo(z, None, 777)
            assert (rc, threads, lds, tile, per, most) == (0, 256, SMALL_LDS, TILE, _cap(ntrials), 0), (nchan, ntrials)
            assert blocks == -(-777 // TILE) * -(-ntrials // per)
    assert geo(np.zeros((8, 64), np.int32))[5] == 8 and geo(np.zeros((4096, 4096), np.int32))[5] == 8
    # blocks = ceil(nout / tile_out) ceil(ntrials / trials_per_block)
    d = dedisp_ref.delays(*DELAY_SETS[2])
    for nout in (0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, 1 << 20):
        rc, blocks, _, _, tile, per, most = geo(d, None, nout)
        assert rc == 0 and blocks == -(-nout // tile) * -(-33 // per) and most == 854
    # a degenerate table is served, by fewer trials a workgroup
    for ntrials, nchan in ((9, 64), (33, 1024), (2, 4), (7, 20)):
        for maxd in (300, 5000, 65535):
            rc, _, threads, lds, tile, per, most = geo(dedisp_ref.random_table(ntrials, nchan, maxd, seed=3), None, 10)
            assert (rc, threads, tile, per, most) == (0, 256, TILE, 1, maxd) and per < _cap(ntrials) and lds <= 65536
            assert built.dedisp_last_error() == ""
    # the sweeps keep whole groups
    for args, largest in zip(DELAY_SETS, LARGEST_DELAYS):
        rc, _, _, lds, _, per, most = geo(dedisp_ref.delays(*args), None, 100)
        assert rc == 0 and per >= 4 and most == largest, (args, per, most)
    # max_delay ignores what the mask leaves out; the spread of the plan does too
    d = np.zeros((9, 64), np.int32)
    d[:, 5], d[3, 40] = 60000, 17
    mask = np.ones(64, np.uint8)
    assert geo(d, None, 10)[5:] == (1, 60000)
    mask[5] = 0
    assert geo(d, mask, 10)[5:] == (8, 17)
    mask[40] = 0
    assert geo(d, mask, 10)[5:] == (8, 0)
    assert geo(d, np.zeros(64, np.uint8), 10)[5:] == (8, 0)
    # any pointer behind nout may be null
    assert built.dedisp_lib().rtlws_dedisp_geometry(64, 9, d.ctypes.data, None, 10, None, None, None, None, None, None) == 0


def test_dedisp_refusals_need_no_gpu(built):
    L = built.dedisp_lib()
    err = built.dedisp_last_error
    for nchan in (4, 8, 20, 1024, 4096):
        for ntrials in (1, 4096):
            assert built.dedisp_supported(nchan, ntrials) == 1 and err() == ""
    for nchan in (0, 3, 18, 4100, -4):
        assert built.dedisp_supported(nchan, 1) == 0 and err() == "rtlws_dedisp: nchan must be 4 .. 4096 and a multiple of 4", nchan
    for ntrials in (0, 4097, -1):
        assert built.dedisp_supported(64, ntrials) == 0 and err() == "rtlws_dedisp: ntrials must be 1 .. 4096", ntrials

    d = np.zeros((3, 16), np.int32)
    ptr = d.ctypes.data

    def geometry(nchan=16, ntrials=3, table=ptr, mask=None, nout=5):
        return L.rtlws_dedisp_geometry(nchan, ntrials, table, mask, nout, None, None, None, None, None, None), err()

    def opened(nchan=16, ntrials=3, table=ptr, mask=None):
        return L.rtlws_dedisp_open(None, nchan, ntrials, table, mask), err()

    for kw, word in (({"nchan": 0}, "nchan must be"), ({"nchan": 3}, "nchan"), ({"nchan": 18}, "nchan"), ({"nchan": 4100}, "nchan"),
                     ({"ntrials": 0}, "ntrials must be 1 .. 4096"), ({"ntrials": 4097}, "ntrials"), ({"table": None}, "null delays")):
        rc, why = geometry(**kw)
        assert rc == -1 and word in why and why.startswith("rtlws_dedisp_geometry: "), (kw, why)
        h, why = opened(**kw)
        assert not h and word in why and why.startswith("rtlws_dedisp_open: "), (kw, why)
    for bad in (-1, 65536):
        for at in ((0, 0), (2, 15), (1, 7)):
            d[:] = 0
            d[at] = bad
            for mask in (None, np.zeros(16, np.uint8).ctypes.data):                # also where the mask leaves it out
                rc, why = geometry(mask=mask)
                assert rc == -1 and why == "rtlws_dedisp_geometry: every delay must be 0 .. 65535", (bad, at)
                h, why = opened(mask=mask)
                assert not h and why == "rtlws_dedisp_open: every delay must be 0 .. 65535"
    d[:] = 65535
    assert geometry() == (0, "")
    assert geometry(nout=-1) == (-1, "rtlws_dedisp_geometry: nout must be >= 0")
    assert geometry(nout=1 << 62) == (-1, "rtlws_dedisp_geometry: more workgroups than one grid holds")
    h, why = opened()
    assert not h and why == "rtlws_dedisp_open: null engine (no usable HIP device: there is no CPU path)"
    with pytest.raises(RuntimeError):
        built.DedispPlan(None, d)
    with pytest.raises(RuntimeError):
        built.DedispPlan(None, d, np.ones(15, np.uint8))
    L.rtlws_dedisp_close(None)
    assert L.rtlws_dedisp_rows_needed(None, 5) == -1 and "null plan" in err()
    assert L.rtlws_dedisp_rows_needed(None, -1) == -1 and "nout must be >= 0" in err()

    A, B = 1 << 20, 2 << 20                                   # stand-ins for device pointers: never dereferenced
    base = (("plan", None), ("rows", A), ("istride", 64), ("nout", 100), ("out", B), ("ostride", 100), ("st", None))

    def run(**kw):
        assert set(kw) <= {k for k, _ in base}
        return L.rtlws_dedisp_run(*[kw.get(k, v) for k, v in base]), err()

    for kw, word in (({"nout": -1}, "nout must be >= 0"), ({"istride": 0}, "in_stride must be >= nchan"), ({"istride": 3}, "in_stride must be >="),
                     ({"istride": 66}, "in_stride must be a multiple of 4"), ({"ostride": 99}, "out_stride must be >= nout"),
                     ({"rows": None}, "null pointer"), ({"out": None}, "null pointer"), ({"rows": A + 4}, "d_rows must be 16-byte aligned"),
                     ({"rows": A + 8}, "d_rows must be 16-byte"), ({"out": B + 2}, "d_out must be 4-byte aligned"),
                     ({"out": B + 1}, "d_out must be 4-byte"), ({}, "null plan"), ({"out": B + 4}, "null plan"),
                     ({"nout": 0, "rows": None, "out": None, "ostride": 0}, "null plan"), ({"ostride": 1 << 40}, "null plan")):
        rc, why = run(**kw)
        assert rc == -1 and word in why and why.startswith("rtlws_dedisp_run: "), (kw, why)
    # the order: a call that breaks rule i and every later rule is refused for rule i
    chain = (({"nout": -1}, "nout"), ({"istride": 2}, "in_stride must be >="), ({"istride": 66}, "multiple of 4"), ({"ostride": 7}, "out_stride"),
             ({"out": None}, "null pointer"), ({"rows": A + 4}, "d_rows"), ({"out": B + 2}, "d_out"), ({}, "null plan"))
    for i, (_, word) in enumerate(chain):
        kw = {}
        for later, _ in reversed(chain[i:]):
            kw.update(later)
        rc, why = run(**kw)
        assert rc == -1 and word in why, (i, kw, why)
    # a refusal here leaves a sibling's error slot empty
    assert built.pfbspec_supported(6, 8, 64, 3) == 1
    assert run(nout=-1)[0] == -1 and err() != "" and built.pfbspec_last_error() == ""


@pytest.mark.parametrize("which", range(len(DELAY_SETS)))
def test_delays_are_the_formula(built, which):
    """rtlws_dedisp_delays against the formula in numpy.float64, entry for entry; an entry may be left out only where the
    f64 quotient lies within 1e-9 of a half-integer, and for these inputs none does."""
    args = DELAY_SETS[which]
    q = dedisp_ref.delay_quotients(*args)
    left_out = np.abs(np.abs(q - np.floor(q)) - 0.5) < 1e-9
    assert left_out.sum() == 0
    got = built.dedisp_delays(*args)
    want = np.rint(q).astype(np.int32)
    assert got.dtype == np.int32 and got.shape == (args[5], args[0]) and np.array_equal(got, want)
    assert got.max() == LARGEST_DELAYS[which]
    # properties of the tables: delays never decrease with the trial, the highest channel is never delayed, no DM no delay
    nchan, shifted = args[0], args[1]
    assert np.all(np.diff(got.astype(np.int64), axis=0) >= 0)
    top = nchan - 1 if shifted else nchan // 2 - 1
    assert np.all(got[:, top] == 0) and np.argmax(dedisp_ref.frequencies_mhz(*args[:4])) == top
    zero = built.dedisp_delays(*(args[:6] + (0.0, args[7])))
    assert not zero[0].any() and (args[7] == 0 or zero[-1].any())
    # shifted is a rotation of the table by half a row
    other = built.dedisp_delays(*((nchan, 1 - shifted) + args[2:]))
    assert np.array_equal(np.roll(other, nchan // 2, axis=1), got)


def test_delays_refusals(built):
    L = built.dedisp_lib()
    out = np.full((7, 16), -7, np.int32)
    base = (("nchan", 16), ("shifted", 0), ("fc", 1420.4e6), ("bw", 2.0e6), ("row", 1e-4), ("ntrials", 7), ("dm0", 10.0), ("step", 25.0),
            ("out", out.ctypes.data))

    def call(**kw):
        return L.rtlws_dedisp_delays(*[kw.get(k, v) for k, v in base]), built.dedisp_last_error()

    assert call() == (0, "") and out.max() == 9
    nan, inf = float("nan"), float("inf")
    for kw, word in (({"nchan": 18}, "nchan must be"), ({"ntrials": 0}, "ntrials must be"), ({"shifted": 2}, "shifted must be 0 or 1"),
                     ({"out": None}, "null delays"), ({"bw": 0.0}, "bandwidth_hz must be finite and > 0"), ({"bw": -1.0}, "bandwidth_hz"),
                     ({"bw": nan}, "bandwidth_hz"), ({"row": 0.0}, "row_seconds must be finite and > 0"), ({"row": inf}, "row_seconds"),
                     ({"fc": 0.0}, "frequency must be finite and > 0"), ({"fc": 1.0e6}, "frequency"), ({"fc": -5e6}, "frequency"),
                     ({"fc": nan}, "frequency"), ({"dm0": -1.0}, "trial 0: the dispersion measure must be finite and >= 0"),
                     ({"step": -3.0}, "trial 4: the dispersion measure"), ({"dm0": nan}, "trial 0"),
                     ({"row": 1e-10}, "trial 0: a delay above 65535 rows"), ({"dm0": 0.0, "row": 1e-9}, "trial 1: a delay above 65535 rows")):
        rc, why = call(**kw)
        assert rc == -1 and word in why and why.startswith("rtlws_dedisp_delays: "), (kw, why)
    with pytest.raises(RuntimeError):
        built.dedisp_delays(16, 0, 1420.4e6, 2.0e6, 1e-9, 7, 10.0, 25.0)
    # the lowest channel lies half the band below the centre: that one must be positive
    assert call(fc=2.0e6, row=100.0)[0] == 0 and call(fc=1.0e6, row=100.0)[0] == -1


# ---- the yardstick's own properties ---------------------------------------------------------------------------

def test_reference_on_itself():
    nchan, ntrials, nout = 20, 5, 37
    rows = dedisp_ref.hashed_rows(nout + 300, nchan + 4, seed=1)
    assert rows.dtype == np.float32 and rows.min() >= 0 and np.isfinite(rows).all()
    expo = np.frexp(rows[rows > 0])[1]
    assert expo.max() - expo.min() == 19                                          # twenty binades
    mask = dedisp_ref.random_mask(nchan, seed=2)
    assert 0 < mask.sum() < nchan
    # a zero table: each row's masked sum in the row's order, one f32 rounding a step
    z = np.zeros((ntrials, nchan), np.int32)
    for m in (None, mask):
        want = np.zeros(nout, np.float32)
        for i in range(nchan):
            if m is None or m[i]:
                want = want + rows[:nout, i]
        got = dedisp_ref.dedisp_ref(rows, z, m, nout)
        assert got.dtype == np.float32 and all(np.array_equal(got[t].view(np.uint32), want.view(np.uint32)) for t in range(ntrials))
    # the order shows in the bits: the same terms descending differ somewhere
    back = np.zeros(nout, np.float32)
    for i in reversed(range(nchan)):
        back = back + rows[:nout, i]
    assert not np.array_equal(back, dedisp_ref.dedisp_ref(rows, z, None, nout)[0])
    # one kept position: that column, delayed, bit for bit -- for non-negative data, as here: a kept -0.0 comes out +0.0
    # (test_reference_on_signed_and_special_rows)
    d = dedisp_ref.random_table(ntrials, nchan, 250, seed=3)
    for i in (0, 7, nchan - 1):
        got = dedisp_ref.dedisp_ref(rows, d, dedisp_ref.one_kept(nchan, i), nout)
        for t in range(ntrials):
            assert np.array_equal(got[t].view(np.uint32), rows[d[t, i]:d[t, i] + nout, i].view(np.uint32))
    assert dedisp_ref.rows_needed(d, None, nout) == nout + 250 and dedisp_ref.rows_needed(d, None, 0) == 0
    assert dedisp_ref.rows_needed(d, dedisp_ref.one_kept(nchan, 5), nout) == nout + d[:, 5].max()
    # nothing kept: +0.0
    none = dedisp_ref.dedisp_ref(rows, d, np.zeros(nchan, np.uint8), nout)
    assert not none.view(np.uint32).any()
    # nout None: what the rows hold; a run from row j0 on gives the outputs from j0 on
    full = dedisp_ref.dedisp_ref(rows, d)
    assert full.shape == (ntrials, rows.shape[0] - 250)
    assert np.array_equal(dedisp_ref.dedisp_ref(rows[3:], d), full[:, 3:])
    # the bound holds for the restatement, and is not idle
    for m in (None, mask):
        err = np.abs(dedisp_ref.dedisp_ref(rows, d, m, nout).astype(np.float64) - dedisp_ref.dedisp_f64(rows, d, m, nout))
        b = dedisp_ref.bound(rows, d, m, nout)
        assert np.all(err <= b) and 0 < (err / b).max() < 1


def _classes(out):
    """(subnormal and not zero, +Inf, -Inf, NaN, +0.0, -0.0) of a float32 array, as boolean arrays"""
    u = out.view(np.uint32)
    return (((u & 0x7F800000) == 0) & ((u & 0x007FFFFF) != 0), u == 0x7F800000, u == 0xFF800000, np.isnan(out), u == 0, u == 0x80000000)


def test_reference_on_signed_and_special_rows():
    """The inputs of tests/test_dedisp_gpu.py::test_signed_and_special_rows, through the restatement alone: signed_rows
    is hashed_rows with a sign, its sums cancel and keep the bound on the magnitudes; special_rows holds every class it
    says, and on each of the six tables the restatement's outputs hold subnormals, both infinities, NaN of Inf - Inf
    where no term is NaN, +0 of terms that are not zero, and never the bits of -0.0."""
    import dedisp_form_cases as forms
    plain, signed = dedisp_ref.hashed_rows(300, 36, seed=5), dedisp_ref.signed_rows(300, 36, seed=5)
    assert signed.dtype == np.float32 and np.array_equal(np.abs(signed).view(np.uint32), plain.view(np.uint32))
    assert 0.4 < np.signbit(signed).mean() < 0.6
    for which, case in enumerate(forms.SIX_FORMS):
        delays = forms.table(case)
        need = dedisp_ref.rows_needed(delays, None, forms.NOUT)
        rows = dedisp_ref.signed_rows(need, forms.NCHAN, seed=which + 1)
        got, got64 = dedisp_ref.dedisp_both(rows, delays, None, forms.NOUT)
        err, b = np.abs(got.astype(np.float64) - got64), dedisp_ref.bound(np.abs(rows), delays, None, forms.NOUT)
        assert np.all(err <= b) and 0 < (err / b).max() < 1
        assert (np.abs(got64) < 0.05 * b * 2.0 ** 24 / forms.NCHAN).any()         # cancellation: a sum far below its terms

        rows = dedisp_ref.special_rows(need, forms.NCHAN, seed=which + 1)
        assert rows.shape == (need, forms.NCHAN) and rows.dtype == np.float32
        assert all(c.any() for c in _classes(rows)), forms.case_id(case)
        assert np.array_equal(rows.view(np.uint32)[np.isnan(rows)], np.full(np.isnan(rows).sum(), 0x7FC00000, np.uint32))
        with np.errstate(invalid="ignore"):
            out = dedisp_ref.dedisp_ref(rows, delays, None, forms.NOUT)
        sub, pinf, ninf, nan, pzero, nzero = _classes(out)
        read_nan = dedisp_ref.dedisp_f64(np.isnan(rows).astype(np.float32), delays, None, forms.NOUT) > 0
        not_zero = dedisp_ref.dedisp_f64((rows != 0).astype(np.float32), delays, None, forms.NOUT) > 0
        counts = tuple(int(c.sum()) for c in (sub, pinf, ninf, nan & ~read_nan, pzero & not_zero, nzero))
        print("%s: subnormal %d, +Inf %d, -Inf %d, NaN of Inf - Inf %d, +0 of cancellation %d, -0 %d of %d outputs"
              % ((forms.case_id(case),) + counts + (out.size,)))
        # one trial a workgroup delays a position of every output: a row's pairs then cancel only by chance
        assert all(counts[:4]) and (counts[4] or case.plan_per == 1) and counts[5] == 0, (forms.case_id(case), counts)
        assert read_nan.any() and np.all(nan[read_nan]) and np.isfinite(out).mean() > 0.5
    # the header's acc = +0.0f start: one kept position holding -0.0 gives +0.0, not that column bit for bit
    rows = np.full((5, 4), -0.0, np.float32)
    out = dedisp_ref.dedisp_ref(rows, np.zeros((2, 4), np.int32), dedisp_ref.one_kept(4, 2), 5)
    assert np.signbit(rows).all() and not out.view(np.uint32).any()


def test_tables_of_the_suites():
    d = dedisp_ref.random_table(9, 64, 300, seed=4)
    assert d.shape == (9, 64) and d.dtype == np.int32 and d.min() == 0 and d.max() == 300 and (d[0, 0], d[0, 1]) == (0, 300)
    m = dedisp_ref.mixed_table(33, 64, seed=5)
    assert m[:8].max() <= 7 * 8 and np.all(np.diff(m[:8].astype(int), axis=0) >= 0) and m[8:].max() > 4000
    assert m[0].max() == 0 and m[7, 0] == 7 * 63 // 8


def test_tile_layout_is_conflict_free():
    """tools/lds_sim.py's bank model on dedisp.hip's tile: the transposing stores and the sums' reads take their ideal
    two LDS cycles per wavefront instruction in every form of the plan; a stride that is not of the rule's form does not."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(INCLUDE), "tools"))
    argv, sys.argv = sys.argv, ["lds_sim"]
    try:
        import lds_sim
    finally:
        sys.argv = argv
    res = lds_sim.analyse_dedisp(verbose=False)
    assert len(res) == 6 * 4 + 1 and all(v == (2, 2) for v in res.values()), res
    for height, quads, want in ((256, 8, 257), (257, 8, 257), (258, 8, 259), (556, 4, 558), (1256, 2, 1260), (3756, 1, 3756)):
        assert lds_sim.dedisp_stride(height, quads) == want
    # the rule written out in csrc/dedisp.h is the model's
    txt = open(os.path.join(os.path.dirname(INCLUDE), "rtl-ws_amd", "csrc", "dedisp.h")).read()
    assert "const int unit = quads > 1 ? 8 / quads : 1;" in txt and "if (quads > 1 && s % 2 == 0) ++s;" in txt
    bad = lds_sim.cycles_b32([(4 * (t % 8)) * 256 + t // 8 for t in range(64)])
    assert bad == 16                                       # eight quads at a stride of 256: every column on the same banks
