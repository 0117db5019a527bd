"""The host-in, host-out drivers of rtlws.Engine where no other suite looks: what they return when there is no work, and
what they leave behind when an allocation fails half way.

The drivers' ordinary results are pinned bit for bit by the libraries' own suites.  What one shared driver skeleton can
get wrong is the rest: an empty capture's stub, an output of no bytes that must not be downloaded, a preset buffer that
comes back whole, an optional row that is not allocated -- and the release of the plan and of every device buffer when
the k-th allocation raises.

(a) tests/golden/engine_drivers.json holds, per case, the dtype, the shape and the SHA-256 of every array a driver
returns (null where it returns None), or the exception's type and text where it raises.  It was RECORDED ON AN MI355X
FROM THE BUILD OF COMMIT 7394e4f ("Periodicity searches: one rule set, one plan, one host driver"), when every driver
still spelled its own skeleton out.  Every driver has one ordinary case at a small shape and one with no work; the six
whose output shape holds a count the caller may give (pfb, pfbspec, pfbsk, pfbxc, pfbbf, pfbbf_power) have one more with
that count -1, which the library's run refuses: the RuntimeError with the library's words is what the record holds, not
an error of numpy's over a shape, and test_negative_count_releases_everything sees the plan closed behind it.  Inputs
come from tests/helpers.py's counter hash alone, the taps from rtlws_pfb_design and rtlws_ddcfir_design (integer tables
the CPU suites pin), so no libm is in the fixture.

(b) For pulse, pfbxc, fm_bank and spectra_long, and for k = 1 .. the number of device buffers the driver makes, the
k-th of Engine.alloc / Engine.upload raises a RuntimeError between two library calls.  The driver must pass it on, every
DevBuf constructed during the call must be freed and every plan opened during it closed by then -- not by a later
__del__ -- and the next ordinary call must still reproduce its recorded digest."""
import hashlib
import json
import os

import numpy as np
import pytest

from helpers import hash_bytes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_drivers.json")
FILL = -12345.678
LOG2_M, T = 4, 2                                          # the polyphase cases: 16 channels, 2 taps a branch, hop M
WORDS = [0, 5]


def cu8(nsamples, seed):
    """uint8 [nsamples, 2] from the counter hash"""
    return hash_bytes(2 * nsamples, seed=seed).reshape(nsamples, 2)


def f32(shape, seed):
    """float32 of the hash's bytes read as int8: small integers, exact"""
    return hash_bytes(int(np.prod(shape)), seed=seed).view(np.int8).astype(np.float32).reshape(shape)


def _polyphase(rtlws, work, nframes=5, seed=11):
    """(capture, taps): nframes frames at hop M, or one sample fewer than a frame"""
    m = 1 << LOG2_M
    return cu8((nframes - 1) * m + T * m if work else T * m - 1, seed), rtlws.pfb_design(LOG2_M, T)


def _weights():
    """complex64 [B = 2, A = 2, M]: small integers in both parts"""
    w = hash_bytes(2 * 2 * 2 << LOG2_M, seed=31).astype(np.int32) % 7 - 3
    return (w[0::2] + 1j * w[1::2]).astype(np.complex64).reshape(2, 2, 1 << LOG2_M)


def _period_series():
    """float32 [2, 1024]: the hash as int8 plus a square wave, so that no whitening block is empty"""
    return f32((2, 1024), 71) + np.float32(24) * ((np.arange(1024) // 19) % 2 == 0).astype(np.float32)


def _spectra(eng, rtlws, work, **kw):
    return eng.spectra(cu8(4 * 1024, 1), 1024, k_avg=2, **kw)


def _spectra_long(eng, rtlws, work):
    return eng.spectra_long(cu8(2 << 14, 2), 1 << 14)


def _spectra_anylen(eng, rtlws, work):
    return eng.spectra_anylen(cu8(2 * 1000, 3), 1000)


def _ddc(eng, rtlws, work):
    return eng.ddc(cu8(300 * 8 if work else 0, 4), 8, WORDS)


def _ddcfir(eng, rtlws, work):
    return eng.ddcfir(cu8(299 * 8 + 32 if work else 31, 5), 8, rtlws.ddcfir_design(8, 32), WORDS)


def _pfb(eng, rtlws, work, layout, **count):
    iq, taps = _polyphase(rtlws, work)
    return eng.pfb(iq, LOG2_M, taps, layout=layout, **count)


def _pfbspec(eng, rtlws, work, output, **count):
    iq, taps = _polyphase(rtlws, work)
    return eng.pfbspec(iq, LOG2_M, taps, 2, output=output, **count)


def _pfbsk(eng, rtlws, work, sub_rows, **count):
    iq, taps = _polyphase(rtlws, work)
    return eng.pfbsk(iq, LOG2_M, taps, 2, 2, sub_rows=sub_rows, **count)


def _pfbxc(eng, rtlws, work, twice, **count):
    a, taps = _polyphase(rtlws, work, nframes=4, seed=12)
    b, _ = _polyphase(rtlws, work, nframes=4, seed=13)
    return eng.pfbxc([a, a] if twice else [a, b], LOG2_M, taps, 2, **count)


def _pfbbf(eng, rtlws, work, **count):
    a, taps = _polyphase(rtlws, work, seed=14)
    b, _ = _polyphase(rtlws, work, seed=15)
    return eng.pfbbf([a, b], _weights(), LOG2_M, taps, **count)


def _pfbbf_power(eng, rtlws, work, **count):
    a, taps = _polyphase(rtlws, work, seed=14)
    b, _ = _polyphase(rtlws, work, seed=15)
    return eng.pfbbf_power([a, b], _weights(), LOG2_M, taps, 2, **count)


def _fm_bank(eng, rtlws, work):
    return eng.fm_bank(cu8(3 * 20 * 8 if work else 0, 6), 8, WORDS, 20, np.zeros((2, rtlws.FM_STATE_FLOATS), np.float32))


def _fm_fir_bank(eng, rtlws, work):
    return eng.fm_fir_bank(cu8((3 * 20 - 1) * 8 + 32 if work else 0, 7), 8, rtlws.ddcfir_design(8, 32), WORDS, 20,
                           np.zeros((2, rtlws.FM_STATE_FLOATS), np.float32))


def _dedisp(eng, rtlws, work, **kw):
    delays = (hash_bytes(3 * 8, seed=8).astype(np.int32) % 6).reshape(3, 8)
    delays[0, 0], delays[2, 7] = 0, 5                     # delays 0 .. 5, both ends taken
    return eng.dedisp(f32((70 + 5, 8), 9), delays, nout=70 if work else 0, **kw)


def _pulse(eng, rtlws, work, **kw):
    return eng.pulse(f32((2, 150 + 7), 10), (1, 3, 8), 64, nout=150 if work else 0, **kw)


def _fold(eng, rtlws, work, **kw):
    steps = [rtlws.fold_step(p) for p in (7.5, 11.0, 13.25)]
    phases = hash_bytes(3 * 8, seed=16).view("<u8")
    return eng.fold(f32((2, 150), 17), steps, phases, 4, 64, nsamp=150 if work else 0, **kw)


def _period(eng, rtlws, work, **kw):
    return eng.period(_period_series(), 10, 5, 16, 64, 1, **kw)


# name -> (the driver's call, its keywords, whether it has a case with no work)
DRIVERS = {
    "spectra-f32": (_spectra, {}, False),
    "spectra-f64": (_spectra, {"f64": True}, False),
    "spectra-f64-rows_f32": (_spectra, {"f64": True, "rows_f32": True}, False),
    "spectra_long": (_spectra_long, {}, False),
    "spectra_anylen": (_spectra_anylen, {}, False),
    "ddc": (_ddc, {}, True),
    "ddcfir": (_ddcfir, {}, True),
    "pfb-channel": (_pfb, {"layout": "channel"}, True),
    "pfb-time": (_pfb, {"layout": "time"}, True),
    "pfbspec-power": (_pfbspec, {"output": "power"}, True),
    "pfbspec-payload": (_pfbspec, {"output": "payload"}, True),
    "pfbsk": (_pfbsk, {"sub_rows": False}, True),
    "pfbsk-sub_rows": (_pfbsk, {"sub_rows": True}, True),
    "pfbxc": (_pfbxc, {"twice": False}, True),
    "pfbxc-twice": (_pfbxc, {"twice": True}, True),
    "pfbbf": (_pfbbf, {}, True),
    "pfbbf_power": (_pfbbf_power, {}, True),
    "fm_bank": (_fm_bank, {}, True),
    "fm_fir_bank": (_fm_fir_bank, {}, True),
    "dedisp": (_dedisp, {}, True),
    "dedisp-fill": (_dedisp, {"out_stride": 80, "fill": FILL}, True),
    "pulse": (_pulse, {}, True),
    "pulse-no_moments": (_pulse, {"want_moments": False}, True),
    "pulse-fill": (_pulse, {"fill": FILL}, True),
    "fold": (_fold, {}, True),
    "fold-no_hits": (_fold, {"want_hits": False}, True),
    "fold-fill": (_fold, {"fill": FILL}, True),
    "period-fill": (_period, {"fill": FILL}, False),
    "period-no_rows": (_period, {"want_rows": False}, False),
}


# the drivers whose output shape holds a count the caller may give: name -> that keyword.  A count of -1 passes the
# driver's own assert (rtlws_*_samples_needed answers -1), so the refusal is the library's run, in its words.
COUNTS = {"pfb-channel": "nframes", "pfbspec-power": "nspectra", "pfbsk": "nspectra", "pfbxc": "nspectra", "pfbbf": "nframes",
          "pfbbf_power": "nspectra"}


def cases():
    """(driver, "work", "nowork" or "negative")"""
    return [(name, kind) for name, (_, _, nowork) in DRIVERS.items()
            for kind in ("work",) + (("nowork",) if nowork else ()) + (("negative",) if name in COUNTS else ())]


def case_id(case):
    return "%s-%s" % case


def run(eng, rtlws, case):
    fn, kw, _ = DRIVERS[case[0]]
    return fn(eng, rtlws, case[1] != "nowork", **kw, **({COUNTS[case[0]]: -1} if case[1] == "negative" else {}))


def digests(eng, rtlws, case):
    """what a case returns, as the golden file holds it"""
    try:
        got = run(eng, rtlws, case)
    except Exception as e:                                # what the parent raised is part of the record
        return {"raises": type(e).__name__, "text": str(e)}
    return [None if o is None else {"dtype": str(o.dtype), "shape": list(o.shape),
                                    "sha256": hashlib.sha256(np.ascontiguousarray(o).tobytes()).hexdigest()}
            for o in (got if isinstance(got, tuple) else (got,))]


def recorded():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_the_record_holds_every_case():
    rec = recorded()
    assert rec["recorded_from"].startswith("7394e4f")
    assert sorted(rec["cases"]) == sorted(case_id(c) for c in cases()) and len(rec["cases"]) == 57
    negative = {k: v for k, v in rec["cases"].items() if k.endswith("-negative")}
    assert len(negative) == 6 and all(v["raises"] == "RuntimeError" and "rtlws_" in v["text"] for v in negative.values())
    work = [v for k, v in rec["cases"].items() if k.endswith("-work")]
    assert all(isinstance(v, list) and all(o is None or int(np.prod(o["shape"])) > 0 for o in v) for v in work)
    nowork = [v for k, v in rec["cases"].items() if k.endswith("-nowork")]
    assert len(nowork) == 22 and all(isinstance(v, dict) or any(o is not None for o in v) for v in nowork)


def test_the_shapes_are_served(built):
    m = 1 << LOG2_M
    assert built.ddc_supported(8, 2) == 1 and built.ddcfir_supported(8, 32, 2) == 1
    assert built.pfb_supported(LOG2_M, T, m) == 1 and built.pfbspec_supported(LOG2_M, T, m, 2, "payload") == 1
    assert built.pfbsk_supported(LOG2_M, T, m, 2, 2) == 1 and built.pfbxc_supported(LOG2_M, T, m, 2, 2) == 1
    assert built.pfbbf_supported(LOG2_M, T, m, 2, 2) == 1
    assert built.fmbank_supported(8, 2, 20, 3) == 1 and built.fmfir_supported(8, 32, 2, 20, 3) == 1
    assert built.dedisp_supported(8, 3) == 1 and built.pulse_supported((1, 3, 8), 64) == 1
    assert built.fold_supported([built.fold_step(p) for p in (7.5, 11.0, 13.25)], [0, 0, 0], 4, 64) == 1
    assert built.period_supported(10, 5, 16, 64, 1) == 1
    assert built.long_supported(built.make_desc(1 << 14)) == 1 and built.anylen_supported(built.make_desc(1000)) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases(), ids=case_id)
def test_driver_returns_what_the_parent_returned(engine, built, case):
    assert digests(engine, built, case) == recorded()["cases"][case_id(case)]


# ---- (b) the k-th allocation fails: the error comes out, nothing stays allocated, the plan is closed ----
BUFFERS = {"pulse": 4, "pfbxc": 4, "fm_bank": 4, "spectra_long": 2}       # the device buffers each driver makes


class Refused(RuntimeError):
    pass


def watched(built, mp):
    """-> (every DevBuf constructed, every plan opened) from here on, through the patches of mp"""
    made, opened = [], []
    dev_init, plan_open = built.DevBuf.__init__, built._Plan._open

    def init(self, *args, **kwargs):
        made.append(self)
        self.ptr = None                                   # a constructor that raises leaves nothing behind
        dev_init(self, *args, **kwargs)

    def open_(self, *args, **kwargs):
        opened.append(self)
        plan_open(self, *args, **kwargs)

    mp.setattr(built.DevBuf, "__init__", init)
    mp.setattr(built._Plan, "_open", open_)
    return made, opened


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(COUNTS))
def test_negative_count_releases_everything(engine, built, monkeypatch, name):
    """the library's refusal comes out (its type and text: the recorded case), and by then nothing is left"""
    with monkeypatch.context() as mp:
        made, opened = watched(built, mp)
        with pytest.raises(RuntimeError, match="rtlws_"):
            run(engine, built, (name, "negative"))
        assert len(made) >= 2 and all(b.ptr is None for b in made), "a device buffer outlives the failed call"
        assert len(opened) == 1 and opened[0].h is None, "the plan outlives the failed call"


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", [(name, k) for name, n in BUFFERS.items() for k in range(1, n + 1)])
def test_kth_allocation_fails(engine, built, monkeypatch, name, k):
    case = (name, "work")
    state = {"calls": 0, "inside": False}

    def counted(orig):
        """orig, raising on the k-th call of alloc / upload (an upload that goes through alloc counts once)"""
        def call(self, *args, **kwargs):
            if state["inside"]:
                return orig(self, *args, **kwargs)
            state["calls"] += 1
            if state["calls"] == k:
                raise Refused("allocation %d refused" % k)
            state["inside"] = True
            try:
                return orig(self, *args, **kwargs)
            finally:
                state["inside"] = False
        return call

    with monkeypatch.context() as mp:
        mp.setattr(built.Engine, "alloc", counted(built.Engine.alloc))
        mp.setattr(built.Engine, "upload", counted(built.Engine.upload))
        made, opened = watched(built, mp)
        with pytest.raises(Refused, match="allocation %d refused" % k):
            run(engine, built, case)
        assert len(made) == k - 1 and state["calls"] == k
        assert all(b.ptr is None for b in made), "a device buffer outlives the failed call"
        assert len(opened) == 1 and opened[0].h is None, "the plan outlives the failed call"
    assert digests(engine, built, case) == recorded()["cases"][case_id(case)]
