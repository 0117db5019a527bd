"""The polyphase family's outputs on fixed inputs, pinned to the bit (rtlws_pfb.h, rtlws_pfbspec.h, rtlws_pfbxc.h,
rtlws_pfbbf.h).

The four libraries share one text of the bank's passes (csrc/pfb_tile.h), of its plan, rules and launch tables, and
the correlator and the beamformer restate the spectrometer's order of the K-frame sums (the slice loop, the in-order
combine of the slices through LDS, the (spectrum, bin) loop).  The SHA-256 digests in
tests/golden/pfb_family_sha256.json were RECORDED ON AN MI355X FROM THE BUILD OF COMMIT 0923e53 ("Polyphase beamformer:
1-4 weighted beams of 1-8 captures, one launch"), before the family's text was shared; whatever is moved between the
libraries' texts afterwards has to give the same bytes.  A digest that differs means an order, a rounding or a
contraction changed -- find which, a tolerance is not the answer.

Inputs come from integer arithmetic alone (tests/helpers.py's counter hash): the captures' bytes, int16 taps, beam
weights that are small integers over 64.  The shapes are the smallest at which every branch of the sums' text is
taken: T = 3 taps per branch, hop M / 2 unless noted, and
  log2 M = 4   F = 256 frames to a tile, 16 slices: the combine through LDS
  log2 M = 8   F = SLICE = 16: one slice
  log2 M = 10  F = 4, four items per thread
each with K = 3 (several spectra to a tile and a remainder -- at log2 M = 10 one spectrum and a remainder; one spectrum
more than a workgroup holds, so the last workgroup is ragged), K = F (one spectrum per workgroup in one tile
iteration, two spectra) and K = F + 1 (two iterations, the second ragged, two spectra): the spectrometer's raw sums,
its dB rows (K = 3, shifted) and payload bytes (K = F + 1, hop M), the correlator of three captures, the power of two
beams of three captures; and the channelizer's and two beams' voltages in both layouts, F + 1 frames from an odd first
frame."""
import hashlib
import json
import os

import numpy as np
import pytest

from helpers import hash_bytes

T = 3
LOG2_MS = (4, 8, 10)
K_KINDS = ("k3", "kF", "kF1")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pfb_family_sha256.json")


def k_and_spectra(log2_m, kind):
    """(K, nspectra) of a K kind at a bank of 2^log2_m channels."""
    f = 4096 >> log2_m
    if kind == "k3":
        return 3, f // 3 + 1
    return (f, 2) if kind == "kF" else (f + 1, 2)


def cases():
    out = []
    for k in LOG2_MS:
        for kind in K_KINDS:
            out += [("pfbspec", k, kind, "power"), ("pfbxc", k, kind, ""), ("pfbbf_power", k, kind, "")]
        out += [("pfbspec", k, "k3", "db"), ("pfbspec", k, "kF1", "payload")]
        out += [(lib, k, "volt", layout) for lib in ("pfb", "pfbbf") for layout in ("channel", "time")]
    return out


def case_id(case):
    return "-".join(str(x) for x in case if x != "")


def taps_of(log2_m):
    """int16 [T * M] from the counter hash, two bytes a tap."""
    return hash_bytes(2 * (T << log2_m), seed=100 + log2_m).view("<i2").astype(np.int16)


def captures_of(log2_m, nsamples):
    return [hash_bytes(2 * nsamples, seed=10 * log2_m + a).reshape(nsamples, 2) for a in range(3)]


def weights_of(log2_m):
    """complex64 [2, 3, M]: both parts integers -8 .. 8 over 64, exact in f32."""
    b = hash_bytes(2 * 2 * 3 << log2_m, seed=200 + log2_m).astype(np.int32) % 17 - 8
    w = b.reshape(2, 3, 1 << log2_m, 2).astype(np.float32) / np.float32(64)
    return np.ascontiguousarray(w[..., 0] + 1j * w[..., 1]).astype(np.complex64)


def output_bytes(eng, case):
    lib, k, kind, what = case
    m, f = 1 << k, 4096 >> k
    taps = taps_of(k)
    if kind == "volt":
        nframes, hop, first = f + 1, m // 2, 7
        iqs = captures_of(k, (nframes - 1) * hop + T * m)
        if lib == "pfb":
            outs = [eng.pfb(iqs[0], k, taps, hop=hop, first_frame_index=first, layout=what, nframes=nframes)]
        else:
            outs = [eng.pfbbf(iqs, weights_of(k), k, taps, hop=hop, first_frame_index=first, layout=what, nframes=nframes)]
    else:
        k_avg, nspectra = k_and_spectra(k, kind)
        hop = m if what == "payload" else m // 2
        iqs = captures_of(k, (nspectra * k_avg - 1) * hop + T * m)
        if lib == "pfbspec":
            outs = [eng.pfbspec(iqs[0], k, taps, k_avg, hop=hop, output=what, shifted=(what == "db"), scale=2.0 ** -20,
                                nspectra=nspectra)]
        elif lib == "pfbxc":
            outs = list(eng.pfbxc(iqs, k, taps, k_avg, hop=hop, nspectra=nspectra))
        else:
            outs = [eng.pfbbf_power(iqs, weights_of(k), k, taps, k_avg, hop=hop, nspectra=nspectra)]
    assert all(o.size > 0 for o in outs)
    return b"".join(np.ascontiguousarray(o).tobytes() for o in outs)


def digest(eng, case):
    return hashlib.sha256(output_bytes(eng, case)).hexdigest()


def test_inputs_are_fixed():
    taps, w, iq = taps_of(4), weights_of(4), captures_of(4, 64)
    assert taps.dtype == np.int16 and taps.shape == (48,) and len(set(taps.tolist())) > 40
    assert w.dtype == np.complex64 and w.shape == (2, 3, 16)
    assert np.array_equal(w.real * 64, np.rint(w.real * 64)) and np.abs(w.real).max() <= 0.125 and np.abs(w.imag).max() <= 0.125
    assert all(x.dtype == np.uint8 and x.shape == (64, 2) for x in iq) and not np.array_equal(iq[0], iq[1])
    with open(GOLDEN) as fh:
        recorded = json.load(fh)
    assert sorted(recorded["sha256"]) == sorted(case_id(c) for c in cases()) and len(recorded["sha256"]) == 45
    assert recorded["inputs_sha256"] == inputs_digest()


def inputs_digest():
    h = hashlib.sha256()
    for k in LOG2_MS:
        h.update(taps_of(k).tobytes())
        h.update(weights_of(k).tobytes())
        for x in captures_of(k, 100):
            h.update(x.tobytes())
    return h.hexdigest()


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases(), ids=case_id)
def test_output_bit_identical_to_the_per_library_text(engine, case):
    with open(GOLDEN) as fh:
        recorded = json.load(fh)["sha256"]
    assert digest(engine, case) == recorded[case_id(case)]
