"""The launch-table model (tests/kernel_matrix.py) against the built library's gfx950 code objects, both ways: every
spectrum instantiation the library holds is reached by a case of the model, and every case names an instantiation
the library holds.  So a new table entry cannot land without a case that tests/test_kernel_matrix_gpu.py runs
against the oracle, and a model that drifts from the tables fails here, without a GPU."""
import re

import kernel_matrix as km

SPECTRUM = ("spectra_fused", "spectra_fused_v2", "spectra_f64_fused", "spectra_f64_1024x", "spectra_f64",
            "spectra_direct")


def _arg(s):
    s = s.strip()
    return s == "true" if s in ("true", "false") else int(s)


def _library_kernels(built):
    """(spectrum instantiations as (name, args), other kernels by short name) of librtlws_hip.so."""
    from rtlws import codeobj
    spec, other = set(), []
    for k in codeobj.kernels(built.HIP_LIB):
        d = k.get("demangled", k["name"])
        m = re.match(r"^(?:void )?rtlws::(\w+)(<[^>]*>)?\(", d)
        assert m, d
        name, targs = m.group(1), m.group(2)
        if name in SPECTRUM:
            t = (name, tuple(_arg(a) for a in targs[1:-1].split(",")))
            assert t not in spec, d
            spec.add(t)
        else:
            other.append(name + (targs or ""))
    return spec, other


def test_every_spectrum_instantiation_has_a_case_and_every_case_an_instantiation(built):
    spec, _ = _library_kernels(built)
    modelled = {}
    for c in km.CASES:
        t = km.instantiation(c)
        assert t is not None, c.label()
        modelled.setdefault(t, []).append(c)
    untested = sorted(spec - set(modelled))
    phantom = sorted((t, [c.label() for c in modelled[t]]) for t in set(modelled) - spec)
    assert not untested, "instantiations no case reaches: %s" % untested
    assert not phantom, "cases that name no instantiation: %s" % phantom
    counts = {n: sum(1 for t in spec if t[0] == n) for n in SPECTRUM}
    print("%d spectrum instantiations, all matched by %d cases: %s" % (len(spec), len(km.CASES), counts))
    assert len(spec) == 650 and counts == {"spectra_fused": 306, "spectra_fused_v2": 24, "spectra_f64_fused": 300,
                                           "spectra_f64_1024x": 14, "spectra_f64": 3, "spectra_direct": 3}
    # one case per instantiation, apart from the runtime-only fields of the row-per-workgroup kernels
    extra = [c for t, cs in modelled.items() for c in cs[1:]]
    assert all(km.instantiation(c)[0] in ("spectra_direct", "spectra_f64") for c in extra), [c.label() for c in extra]


def test_the_other_kernels_are_a_named_list(built):
    _, other = _library_kernels(built)
    assert sorted(other) == sorted(km.OTHER_KERNELS), sorted(other)
    print("%d other kernels: %s" % (len(other), ", ".join(sorted(other))))


def test_model_restates_the_routing_rules():
    """Spot checks of the rules the model restates (rtlws_internal.h, shim.hip), so that a slip in the model
    shows as such and not as a library mismatch."""
    o = dict(km.DEFAULT_OPTS)
    assert [km.cic_in_kind(R, o) for R in km.CIC_DEFAULT] == [km.IN_CU8_CICR_LDS4, km.IN_CU8_CICR_LDS2,
                                                              km.IN_CU8_CICR_LDS1, km.IN_CU8_CIC8,
                                                              km.IN_CU8_CIC10, km.IN_CU8_CIC12]
    o["cic_direct"] = 1
    assert [km.cic_in_kind(R, o) for R in km.CIC_DIRECT] == [km.IN_CU8_CICR2, km.IN_CU8_CICR4, km.IN_CU8_CICR8,
                                                             km.IN_CU8_CICR16]
    assert km.cic_in_kind(8, o) == km.IN_CU8_CIC8 and km.cic_in_kind(2, km.DEFAULT_OPTS) == km.IN_CU8_CICR4
    c = km.Case(False, 4096, "cu8", 0, 1, "rect", "power_sum", 0, False, ())
    assert km.instantiation(c) == ("spectra_fused_v2", (4096, False, 0, True))
    assert km.instantiation(c._replace(K=2)) == ("spectra_fused", (4096, 0, False, 0, False))
    assert km.instantiation(c._replace(input="cs32")) == ("spectra_fused", (4096, 1, False, 0, False))
    c = km.Case(True, 1024, "cu8", 0, 2, "rect", "mean_db", 0, True, (("f64_x_waves", 8),))
    assert km.instantiation(c) == ("spectra_f64_fused", (1024, 0, False, 1, False, True))
    assert km.instantiation(c._replace(K=1)) == ("spectra_f64_1024x", (1, True, True, 8))
    assert km.instantiation(c._replace(K=1, output="payload_u8")) == ("spectra_f64_1024x", (2, True, False, 8))
    assert km.instantiation(c._replace(cic_r=3)) == ("spectra_f64", (0,))
    # every payload gain of the matrix reaches both clamps on the GPU test's rows; both occur
    gains = {c.gain_db for c in km.CASES if c.output == "payload_u8"}
    assert gains == set(km.PAYLOAD_GAINS)
