"""The public surface of the ctypes binding (rtl-ws_amd/rtlws/__init__.py), pinned: every public name with its kind, the
signature of every public function and of every public method of Engine and of the plan classes, and the ctypes
prototypes each library's functions carry once its loader has run.

tests/golden/python_api.json was RECORDED FROM COMMIT 7394e4f ("Periodicity searches: one rule set, one plan, one host
driver"), when every library still had its own loader, error reader and hand-kept symbol list.  However the module is
arranged afterwards, a caller sees the same names, the same arguments and defaults, and a C function gets its arguments
converted the same way.  One difference is allowed: five functions of librtlws_hip.so had no complete prototype then;
they may carry the one include/rtlws_hip.h declares, which is asserted here against the header's text.

A function without argtypes passes a pointer as a C int; so every function of a satellite's symbol list must come from
its prototype table, which the last test asserts."""
import ctypes
import inspect
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "python_api.json")
SATELLITES = ("long", "anylen", "fm", "ddc", "ddcfir", "fmbank", "fmfir", "pfb", "pfbspec", "pfbxc", "pfbbf", "pfbsk",
              "dedisp", "pulse", "fold", "period", "periodlong", "accel")
# librtlws_hip.so's functions that may gain the prototype of include/rtlws_hip.h: name -> (argtypes, restype)
HIP_COMPLETED = {
    "rtlws_device_count": ([], "c_int"),
    "rtlws_device_pci_bus_id": (["c_int", "c_char_p", "c_int"], "c_int"),
    "rtlws_last_error": ([], "c_char_p"),
    "rtlws_event_create": ([], "c_void_p"),
    "rtlws_event_create_blocking": ([], "c_void_p"),
}
C_TYPES = {"int": "c_int", "void*": "c_void_p", "char*": "c_char_p", "const char*": "c_char_p"}


def _kind(value):
    if inspect.isclass(value):
        return "class"
    if inspect.isfunction(value):
        return "function"
    if inspect.ismodule(value):
        return "module"
    return type(value).__name__


def _plans(rtlws):
    out, todo = [], [rtlws._Plan]
    while todo:
        cls = todo.pop()
        out.append(cls)
        todo += cls.__subclasses__()
    return sorted(out, key=lambda c: c.__name__)


def _methods(cls):
    out = {}
    for name in dir(cls):
        if not name.startswith("_"):
            raw = inspect.getattr_static(cls, name)
            out[name] = "property" if isinstance(raw, property) else str(inspect.signature(getattr(cls, name))) if callable(
                getattr(cls, name)) else _kind(raw)
    return out


def _prototype(fn):
    return [None if fn.argtypes is None else [t.__name__ for t in fn.argtypes], getattr(fn.restype, "__name__", "None")]


def snapshot(rtlws):
    """what the golden file holds, of the module as it is"""
    public = {n: v for n, v in vars(rtlws).items() if not n.startswith("_")
              and not (inspect.ismodule(v) and v.__name__.startswith(rtlws.__name__ + "."))}    # a submodule, once imported
    libs = {"hip": (rtlws.hip_lib(), rtlws.HIP_SYMBOLS)}
    for name in SATELLITES:
        libs[name] = (getattr(rtlws, name + "_lib")(), getattr(rtlws, name.upper() + "_SYMBOLS"))
    return {
        "names": {n: _kind(v) for n, v in sorted(public.items())},
        "functions": {n: str(inspect.signature(v)) for n, v in sorted(public.items()) if inspect.isfunction(v)},
        "methods": {cls.__name__: _methods(cls) for cls in [rtlws.Engine] + _plans(rtlws)},
        "prototypes": {lib: {f: _prototype(getattr(L, f)) for f in sorted(symbols)} for lib, (L, symbols) in libs.items()},
    }


def _recorded():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_the_record_is_the_parents():
    rec = _recorded()
    assert rec["recorded_from"].startswith("7394e4f")
    assert sorted(rec["prototypes"]) == sorted(SATELLITES + ("hip",)) and len(SATELLITES) == 18
    assert len(rec["functions"]) > 100 and len(rec["methods"]["Engine"]) == 37 and len(rec["methods"]) == 23
    assert all(rec["prototypes"]["hip"][f][0] is None for f in HIP_COMPLETED)


def test_names_and_signatures(built):
    rec, now = _recorded(), snapshot(built)
    for part in ("names", "functions", "methods"):
        assert now[part] == rec[part], part
    for name in rec["functions"]:
        assert getattr(built, name).__name__ == name
    for name in SATELLITES:
        assert ("librtlws_%s.so (include/rtlws_%s.h)" % (name, name)) in getattr(built, name + "_lib").__doc__


def test_prototypes(built):
    rec, now = _recorded()["prototypes"], snapshot(built)["prototypes"]
    for lib in rec:
        assert sorted(now[lib]) == sorted(rec[lib]), lib
        for f, proto in rec[lib].items():
            if lib == "hip" and f in HIP_COMPLETED and now[lib][f] != proto:
                assert now[lib][f] == list(HIP_COMPLETED[f]), f
            else:
                assert now[lib][f] == proto, (lib, f)


def test_the_completed_prototypes_are_the_headers():
    txt = open(os.path.join(ROOT, "include", "rtlws_hip.h")).read()
    for f, (argtypes, restype) in HIP_COMPLETED.items():
        m = re.search(r"^([a-z][a-z ]*?\*?)\s*%s\(([^)]*)\);" % f, txt, flags=re.M)
        assert m, f
        params = [] if m.group(2).strip() == "void" else [re.sub(r"\s*\w+$", "", p.strip()) for p in m.group(2).split(",")]
        assert [C_TYPES[p] for p in params] == argtypes and C_TYPES[m.group(1).strip()] == restype, f
        assert getattr(ctypes, restype) and all(getattr(ctypes, a) for a in argtypes)


def test_symbol_lists_are_the_tables(built):
    for name in SATELLITES:
        symbols, table = getattr(built, name.upper() + "_SYMBOLS"), getattr(built, "_%s_PROTOTYPES" % name.upper())
        assert set(symbols) == set(table) and len(symbols) == len(set(symbols)), name
        L = getattr(built, name + "_lib")()
        assert all(getattr(L, f).argtypes is not None for f in symbols), name
