"""The signature table of the Python binding (generalized_rbda_amd/_abi.py) against include/grbda_hip.h, parameter by parameter.

ctypes cannot see a prototype: a function without `argtypes` takes a Python int as a 32-bit int (wrong for size_t B and for addresses),
and a table that disagrees with the header passes garbage without a word.  So every prototype of the header is parsed here and held
against the table -- parameter count, the scalar class at each position, pointer or not, the return kind -- and the loaded library
against the table.  The comparison itself is shown to fail on four seeded defects.  No device call is made."""
import ctypes
import os
import re
from ctypes import c_char_p, c_double, c_int, c_size_t, c_void_p

import pytest

import generalized_rbda_amd as G
from generalized_rbda_amd._abi import SIGNATURES

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "grbda_hip.h")
SCALARS = {"int": c_int, "size_t": c_size_t, "double": c_double}
RETURNS = {"int": c_int, "const char *": c_char_p, "void": None}


def header_prototypes():
    """name -> (return type, [(parameter kind, parameter name)]): kind is "pointer" for anything with * or [n], else the scalar's type"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = {}
    for ret, name, args in re.findall(r"^([\w \*]+?)\s*\b(grbda_\w+)\s*\(([^()]*)\)\s*;", text, flags=re.M):
        params = []
        for a in (a.strip() for a in args.split(",")):
            if a == "void":
                continue
            *kind, pname = re.sub(r"\[\w*\]", "", a).replace("*", " ").split()
            params.append(("pointer" if "*" in a or "[" in a else " ".join(kind), pname))
        protos[name] = (ret.strip(), params)
    return protos


def table_kind(t):
    if t in (c_void_p, c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return "pointer"
    return next(name for name, c in SCALARS.items() if t is c)


def compare(table, protos):
    """asserts that `table` declares what the header's prototypes do"""
    assert set(table) == set(protos), set(table) ^ set(protos)
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert restype is RETURNS[ret], f"{name}: returns {ret}, the table says {restype}"
        assert len(argtypes) == len(params), f"{name}: {len(params)} parameters, the table has {len(argtypes)}"
        for i, ((kind, pname), t) in enumerate(zip(params, argtypes)):
            assert table_kind(t) == kind, f"{name}: parameter {i} ({pname}) is {kind}, the table says {t.__name__}"


PROTOS = header_prototypes()


def test_the_header_parse_finds_every_prototype():
    assert len(PROTOS) == 96
    assert PROTOS["grbda_last_error"] == ("const char *", []) and PROTOS["grbda_plan_free"][0] == "void"
    assert PROTOS["grbda_plan_set_gravity"][1] == [("pointer", "plan"), ("pointer", "g")]  # (const double g[3])
    assert PROTOS["grbda_kernel_name"][1][3] == ("size_t", "B") and PROTOS["grbda_fd_dq_f32"][1][4] == ("double", "step")


def test_the_table_declares_what_the_header_does():
    compare(SIGNATURES, PROTOS)
    assert G.C_ABI_SYMBOLS == list(SIGNATURES) and len(set(G.C_ABI_SYMBOLS)) == 96


def test_the_loaded_library_carries_the_table(monkeypatch):
    monkeypatch.setattr(G, "_lib", None)  # (a fresh load: other tests set argtypes of their own on the shared one)
    L = G.lib()
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and tuple(fn.argtypes) == tuple(argtypes), name
        assert fn.restype is restype, name
    assert len(L.grbda_contact_impulse_f64.argtypes) == 14


def _position(name, pname):
    return [p for _, p in PROTOS[name][1]].index(pname)


def _dropped(t):
    t["grbda_aba_f64"] = (c_int, t["grbda_aba_f64"][1][:-1])


def _int_for_size_t(t):
    args, i = list(t["grbda_rnea_f32"][1]), _position("grbda_rnea_f32", "B")
    assert args[i] is c_size_t
    args[i] = c_int
    t["grbda_rnea_f32"] = (c_int, tuple(args))


def _size_t_for_int(t):
    args, i = list(t["grbda_rnea_f32"][1]), _position("grbda_rnea_f32", "device")
    args[i] = c_size_t
    t["grbda_rnea_f32"] = (c_int, tuple(args))


def _pointer_for_step(t):
    args, i = list(t["grbda_fd_dq_f64"][1]), _position("grbda_fd_dq_f64", "step")
    assert args[i] is c_double
    args[i] = c_void_p
    t["grbda_fd_dq_f64"] = (c_int, tuple(args))


def _step_for_pointer(t):
    args, i = list(t["grbda_rnea_derivatives_f32"][1]), _position("grbda_rnea_derivatives_f32", "dtau_dq")
    args[i] = c_double
    t["grbda_rnea_derivatives_f32"] = (c_int, tuple(args))


def _host_with_stream(t):
    t["grbda_step_host_f64"] = (c_int, t["grbda_step_host_f64"][1] + (c_void_p,))


def _int_for_text(t):
    t["grbda_strerror"] = (c_int, t["grbda_strerror"][1])


def _missing(t):
    del t["grbda_spd_bad_pivots"]


@pytest.mark.parametrize("defect", [_dropped, _int_for_size_t, _size_t_for_int, _pointer_for_step, _step_for_pointer, _host_with_stream,
                                    _int_for_text, _missing], ids=lambda f: f.__name__.lstrip("_"))
def test_the_comparison_fails_on_a_seeded_defect(defect):
    table = dict(SIGNATURES)
    defect(table)
    with pytest.raises(AssertionError):
        compare(table, PROTOS)
