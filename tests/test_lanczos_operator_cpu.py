"""The choice of the Lanczos near-field operator (pse_set_lanczos_operator) at its host-side boundaries: the C-ABI declarations, the
Python layers that name the modes, and the argument checks that need no device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def _header():
    return open(os.path.join(ROOT, "include", "pse_amd.h")).read()


def test_header_declares_the_operator_enum_and_entry_points():
    h = _header()
    enum = re.search(r"enum pse_lanczos_operator\s*\{([^}]*)\}", h)
    assert enum, "enum pse_lanczos_operator missing"
    values = dict((k, int(v)) for k, v in re.findall(r"(PSE_LANCZOS_\w+)\s*=\s*(-?\d+)", enum.group(1)))
    assert values == {"PSE_LANCZOS_RECORDS16": 0, "PSE_LANCZOS_FP64": 1}
    assert re.search(r"^int pse_set_lanczos_operator\(pse_handle \*h, int op\);", h, flags=re.M)
    assert re.search(r"^int pse_get_lanczos_operator\(pse_handle \*h, int \*op\);", h, flags=re.M)


def test_lib_declares_both_symbols_with_the_header_signatures():
    from pse_amd import _lib
    res, args = _lib.SYMBOLS["pse_set_lanczos_operator"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_int]
    res, args = _lib.SYMBOLS["pse_get_lanczos_operator"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]


def test_python_names_match_the_enum():
    from pse_amd.engine import LANCZOS_OPERATORS
    assert LANCZOS_OPERATORS == {"records16": 0, "fp64": 1}


def test_engine_rejects_an_unknown_operator_before_touching_the_library(monkeypatch):
    import pse_amd
    from pse_amd import _lib

    def no_library():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_library)
    with pytest.raises(ValueError, match="lanczos_operator"):
        pse_amd.Engine(100, (20.0, 20.0, 20.0, 0.0), lanczos_operator="fp32")


def test_ui_mirror_rejects_an_unknown_operator():
    from pse_amd import integrate

    class _Sys:
        n = 10
        box = (20.0, 20.0, 20.0, 0.0)
        dt = 1e-3
        integrators = []

    class _Group:
        system = _Sys()
        members = None

    with pytest.raises(ValueError, match="lanczos_operator"):
        integrate.PSEv1(_Group(), 1.0, lanczos_operator="float64")
    assert _Sys.integrators == []


def test_host_class_refuses_an_unknown_operator():
    from pse_amd import _PSEv1
    s = _PSEv1.Stokes(10, 20.0, 20.0, 20.0, 0.0, _PSEv1.VariantConst(1.0), 1, 0.5, 1e-3, 1e-3)
    with pytest.raises(ValueError):
        s.setLanczosOperator(2)
    s.setLanczosOperator(1)   # recorded: applied by setParams (no engine yet)


def test_null_arguments_are_refused():
    from pse_amd import _lib
    lib = _lib.load()
    v = ctypes.c_int(-7)
    assert lib.pse_set_lanczos_operator(None, 0) == -1
    assert b"null" in lib.pse_last_error()
    assert lib.pse_get_lanczos_operator(None, ctypes.byref(v)) == -1
    assert v.value == -7
