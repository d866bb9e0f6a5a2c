"""CPU-only checks of ioc_left_adopt's place in the C ABI: declared in include/isonclust2_hip.h, exported by the library, bound
in _lib.py, and an argument error without a context (no device is touched)."""
import ctypes as C
import os
import re

from isonclust2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IOC_ERR_ARG = -1


def test_left_adopt_is_declared_and_exported():
    txt = open(os.path.join(ROOT, "include", "isonclust2_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+ioc_left_adopt\s*\(\s*ioc_ctx\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*\)\s*;", code)
    L = _lib.load()
    assert hasattr(L, "ioc_left_adopt") and "ioc_left_adopt" in _lib.SYMBOLS
    assert L.ioc_left_adopt.argtypes == [C.c_void_p, C.POINTER(C.c_int32)]


def test_left_adopt_without_a_context_is_an_argument_error():
    L = _lib.load()
    n = C.c_int32(-7)
    assert L.ioc_left_adopt(None, C.byref(n)) == IOC_ERR_ARG
    assert L.ioc_left_adopt(None, None) == IOC_ERR_ARG
    assert n.value == -7
