"""CPU: the boundary of the pose-graph solve probe (include/cubeslam_hip/essential_graph_solve.h): every function it declares is exported and typed from the header, its
version is answered, the main header is what it was, a wrong dtype is refused before the call, and NULL arguments return CS_ERR_BAD_ARG before any HIP call (this test runs
without a device).  The refusal of a handle of another context needs a handle, which cannot be created without a device: tests/test_essential_graph_solve_gpu.py has it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT = os.path.join(ROOT, "include", "cubeslam_hip", "essential_graph_solve.h")
BAD_ARG = -2
NAMES = ["cs_essential_graph_solve", "cs_essential_graph_solve_version"]


def test_main_header_is_unchanged():
    from cube_slam_amd import _lib
    text = open(_lib.HEADER).read()
    assert len(_lib.signatures(text)) == 184 and _lib.header_version() == 108
    assert not set(NAMES) & set(_lib.signatures(text)) and "CS_ESSENTIAL_GRAPH_SOLVE_VERSION" not in text
    assert _lib.lib().cs_version() == 108


def test_extension_header_is_exported_and_typed():
    from cube_slam_amd import _lib
    text = open(EXT).read()
    assert EXT in _lib.extension_headers() and _lib.extension_version(text) == ("essential_graph_solve", 1)
    assert re.search(r'#include "\.\./cubeslam_hip\.h"', text)
    sigs = _lib.signatures(text)
    naive = sorted(set(re.findall(r"\b(cs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert sorted(sigs) == naive == NAMES
    lib = _lib.lib()
    assert lib.cs_essential_graph_solve_version() == 1
    for n, (restype, argtypes) in sigs.items():
        f = getattr(lib, n)  # exported
        assert f.restype is restype is C.c_int and f.argtypes == argtypes, n
    dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
    assert lib.cs_essential_graph_solve.argtypes == [vp, vp, dp, dp, C.c_double, dp, ip]  # ctx, eg, J, err, lambda, x_out, status
    assert lib.cs_essential_graph_solve_version.argtypes == []
    # the header says what the probe does not read
    assert re.search(r"fixed vertex's side of J is not read", re.sub(r"\s*\*?\s+", " ", text))


def test_wrong_dtype_is_refused_before_the_call():
    from cube_slam_amd._lib import lib, ptr
    J, e, x, st = np.zeros((2, 14, 7)), np.zeros((2, 7)), np.zeros((3, 7)), C.c_int(5)
    assert lib().cs_essential_graph_solve(None, None, ptr(J), ptr(e), 1.0, ptr(x), C.byref(st)) == BAD_ARG
    with pytest.raises(C.ArgumentError):
        lib().cs_essential_graph_solve(None, None, ptr(J.astype(np.float32)), ptr(e), 1.0, ptr(x), C.byref(st))
    with pytest.raises(C.ArgumentError):
        lib().cs_essential_graph_solve(None, None, ptr(J), ptr(e), 1.0, ptr(x.astype(np.float32)), C.byref(st))
    with pytest.raises(C.ArgumentError):
        lib().cs_essential_graph_solve(None, None, ptr(J), ptr(e), "1.0", ptr(x), C.byref(st))
    with pytest.raises(C.ArgumentError):
        lib().cs_essential_graph_solve(None, None, ptr(J), ptr(e), 1.0, ptr(x), ptr(np.zeros(1, np.int64)))


def test_null_arguments_are_refused_without_a_device():
    """A NULL context or handle: CS_ERR_BAD_ARG before any HIP call, for every lambda (a non-finite one is not what is refused); the outputs are left alone."""
    from cube_slam_amd._lib import lib, ptr
    J, e, x, st = np.zeros((2, 14, 7)), np.zeros((2, 7)), np.full((3, 7), 7.0), C.c_int(5)
    for lam in (1.0, 0.0, -1.0, float("nan"), float("inf")):
        assert lib().cs_essential_graph_solve(None, None, ptr(J), ptr(e), lam, ptr(x), C.byref(st)) == BAD_ARG
    assert lib().cs_essential_graph_solve(None, None, None, None, 1.0, None, None) == BAD_ARG
    assert st.value == 5 and (x == 7.0).all()
