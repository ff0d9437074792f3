"""CPU: the boundary of the Sim3 refinement's probes (include/cubeslam_hip/sim3_opt_trace.h): every function the header declares is exported and typed from it, its version
is answered, the main header is what it was and says what cs_sim3_optimization demands of corr_off, a wrong dtype is refused before the call, and bad arguments return
CS_ERR_BAD_ARG before any HIP call with the outputs left alone (these tests run without a device; tests/test_sim3_opt_edges_gpu.py repeats the refusals with a context)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT = os.path.join(ROOT, "include", "cubeslam_hip", "sim3_opt_trace.h")
BAD_ARG = -2
NAMES = ["cs_sim3_exp", "cs_sim3_opt_trace_version", "cs_sim3_optimization_trace"]


def test_main_header_keeps_its_abi_and_states_the_offset_rule():
    from cube_slam_amd import _lib
    text = open(_lib.HEADER).read()
    assert len(_lib.signatures(text)) == 184 and _lib.header_version() == 108 and _lib.lib().cs_version() == 108
    assert not set(NAMES) & set(_lib.signatures(text)) and "CS_SIM3_OPT_TRACE_VERSION" not in text
    flat = re.sub(r"\s*\*?\s+", " ", text)
    comment = flat[flat.index("Optimizer::OptimizeSim3(KeyFrame*"):flat.index("int cs_sim3_optimization(")]
    assert "corr_off[0] must be 0" in comment and "CS_ERR_BAD_ARG" in comment


def test_extension_header_is_exported_and_typed():
    from cube_slam_amd import _lib
    text = open(EXT).read()
    assert EXT in _lib.extension_headers() and _lib.extension_version(text) == ("sim3_opt_trace", 1)
    assert re.search(r'#include "\.\./cubeslam_hip\.h"', text)
    sigs = _lib.signatures(text)
    naive = sorted(set(re.findall(r"\b(cs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert sorted(sigs) == naive == NAMES
    lib = _lib.lib()
    assert lib.cs_sim3_opt_trace_version() == 1
    for n, (restype, argtypes) in sigs.items():
        f = getattr(lib, n)  # exported
        assert f.restype is restype is C.c_int and f.argtypes == argtypes, n
    dp, ip, up, fp, vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.c_void_p
    product = _lib.signatures(open(_lib.HEADER).read())["cs_sim3_optimization"][1]
    assert product == [vp, C.c_int, ip, dp, dp, dp, dp, dp, dp, dp, dp, fp, up, dp, up, ip]
    assert lib.cs_sim3_optimization_trace.argtypes == product + [C.c_int, dp, ip, dp]  # the product's arguments, then max_trials, trace, n_trials, system0
    assert lib.cs_sim3_exp.argtypes == [vp, C.c_int, dp, dp] and lib.cs_sim3_opt_trace_version.argtypes == []
    from tests import sim3_opt_restatement as R
    assert int(re.search(r"#define\s+CS_SIM3_TRACE_RECORD\s+(\d+)", text).group(1)) == R.TRACE_RECORD and int(re.search(r"#define\s+CS_SIM3_TRACE_SYSTEM\s+(\d+)", text).group(1)) == 36


def test_wrong_dtype_is_refused_before_the_call():
    from cube_slam_amd._lib import lib, ptr
    u, o = np.zeros((2, 7)), np.zeros((2, 8))
    assert lib().cs_sim3_exp(None, 2, ptr(u), ptr(o)) == BAD_ARG
    with pytest.raises(C.ArgumentError):
        lib().cs_sim3_exp(None, 2, ptr(u.astype(np.float32)), ptr(o))
    with pytest.raises(C.ArgumentError):
        lib().cs_sim3_exp(None, 2.0, ptr(u), ptr(o))
    with pytest.raises(C.ArgumentError):
        lib().cs_sim3_optimization_trace(None, 0, None, None, None, None, None, None, None, None, None, None, None, None, None, None, 4, ptr(np.zeros(28, np.float32)), None, None)


def test_bad_arguments_are_refused_without_a_device():
    from cube_slam_amd._lib import lib, ptr
    u, o = np.zeros((2, 7)), np.full((2, 8), 7.0)
    assert lib().cs_sim3_exp(None, 2, ptr(u), ptr(o)) == BAD_ARG and lib().cs_sim3_exp(None, -1, ptr(u), ptr(o)) == BAD_ARG and lib().cs_sim3_exp(None, 0, None, None) == BAD_ARG
    tr, nt, s0 = np.full((1, 4, 7), 7.0), np.full(1, -7, np.int32), np.full((1, 36), 7.0)
    none16 = [None] * 14
    assert lib().cs_sim3_optimization_trace(None, 0, *none16, 4, ptr(tr), ptr(nt), ptr(s0)) == BAD_ARG  # no context
    assert lib().cs_sim3_optimization(None, 0, *none16) == BAD_ARG
    assert (o == 7.0).all() and (tr == 7.0).all() and (nt == -7).all() and (s0 == 7.0).all()
