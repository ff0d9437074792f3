"""CPU: the boundary of the stereo-search extension (include/cubeslam_hip/stereo_search.h): every function it declares is exported and typed from the header, its version is
answered, a wrong dtype is refused before the call, and NULL arguments return CS_ERR_BAD_ARG before any HIP call (this test runs without a device).  The two refusals that need a
matcher with a frame -- n != N and mono = 0 without u_right -- are in tests/test_stereo_search_gpu.py::test_errors_leave_the_matcher_usable: a matcher cannot be created without a
device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT = os.path.join(ROOT, "include", "cubeslam_hip", "stereo_search.h")
BAD_ARG = -2
NAMES = ["cs_match_by_projection_frame_stereo", "cs_match_by_projection_stream_stereo", "cs_match_local_map_frustum_stereo", "cs_match_local_map_stereo", "cs_matcher_set_u_right",
         "cs_stereo_search_version"]
MONO = {"cs_match_by_projection_frame_stereo": "cs_match_by_projection_frame", "cs_match_by_projection_stream_stereo": "cs_match_by_projection_stream",
        "cs_match_local_map_stereo": "cs_match_local_map", "cs_match_local_map_frustum_stereo": "cs_match_local_map_frustum"}


def test_extension_header_is_exported_and_typed():
    from cube_slam_amd import _lib
    text = open(EXT).read()
    assert EXT in _lib.extension_headers() and _lib.extension_version(text) == ("stereo_search", 1)
    assert re.search(r'#include "\.\./cubeslam_hip\.h"', text)
    sigs = _lib.signatures(text)
    naive = sorted(set(re.findall(r"\b(cs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert sorted(sigs) == naive == NAMES
    main = _lib.signatures(open(_lib.HEADER).read())
    assert not set(NAMES) & set(main) and "CS_STEREO_SEARCH_VERSION" not in open(_lib.HEADER).read()
    lib = _lib.lib()
    assert lib.cs_stereo_search_version() == 1
    for n, (restype, argtypes) in sigs.items():
        f = getattr(lib, n)  # exported
        assert f.restype is restype is C.c_int and f.argtypes == argtypes, n
    ip, fp, vp, f, i = C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_void_p, C.c_float, C.c_int
    # each stereo entry takes the arguments of the entry it is named after, and more behind them
    for n, base in MONO.items():
        assert sigs[n][1][:len(main[base][1])] == main[base][1], n
    extra = lambda n: sigs[n][1][len(main[MONO[n]][1]):]
    assert extra("cs_match_by_projection_frame_stereo") == [fp, f, f, i, ip]          # Tlw, bf, mb, mono, direction
    assert extra("cs_match_by_projection_stream_stereo") == [fp, fp, i, f, f, i, ip]  # Tlw, u_right, u_right_on_device, bf, mb, mono, direction
    assert extra("cs_match_local_map_stereo") == [fp]                                 # proj_xr
    assert extra("cs_match_local_map_frustum_stereo") == []
    assert sigs["cs_matcher_set_u_right"][1] == [vp, vp, fp, i, i]


def test_wrong_dtype_is_refused_before_the_call():
    from cube_slam_amd._lib import lib, ptr
    u = np.zeros(4, np.float32)
    assert lib().cs_matcher_set_u_right(None, None, ptr(u), 4, 0) == BAD_ARG
    with pytest.raises(C.ArgumentError):
        lib().cs_matcher_set_u_right(None, None, ptr(u.astype(np.float64)), 4, 0)
    with pytest.raises(C.ArgumentError):
        lib().cs_matcher_set_u_right(None, None, ptr(u), 4.0, 0)  # a Python float for an int
    a = _frame_args()
    with pytest.raises(C.ArgumentError):
        _frame_call(dict(a, Tlw=a["Tlw"].astype(np.float64)))
    with pytest.raises(C.ArgumentError):
        _frame_call(dict(a, direction=np.zeros(1, np.float32)))
    with pytest.raises(C.ArgumentError):
        _frame_call(dict(a, mono=0.5))


def _frame_args():
    n = 3
    return dict(ctx=None, m=None, n=n, wp=np.zeros((n, 3), np.float32), valid=np.ones(n, np.uint8), blocks=np.ones(n, np.uint8), desc=np.zeros((n, 32), np.uint8),
                octave=np.zeros(n, np.int32), angle=np.zeros(n, np.float32), Tcw=np.eye(4, dtype=np.float32)[:3].copy(), sf=np.ones(8, np.float32), tm=np.zeros(8, np.int32),
                nm=np.zeros(1, np.int32), Tlw=np.eye(4, dtype=np.float32)[:3].copy(), mono=0, direction=np.zeros(1, np.int32))


def _frame_call(a):
    from cube_slam_amd._lib import lib, ptr
    return lib().cs_match_by_projection_frame_stereo(a["ctx"], a["m"], a["n"], ptr(a["wp"]), ptr(a["valid"]), ptr(a["blocks"]), ptr(a["desc"]), ptr(a["octave"]), ptr(a["angle"]), ptr(a["Tcw"]),
                                                     1.0, 1.0, 0.0, 0.0, ptr(a["sf"]), len(a["sf"]), 10.0, 0, None, ptr(a["tm"]), ptr(a["nm"]), ptr(a["Tlw"]), 8.0, 0.5, a["mono"],
                                                     ptr(a["direction"]))


def test_null_arguments_are_refused_without_a_device():
    """A NULL context or matcher: CS_ERR_BAD_ARG from every entry, with mono = 0 and with mono = 1, before any HIP call; the outputs are left alone."""
    from cube_slam_amd._lib import lib, ptr
    a = _frame_args()
    a["direction"][0] = 77
    for mono in (0, 1):
        assert _frame_call(dict(a, mono=mono)) == BAD_ARG
        assert _frame_call(dict(a, mono=mono, Tcw=None)) == BAD_ARG
    assert a["direction"][0] == 77
    f4 = np.zeros(4, np.float32); u8 = np.zeros(4, np.uint8); i4 = np.zeros(4, np.int32)
    for mono in (0, 1):
        assert lib().cs_match_by_projection_stream_stereo(None, None, None, 0, 1, ptr(f4), None, 0.0, 1.0, 0.0, 1.0, 4, 4, ptr(np.zeros(12, np.float32)), ptr(u8), ptr(u8), None,
                                                          ptr(np.zeros(12, np.float32)), 1.0, 1.0, 0.0, 0.0, ptr(f4), 4, 5.0, 0, ptr(i4), ptr(i4), ptr(np.zeros(12, np.float32)), ptr(f4), 0,
                                                          8.0, 0.5, mono, None) == BAD_ARG
    assert lib().cs_match_local_map_stereo(None, None, 4, ptr(np.zeros(8, np.float32)), ptr(f4), ptr(i4), ptr(u8), ptr(u8), ptr(np.zeros(128, np.uint8)), ptr(f4), 4, 1.0, 0.8, None, ptr(i4),
                                           ptr(i4), ptr(f4)) == BAD_ARG
    r3 = np.zeros(9, np.float32); t3 = np.zeros(3, np.float32); w = np.zeros(12, np.float32)
    assert lib().cs_match_local_map_frustum_stereo(None, None, ptr(r3), ptr(t3), ptr(t3), 4, ptr(w), ptr(w), ptr(f4), ptr(f4), ptr(u8), ptr(u8), ptr(np.zeros(128, np.uint8)), None, 1.0, 1.0,
                                                   0.0, 0.0, 8.0, 0.18, ptr(f4), 4, 0.5, 1.0, 0.8, ptr(i4), ptr(i4), ptr(i4), None, ptr(u8), None, None, None) == BAD_ARG
    assert lib().cs_matcher_set_u_right(None, None, None, 0, 0) == BAD_ARG
