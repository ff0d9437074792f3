"""CPU: the boundary of the covisibility extension (include/cubeslam_hip/covisibility.h): every function it declares is exported and typed from the header, a wrong dtype is
refused before the call, bad arguments return CS_ERR_BAD_ARG (a NULL context before any HIP call), and the main header is what it was."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import covisibility_patterns as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT = os.path.join(ROOT, "include", "cubeslam_hip", "covisibility.h")
BAD_ARG = -2
NAMES = ["cs_covisibility_update", "cs_covisibility_update_host", "cs_covisibility_version", "cs_keyframe_culling", "cs_keyframe_culling_host", "cs_mappoint_culling",
         "cs_mappoint_culling_host"]


def test_main_header_is_unchanged():
    from cube_slam_amd import _lib
    text = open(_lib.HEADER).read()
    assert len(_lib.signatures(text)) == 184 and _lib.header_version() == 108 and _lib.header_version(text) == 108
    assert not set(NAMES) & set(_lib.signatures(text)) and "CS_COVISIBILITY_VERSION" not in text
    assert _lib.lib().cs_version() == 108


def test_extension_header_is_exported_and_typed():
    from cube_slam_amd import _lib
    text = open(EXT).read()
    assert EXT in _lib.extension_headers() and _lib.extension_version(text) == ("covisibility", 1)
    assert re.search(r'#include "\.\./cubeslam_hip\.h"', text)
    sigs = _lib.signatures(text)
    naive = sorted(set(re.findall(r"\b(cs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert sorted(sigs) == naive == NAMES
    lib = _lib.lib()
    assert lib.cs_covisibility_version() == 1
    for n, (restype, argtypes) in sigs.items():
        f = getattr(lib, n)  # exported
        assert f.restype is restype is C.c_int and f.argtypes == argtypes, n
    ip, bp, fp, vp = C.POINTER(C.c_int), C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.c_void_p
    assert lib.cs_covisibility_update.argtypes == [vp, vp, C.c_int, ip, ip, ip, C.c_int, C.c_int, C.c_int, ip, ip, ip, ip, ip, ip, ip, ip]
    assert lib.cs_covisibility_update_host.argtypes == lib.cs_covisibility_update.argtypes[1:]
    assert lib.cs_keyframe_culling_host.argtypes == [vp, C.c_int, ip, ip, ip, ip, fp, fp, C.c_int, bp, C.c_int, bp, ip, ip, ip, bp, bp, ip]
    assert lib.cs_mappoint_culling.argtypes == [vp, vp, C.c_int, ip, ip, ip, ip, C.c_int, C.c_int, bp]


def test_struct_layout_matches_the_header():
    from cube_slam_amd.covisibility import CsObsTable
    body = re.search(r"typedef struct cs_obs_table \{(.*?)\} cs_obs_table;", re.sub(r"/\*.*?\*/", "", open(EXT).read(), flags=re.S), flags=re.S).group(1)
    fields = [n for decl in body.split(";") if decl.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert fields == [n for n, _ in CsObsTable._fields_]
    assert C.sizeof(CsObsTable) == 8 + 6 * 8 and CsObsTable.obs_off.offset == 8 and CsObsTable.mp_flags.offset == 48


def test_wrong_dtype_is_refused_before_the_call():
    from cube_slam_amd._lib import lib, ptr
    from cube_slam_amd.covisibility import ObsTable
    c = P.case("vote_threshold")
    t = P.obs_table(c["t"])
    s = t.c_struct()
    nq = len(c["query_kf"])
    out = [np.zeros(64, np.int32) for _ in range(8)]
    host = lambda q, off: lib().cs_covisibility_update_host(C.byref(s), nq, ptr(q), ptr(off), ptr(c["kf_mp"]), 1, 15, 64, *[ptr(o) for o in out])
    device = lambda q, off: lib().cs_covisibility_update(None, C.byref(s), nq, ptr(q), ptr(off), ptr(c["kf_mp"]), 1, 15, 64, *[ptr(o) for o in out])
    assert host(c["query_kf"], c["kf_off"]) == 0 and device(c["query_kf"], c["kf_off"]) == BAD_ARG
    for call in (host, device):
        with pytest.raises(C.ArgumentError):
            call(c["query_kf"].astype(np.int64), c["kf_off"])
        with pytest.raises(C.ArgumentError):
            call(c["query_kf"], c["kf_off"].astype(np.float32))
    with pytest.raises(C.ArgumentError):
        lib().cs_mappoint_culling_host(C.byref(s), 0, None, None, None, None, 1.5, 3, None)  # a Python float for an int
    # the table's fields are typed too: the struct does not take a pointer of another type
    t.obs_kf = t.obs_kf.astype(np.int64)
    with pytest.raises(TypeError):
        t.c_struct()
    assert ObsTable(1, [0], [], [], [], [], []).n_points == 0


def _vote_args(c, **over):
    a = dict(t=c["t"], n=len(c["query_kf"]), q=c["query_kf"], off=c["kf_off"], mp=c["kf_mp"], cap=64, outs=[np.zeros(64, np.int32) for _ in range(8)])
    a.update(over)
    return a


def _vote_host(a, ctx_null=False):
    from cube_slam_amd._lib import lib, ptr
    s = P.obs_table(a["t"]).c_struct() if a["t"] is not None else None
    args = [C.byref(s) if s is not None else None, a["n"], ptr(a["q"]), ptr(a["off"]), ptr(a["mp"]), 1, 15, a["cap"]] + [ptr(o) for o in a["outs"]]
    return lib().cs_covisibility_update(None, *args) if ctx_null else lib().cs_covisibility_update_host(*args)


def _table_with(t, **over):
    t = dict(t)
    t.update(over)
    return t


def test_bad_arguments_of_the_vote():
    c = P.case("vote_threshold")
    t = c["t"]
    assert _vote_host(_vote_args(c)) == 0
    assert _vote_host(_vote_args(c), ctx_null=True) == BAD_ARG  # NULL context: refused before any HIP call (this test runs without a device)
    edit = lambda a, i, v: (lambda b: (b.__setitem__(i, v), b)[1])(a.copy())
    bad = [
        _vote_args(c, t=None), _vote_args(c, q=None), _vote_args(c, off=None), _vote_args(c, mp=None), _vote_args(c, n=-1), _vote_args(c, cap=-1),
        _vote_args(c, outs=[None] + [np.zeros(64, np.int32) for _ in range(7)]), _vote_args(c, outs=[np.zeros(64, np.int32) for _ in range(7)] + [None]),
        _vote_args(c, q=edit(c["query_kf"], 0, t["n_kf"])), _vote_args(c, q=edit(c["query_kf"], 0, -1)),  # the query outside the key-frame table
        _vote_args(c, mp=edit(c["kf_mp"], 2, t["n_points"])), _vote_args(c, mp=edit(c["kf_mp"], 2, -2)),  # a slot outside the point table
        _vote_args(c, off=np.array([1, 16], np.int32)), _vote_args(c, off=np.array([0, 16, 3], np.int32), n=2, q=np.array([0, 1], np.int32)),  # offsets not from 0; decreasing
        _vote_args(c, t=_table_with(t, obs_off=edit(t["obs_off"], 3, int(t["obs_off"][2]) - 1))),  # point offsets decreasing
        _vote_args(c, t=_table_with(t, obs_kf=edit(t["obs_kf"], 0, t["n_kf"]))), _vote_args(c, t=_table_with(t, obs_kf=edit(t["obs_kf"], 0, -1))),
        _vote_args(c, t=_table_with(t, obs_kf=edit(t["obs_kf"], 1, int(t["obs_kf"][0])))),  # a run that is not strictly ascending
        _vote_args(c, t=_table_with(t, n_kf=-1)),
    ]
    for i, a in enumerate(bad):
        assert _vote_host(a) == BAD_ARG, i
        assert _vote_host(a, ctx_null=True) == BAD_ARG, i


def test_bad_arguments_of_the_cullings():
    from cube_slam_amd._lib import lib, ptr
    c = P.case("cull_boundary")
    s = P.obs_table(c["t"]).c_struct()
    nl, np_, no = len(c["local_kf"]), c["t"]["n_points"], len(c["t"]["obs_kf"])
    outs = lambda: [np.zeros(nl, np.uint8), np.zeros(nl, np.int32), np.zeros(nl, np.int32), np.zeros(np_, np.int32), np.zeros(np_, np.uint8), np.zeros(no, np.uint8)]

    def cull(ctx_null=False, **over):
        a = dict(n=nl, local=c["local_kf"], off=c["kf_off"], mp=c["kf_mp"], octave=c["slot_octave"], depth=c["slot_depth"], th=c["kf_th_depth"], flags=c["kf_flags"], outs=outs())
        a.update(over)
        args = [C.byref(s), a["n"], ptr(a["local"]), ptr(a["off"]), ptr(a["mp"]), ptr(a["octave"]), ptr(a["depth"]), ptr(a["th"]), 1, ptr(a["flags"]), 3] + [ptr(o) for o in a["outs"]] + [None]
        return lib().cs_keyframe_culling(None, *args) if ctx_null else lib().cs_keyframe_culling_host(*args)

    assert cull() == 0 and cull(ctx_null=True) == BAD_ARG
    local = c["local_kf"].copy(); local[1] = c["t"]["n_kf"]
    mp = c["kf_mp"].copy(); mp[0] = np_
    off = c["kf_off"].copy(); off[2] = off[1] - 1
    for over in (dict(local=None), dict(off=None), dict(mp=None), dict(octave=None), dict(depth=None), dict(th=None), dict(flags=None), dict(n=-1), dict(local=local), dict(mp=mp),
                 dict(off=off), dict(outs=[None] + outs()[1:]), dict(outs=outs()[:5] + [None])):
        assert cull(**over) == BAD_ARG and cull(ctx_null=True, **over) == BAD_ARG, sorted(over)

    m = P.case("mpcull_cases")
    ms = P.obs_table(m["t"]).c_struct()
    nr = len(m["recent"])

    def mpcull(ctx_null=False, **over):
        a = dict(n=nr, recent=m["recent"], found=m["mp_found"], visible=m["mp_visible"], first=m["mp_first_kf_id"], cases=np.zeros(nr, np.uint8))
        a.update(over)
        args = [C.byref(ms), a["n"], ptr(a["recent"]), ptr(a["found"]), ptr(a["visible"]), ptr(a["first"]), 10, 3, ptr(a["cases"])]
        return lib().cs_mappoint_culling(None, *args) if ctx_null else lib().cs_mappoint_culling_host(*args)

    assert mpcull() == 0 and mpcull(ctx_null=True) == BAD_ARG
    recent = m["recent"].copy(); recent[-1] = m["t"]["n_points"]
    for over in (dict(recent=None), dict(found=None), dict(visible=None), dict(first=None), dict(cases=None), dict(n=-1), dict(recent=recent)):
        assert mpcull(**over) == BAD_ARG and mpcull(ctx_null=True, **over) == BAD_ARG, sorted(over)
    assert lib().cs_mappoint_culling_host(None, 0, None, None, None, None, 10, 3, None) == BAD_ARG  # no table
