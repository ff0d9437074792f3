"""CPU: the boundary of the object-points extension (include/cubeslam_hip/object_points.h): every function it declares is exported and typed from the header, the version
answers 1, a wrong dtype is refused before the call, and the CS_ERR_BAD_ARG cases write nothing (ctx == NULL is the host form, so every check is reached without a device).
The main header is what it was."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import object_points_patterns as P
from tests import object_points_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT = os.path.join(ROOT, "include", "cubeslam_hip", "object_points.h")
BAD_ARG = -2
NAMES = ["cs_object_depth_points", "cs_object_points_version", "cs_triangulate_dynamic_points"]


def test_main_header_is_unchanged():
    from cube_slam_amd import _lib
    text = open(_lib.HEADER).read()
    assert len(_lib.signatures(text)) == 184 and _lib.header_version() == 108
    assert not set(NAMES) & set(_lib.signatures(text)) and "CS_OBJECT_POINTS_VERSION" not in text
    assert _lib.lib().cs_version() == 108


def test_extension_header_is_exported_and_typed():
    from cube_slam_amd import _lib
    text = open(EXT).read()
    assert EXT in _lib.extension_headers() and _lib.extension_version(text) == ("object_points", 1)
    assert re.search(r'#include "\.\./cubeslam_hip\.h"', text)
    sigs = _lib.signatures(text)
    naive = sorted(set(re.findall(r"\b(cs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert sorted(sigs) == naive == NAMES
    lib = _lib.lib()
    assert lib.cs_object_points_version() == 1
    for n, (restype, argtypes) in sigs.items():
        f = getattr(lib, n)  # exported
        assert f.restype is restype is C.c_int and f.argtypes == argtypes, n
    ip, bp, fp, dp, vp = C.POINTER(C.c_int), C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_void_p
    assert lib.cs_triangulate_dynamic_points.argtypes == [vp, C.c_int, ip, fp, fp, fp, ip, dp, ip, dp, ip, ip, fp, fp, ip, ip, ip, fp, bp, fp, fp, dp]
    assert lib.cs_object_depth_points.argtypes == [vp, C.c_int, C.c_int, ip, vp, bp, ip, ip, fp, fp, fp, fp, ip, ip, ip, ip, ip, ip, ip, ip, ip, ip, fp]


def test_constants_match_the_header_and_the_kernel_source():
    from cube_slam_amd import object_points as O
    text = open(EXT).read()
    d = {k: int(v) for k, v in re.findall(r"#define\s+(CS_(?:DYN|OBJECT_DEPTH)_\w+)\s+(\d+)", text)}
    assert [d["CS_DYN_TRIANGULATED"], d["CS_DYN_NO_OBSERVATION"], d["CS_DYN_TRACKLET"], d["CS_DYN_W_ZERO"], d["CS_DYN_TOO_FAR"]] == [O.TRIANGULATED, O.NO_OBSERVATION, O.TRACKLET, O.W_ZERO,
                                                                                                                                 O.TOO_FAR] == [0, 1, 2, 3, 4]
    assert [d["CS_OBJECT_DEPTH_FIRST_FRAME"], d["CS_OBJECT_DEPTH_TRACKING"], d["CS_OBJECT_DEPTH_LOCAL_MAPPING"]] == [O.FIRST_FRAME, O.TRACKING, O.LOCAL_MAPPING] == list(P.MODES)
    assert O.KEYPOINT_DTYPE.itemsize == 28


TRI_ORDER = ["first", "Tcw_last", "Tcw_now", "K4", "cub_first_last", "cub_pose_last", "cub_first_now", "cub_pose_now", "tracklet_last", "tracklet_now", "kp1", "kp2", "obj_last",
             "obj_now", "idx_last", "world_pos"]
OD_ORDER = ["first", "keys", "has_map_point", "object_id", "cub_first", "cuboid_depth", "K4", "bounds", "Twc", "draw_first", "draws"]


def _tri(c, n_pairs=None, outs=None, **over):
    from cube_slam_amd._lib import lib, ptr
    a = {k: c[k] for k in TRI_ORDER}
    a.update(over)
    P_ = int(c["first"][-1])
    outs = outs if outs is not None else [np.full(P_, 7, np.uint8), np.full((P_, 3), 7, np.float32), np.full((P_, 3), 7, np.float32), np.full((P_, 3), 7, np.float64)]
    r = lib().cs_triangulate_dynamic_points(None, len(c["first"]) - 1 if n_pairs is None else n_pairs, *[ptr(a[k]) for k in TRI_ORDER], *[ptr(o) for o in outs])
    return r, outs


def _od(c, mode, n_frames=None, outs=None, **over):
    from cube_slam_amd._lib import lib, ptr
    a = {k: c[k] for k in OD_ORDER}
    a.update(over)
    F, n = len(c["first"]) - 1, int(c["first"][-1])
    outs = outs if outs is not None else [np.full(F, 7, np.int32), np.full(F, 7, np.int32), np.full(F, 7, np.int32), np.full(F + 1, 7, np.int32), np.full(n, 7, np.int32),
                                          np.full(n, 7, np.int32), np.full(F + 1, 7, np.int32), np.full(n, 7, np.int32), np.full((n, 3), 7, np.float32)]
    r = lib().cs_object_depth_points(None, mode, F if n_frames is None else n_frames, *[ptr(a[k]) for k in OD_ORDER], *[ptr(o) for o in outs])
    return r, outs


def _untouched(outs):
    return all((np.asarray(o) == 7).all() for o in outs if o is not None)


def test_wrong_dtype_is_refused_before_the_call():
    t, o = P.case("tri_statuses"), P.case("od_two_in_cell")
    assert _tri(t)[0] == 0 and _od(o, R.TRACKING)[0] == 0
    for over in (dict(first=t["first"].astype(np.int64)), dict(Tcw_last=t["Tcw_last"].astype(np.float64)), dict(cub_pose_last=t["cub_pose_last"].astype(np.float32)),
                 dict(kp1=t["kp1"].astype(np.float64)), dict(idx_last=t["idx_last"].astype(np.int16))):
        with pytest.raises(C.ArgumentError):
            _tri(t, **over)
    for over in (dict(has_map_point=o["has_map_point"].astype(np.int32)), dict(object_id=o["object_id"].astype(np.int64)), dict(cuboid_depth=o["cuboid_depth"].astype(np.float64)),
                 dict(draws=o["draws"].astype(np.int64))):
        with pytest.raises(C.ArgumentError):
            _od(o, R.TRACKING, **over)
    with pytest.raises(C.ArgumentError):
        _od(o, 1.5)  # a Python float for the mode


def test_bad_arguments_of_the_triangulation_write_nothing():
    c = P.case("tri_statuses")
    edit = lambda a, i, v: (lambda b: (b.__setitem__(i, v), b)[1])(a.copy())
    bad = [dict(first=None), dict(Tcw_last=None), dict(Tcw_now=None), dict(K4=None), dict(cub_first_last=None), dict(cub_pose_last=None), dict(cub_first_now=None),
           dict(cub_pose_now=None), dict(tracklet_last=None), dict(tracklet_now=None),  # one tracklet table without the other
           dict(kp1=None), dict(kp2=None), dict(obj_last=None), dict(obj_now=None), dict(idx_last=None), dict(world_pos=None),
           dict(first=edit(c["first"], 0, 1)), dict(first=np.array([0, 7, 5], np.int32), n_pairs=2),  # offsets not from 0; decreasing
           dict(cub_first_last=edit(c["cub_first_last"], 0, 1)), dict(cub_first_now=edit(c["cub_first_now"], 1, -1)),
           dict(obj_last=edit(c["obj_last"], 3, 2)), dict(obj_last=edit(c["obj_last"], 3, -1)), dict(obj_now=edit(c["obj_now"], 5, 2)), dict(obj_now=edit(c["obj_now"], 5, -1)),
           dict(idx_last=edit(c["idx_last"], 3, -2)),
           dict(kp1=edit(c["kp1"], (4, 0), np.nan)), dict(kp1=edit(c["kp1"], (4, 1), np.inf)), dict(kp2=edit(c["kp2"], (6, 1), -np.inf)), dict(kp2=edit(c["kp2"], (0, 0), np.nan)),
           dict(n_pairs=-1)]
    for i, over in enumerate(bad):
        r, outs = _tri(c, **over)
        assert r == BAD_ARG and _untouched(outs), (i, sorted(over))
    for k in range(4):  # a NULL output
        outs = [np.full(7, 7, np.uint8), np.full((7, 3), 7, np.float32), np.full((7, 3), 7, np.float32), np.full((7, 3), 7, np.float64)]
        outs[k] = None
        r, outs = _tri(c, outs=outs)
        assert r == BAD_ARG and _untouched(outs), k
    # what is legal: object rows outside the tables on a point without an observation (the pattern has them), an empty batch with nothing at all
    from cube_slam_amd._lib import lib
    assert lib().cs_triangulate_dynamic_points(None, 0, *([None] * 20)) == 0


def test_bad_arguments_of_the_object_depth_write_nothing():
    c = P.case("od_batch")
    edit = lambda a, i, v: (lambda b: (b.__setitem__(i, v), b)[1])(a.copy())
    big_first = np.array([0, 8193], np.int32)
    bad = [dict(first=None), dict(keys=None), dict(has_map_point=None), dict(object_id=None), dict(cub_first=None), dict(cuboid_depth=None), dict(K4=None), dict(bounds=None),
           dict(Twc=None), dict(draw_first=None), dict(draws=None),
           dict(first=edit(c["first"], 0, 1)), dict(first=edit(c["first"], 2, 10)), dict(cub_first=edit(c["cub_first"], 1, -1)), dict(draw_first=edit(c["draw_first"], 0, 2)),
           dict(object_id=edit(c["object_id"], 0, 2)),  # frame 0 has two cuboids
           dict(object_id=edit(c["object_id"], 20, 0)),  # frame 1 has none
           dict(draws=edit(c["draws"], 3, -1)),
           dict(draw_first=np.array([0, 2] + [2] * 6, np.int32)),  # frame 0 needs 3 draws
           dict(bounds=edit(c["bounds"], (2, 1), np.inf)), dict(bounds=edit(c["bounds"], (0, 0), np.nan)), dict(bounds=edit(c["bounds"], (1, 2), -3e9)),
           dict(bounds=edit(c["bounds"], (3, 1), 0.0)), dict(bounds=edit(c["bounds"], (6, 3), -1.0)),  # mnMaxX <= mnMinX, mnMaxY <= mnMinY
           dict(n_frames=-1)]
    for i, over in enumerate(bad):
        r, outs = _od(c, R.TRACKING, **over)
        assert r == BAD_ARG and _untouched(outs), (i, sorted(over))
    for mode in (-1, 3):
        r, outs = _od(c, mode)
        assert r == BAD_ARG and _untouched(outs)
    # more than CS_RGBD_MAX_KEYPOINTS key points in a frame
    n = 8193
    from cube_slam_amd.object_points import KEYPOINT_DTYPE
    huge = dict(first=big_first, keys=np.zeros(n, KEYPOINT_DTYPE), has_map_point=np.zeros(n, np.uint8), object_id=np.full(n, -1, np.int32), cub_first=np.array([0, 0], np.int32),
                cuboid_depth=np.zeros(1, np.float32), K4=c["K4"][:1], bounds=c["bounds"][:1], Twc=c["Twc"][:1], draw_first=np.array([0, 0], np.int32), draws=np.zeros(1, np.int32))
    r, outs = _od(huge, R.LOCAL_MAPPING)
    assert r == BAD_ARG and _untouched(outs)
    huge["first"] = np.array([0, 8192], np.int32)
    assert _od(huge, R.LOCAL_MAPPING)[0] == 0
    for k in range(9):  # a NULL output
        _, outs = _od(c, R.TRACKING)
        outs = [np.full_like(o, 7) for o in outs]
        outs[k] = None
        r, outs = _od(c, R.TRACKING, outs=outs)
        assert r == BAD_ARG and _untouched(outs), k
    # what the first-frame mode does not read may be NULL there
    assert _od(c, R.FIRST_FRAME, has_map_point=None, bounds=None, draw_first=None, draws=None)[0] == 0
    assert _od(c, R.LOCAL_MAPPING, bounds=None)[0] == 0
