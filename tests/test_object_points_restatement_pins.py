"""The judge of the object-point tests (tests/object_points_restatement.py) against the reference's own text, cut out of the reference at test time into tmp_path and compiled
there around tests/cpp/ref_object_points_standins.cpp.  Nothing cut or compiled is written inside the repository.

Cut: the triangulation block of Tracking::CreateNewKeyFrame (orb_object_slam/src/Tracking.cc:2144-2244, between `if (triangulate_dynamic_pts)` and `if (1) // randomly select N
points`), the loop of MonoObjDepthInitialization (:876-898), the grid-gated branch (:2341-2423, from the declaration of has_object_depth_pixel_inds to the line that prints the
count), the tail of LocalMapping::CreateNewMapPoints (LocalMapping.cc:574-652), random_unique2 / random_unique, Frame::UnprojectDepth, KeyFrame::UnprojectDepth,
KeyFrame::PosInGrid and five Converter functions.  g2o::SE3Quat is the reference's own header on the Eigen stand-in of oracle/ref_shim/eigen_full.

What the reference lets one observe must be equal on every pattern: is_triangulated and which error a point raised (statuses 3 and 4 both leave silently and are told apart by
the restatement alone), the candidate list after the draws and the three counts (tracking mode), the created points in creation order (the order of mlpRecentAddedMapPoints in the
local-mapping mode).  A point from UnprojectDepth must be equal bit for bit.  PosToObj of a triangulated point differs by construction (float SVD against the stated f64 Jacobi): its
distance in the unit of tests/test_local_mapping_restatement_pins.py (2^-24 sigma_1 / (sigma_3 - sigma_4) |x3D|) is measured, its maximum recorded as R.MAX_X3D_UNITS, and
10 x that is the bound (R.TOL_X3D)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import object_points_patterns as P
from tests import object_points_restatement as R
from tests.local_mapping_restatement import x3d_scale
from tests.test_sim3_restatement_pins import _cut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="the restatement is pinned to the reference's text under /root/reference")

FUNCTIONS = [("orb_object_slam/src/Tracking.cc", ["BidiIter random_unique2(BidiIter begin, BidiIter end, int num_random)"]),
             ("orb_object_slam/src/LocalMapping.cc", ["BidiIter random_unique(BidiIter begin, BidiIter end, size_t num_random)"]),
             ("orb_object_slam/src/Frame.cc", ["cv::Mat Frame::UnprojectDepth(const int &i, float depth)"]),
             ("orb_object_slam/src/KeyFrame.cc", ["cv::Mat KeyFrame::UnprojectDepth(int i, float depth)", "bool KeyFrame::PosInGrid(const cv::KeyPoint &kp, int &posX, int &posY)"]),
             ("orb_object_slam/src/Converter.cc", ["cv::Mat Converter::toCvMat(const g2o::SE3Quat &SE3)", "cv::Mat Converter::toCvMat(const Eigen::Matrix<double, 4, 4> &m)",
                                                   "cv::Mat Converter::toCvMat(const Eigen::Matrix<double, 3, 1> &m)",
                                                   "Eigen::Matrix<double, 3, 1> Converter::toVector3d(const cv::Mat &cvVector)",
                                                   "Eigen::Matrix<float, 3, 1> Converter::toVector3f(const cv::Mat &cvVector)"])]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    d = tmp_path_factory.mktemp("ref_object_points")
    parts = []
    for rel, sigs in FUNCTIONS:
        text = open(os.path.join(REF, rel)).read()
        parts += [("template <class BidiIter>\n" if s.startswith("BidiIter") else "") + _cut(text, s) for s in sigs]
    (d / "ref_object_points_functions.inc").write_text("\n\n".join(parts) + "\n")
    t = open(os.path.join(REF, "orb_object_slam/src/Tracking.cc")).read()
    a = t.index("if (triangulate_dynamic_pts)")
    (d / "ref_object_points_triangulate.inc").write_text(t[a:t.index("if (1) // randomly select N points", a)] + "\n")
    a = t.index("for (int i = 0; i < mCurrentFrame.N; i++)", t.index("AssociateCuboids(pKFini);"))
    (d / "ref_object_points_first_frame.inc").write_text(_cut(t[a:], "for (int i = 0; i < mCurrentFrame.N; i++)") + "\n")
    a = t.index("std::vector<int> has_object_depth_pixel_inds; // points with no depth yet but with matching object and plane")
    b = t.index("\n", t.index("Online depth create mappoints", a))
    (d / "ref_object_points_tracking.inc").write_text(t[a:b] + "\n}\n")  # (closes `if (whether_actually_planeobj_init_pt)`)
    lm = open(os.path.join(REF, "orb_object_slam/src/LocalMapping.cc")).read()
    (d / "ref_object_points_local_mapping.inc").write_text(_cut(lm, "if (mono_allframe_Obj_depth_init && !whether_dynamic_object)") + "\n")
    so = str(d / "libref_object_points.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-ffp-contract=off", "-fPIC", "-shared", "-I" + str(d), "-I" + os.path.join(REF, "orb_object_slam"),
                           "-I" + os.path.join(ROOT, "oracle", "ref_shim", "eigen_full"), "-o", so, os.path.join(ROOT, "tests", "cpp", "ref_object_points_standins.cpp")])
    return C.CDLL(so)


def _p(a, t):
    return None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.POINTER(t))


def _pair(c, f):
    """Pair f of a triangulation case as pin_triangulate takes it."""
    a, b = c["first"][f], c["first"][f + 1]
    cl, cn = slice(c["cub_first_last"][f], c["cub_first_last"][f + 1]), slice(c["cub_first_now"][f], c["cub_first_now"][f + 1])
    idx = c["idx_last"][a:b].copy()
    obj_last, obj_now = c["obj_last"][a:b].copy(), c["obj_now"][a:b].copy()
    gone = idx == -1
    obj_last[gone], obj_now[gone] = 0, 0  # (rows of a point without an observation are not read; the stand-in stores them in arrays of its own)
    return dict(n=int(b - a), Tl=c["Tcw_last"][f], Tn=c["Tcw_now"][f], K4=c["K4"][f], pl=c["cub_pose_last"][cl], pn=c["cub_pose_now"][cn],
                tl=None if c["tracklet_last"] is None else c["tracklet_last"][cl], tn=None if c["tracklet_now"] is None else c["tracklet_now"][cn], kp1=c["kp1"][a:b],
                kp2=c["kp2"][a:b], ol=obj_last, on=obj_now, il=idx, wp=c["world_pos"][a:b], span=(a, b))


def _run_pair(ref, q, harris, associated):
    n = q["n"]
    tri, pto, err = np.zeros(max(n, 1), np.uint8), np.zeros((max(n, 1), 3), np.float32), np.zeros(max(n, 1), np.int32)
    flags = np.full(len(q["pl"]), 1 if associated else 0, np.uint8)
    r = ref.pin_triangulate(n, _p(q["Tl"], C.c_float), _p(q["Tn"], C.c_float), _p(q["K4"], C.c_float), len(q["pl"]), _p(q["pl"], C.c_double), len(q["pn"]), _p(q["pn"], C.c_double),
                            _p(q["tl"], C.c_int), _p(q["tn"], C.c_int), _p(flags, C.c_uint8), int(harris), _p(q["kp1"], C.c_float), _p(q["kp2"], C.c_float), _p(q["ol"], C.c_int),
                            _p(q["on"], C.c_int), _p(q["il"], C.c_int), _p(q["wp"], C.c_float), _p(tri, C.c_uint8), _p(pto, C.c_float), _p(err, C.c_int))
    assert r == 0
    return tri[:n], pto[:n], err[:n]


def test_triangulation_equals_the_reference(ref):
    worst = 0.0
    for name in P.TRI_NAMES:
        c, want, infos = P.case(name), P.expected(name), P.infos(name)
        for f in range(len(c["first"]) - 1):
            q = _pair(c, f)
            a, b = q["span"]
            for harris, associated in ((1, 0), (0, 1)):  # both key-point sources, both ways the last pose is resolved: the arithmetic is the same text
                tri, pto, err = _run_pair(ref, q, harris, associated)
                st = want["status"][a:b]
                assert np.array_equal(tri, (st == R.TRIANGULATED).astype(np.uint8)), name
                assert np.array_equal(err, np.where(st == R.NO_OBSERVATION, 1, np.where(st == R.TRACKLET, 2, 0))), name
                for i in np.flatnonzero(st == R.TRIANGULATED):
                    d = float(np.abs(pto[i].astype(np.float64) - want["pos_to_obj"][a + i]).max()) / x3d_scale(infos[a + i]["A"], want["x3D"][a + i])
                    assert d <= R.TOL_X3D, (name, f, i, d)
                    worst = max(worst, d)
    print("MAX_X3D_UNITS = %r" % worst)
    assert 0.5 * R.MAX_X3D_UNITS <= worst <= R.MAX_X3D_UNITS and R.TOL_X3D == 10 * R.MAX_X3D_UNITS


@pytest.mark.parametrize("name", P.OD_NAMES)
@pytest.mark.parametrize("mode", P.MODES)
def test_object_depth_equals_the_reference(ref, name, mode):
    c, want = P.case(name), P.expected(name, mode)
    for f in range(len(c["first"]) - 1):
        a, b = c["first"][f], c["first"][f + 1]
        N = int(b - a)
        k = c["keys"][a:b]
        xy = np.stack([k["x"], k["y"]], 1).astype(np.float32) if N else np.zeros((1, 2), np.float32)
        cub = c["cuboid_depth"][c["cub_first"][f]:c["cub_first"][f + 1]]
        draws = c["draws"][c["draw_first"][f]:c["draw_first"][f + 1]]
        m = max(N, 1)
        nc, raw, mx = C.c_int(), C.c_int(), C.c_int()
        shuffled, new_idx, new_x = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros((m, 3), np.float32)
        pad = lambda v, dt: np.ascontiguousarray(v if len(v) else np.zeros(1, dt), dt)
        n_new = ref.pin_object_depth(mode, N, _p(xy, C.c_float), _p(pad(k["octave"], np.int32), C.c_int), _p(pad(c["has_map_point"][a:b], np.uint8), C.c_uint8),
                                     _p(pad(c["object_id"][a:b], np.int32), C.c_int), len(cub), _p(pad(cub, np.float32), C.c_float), _p(c["K4"][f], C.c_float),
                                     _p(c["bounds"][f], C.c_float), _p(c["Twc"][f], C.c_float), len(draws), _p(pad(draws, np.int32), C.c_int), C.byref(nc), C.byref(raw), C.byref(mx),
                                     _p(shuffled, C.c_int), _p(new_idx, C.c_int), _p(new_x, C.c_float))
        w0, w1 = want["new_first"][f], want["new_first"][f + 1]
        assert n_new == w1 - w0, (name, mode, f)
        assert np.array_equal(new_idx[:n_new], want["new_idx"][w0:w1]), (name, mode, f)
        assert new_x[:n_new].tobytes() == want["new_x3D"][w0:w1].tobytes(), (name, mode, f)
        if mode == R.TRACKING:
            c0, c1 = want["cand_first"][f], want["cand_first"][f + 1]
            assert (nc.value, raw.value, mx.value) == (want["n_candidates"][f], want["raw_depth_pts"][f], want["max_initialize_pts"][f]), (name, f)
            assert np.array_equal(shuffled[:nc.value], want["shuffled"][c0:c1]) and sorted(shuffled[:nc.value].tolist()) == want["candidates"][c0:c1].tolist(), (name, f)


def test_out_of_draws_is_the_references_too(ref):
    """With fewer draws than max_initialize_pts the reference's rand() would have been called once more: the stand-in's replay runs dry exactly where the restatement raises."""
    c = P.case("od_more_than_80")
    k = c["keys"]
    xy = np.stack([k["x"], k["y"]], 1).astype(np.float32)
    z = np.zeros(400, np.int32)
    args = lambda n: (1, 400, _p(xy, C.c_float), _p(np.ascontiguousarray(k["octave"]), C.c_int), _p(c["has_map_point"], C.c_uint8), _p(c["object_id"], C.c_int), 3,
                      _p(c["cuboid_depth"], C.c_float), _p(c["K4"][0], C.c_float), _p(c["bounds"][0], C.c_float), _p(c["Twc"][0], C.c_float), n, _p(c["draws"], C.c_int),
                      C.byref(C.c_int()), C.byref(C.c_int()), C.byref(C.c_int()), _p(z, C.c_int), _p(z.copy(), C.c_int), _p(np.zeros((400, 3), np.float32), C.c_float))
    assert ref.pin_object_depth(*args(79)) == -1 and ref.pin_object_depth(*args(80)) == 80
