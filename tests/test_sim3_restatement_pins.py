"""The judge of the Sim3 / relocalisation GPU tests (tests/sim3_restatement.py) against the reference's own text: ORBmatcher::SearchByProjection(pKF, Scw, ...)
(orb_object_slam/src/ORBmatcher.cc:309-427), Fuse(pKF, Scw, ...) (:1010-1139), SearchBySim3 (:1141-1371), SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist)
(:1727-1858), MapPoint::PredictScale with the two distance getters, KeyFrame::GetFeaturesInArea / IsInImage and Frame::GetFeaturesInArea are cut out of the reference at test
time into tmp_path, compiled there around tests/cpp/ref_sim3_standins.cpp (our stand-ins for MapPoint / KeyFrame / Frame and the cv::MatExpr forms; oracle/ref_shim/cvshim.hpp for
cv::Mat) and run on the inputs of tests/test_match_sim3_gpu.py, built from the same seeds.  Match vectors and counts must be equal.  Nothing cut or compiled is written inside
the repository.  The Scw / s12 scales are 1, 2 and 0.5 only and the Sim3 rotations turn about the x axis, so the scalar cv::MatExpr operations of the reference's first lines are
exact under any reading and the decomposition handed to the restatement is the reference's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import sim3_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="the restatement is pinned to the reference's text under /root/reference")

WANT = [("orb_object_slam/src/ORBmatcher.cc", ["const int ORBmatcher::TH_HIGH = 100;", "const int ORBmatcher::TH_LOW = 50;", "const int ORBmatcher::HISTO_LENGTH = 30;",
                                               "int ORBmatcher::SearchByProjection(KeyFrame *pKF, cv::Mat Scw, const vector<MapPoint *> &vpPoints, vector<MapPoint *> &vpMatched, int th)",
                                               "int ORBmatcher::Fuse(KeyFrame *pKF, cv::Mat Scw, const vector<MapPoint *> &vpPoints, float th, vector<MapPoint *> &vpReplacePoint)",
                                               "int ORBmatcher::SearchBySim3(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint *> &vpMatches12,",
                                               "int ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint *> &sAlreadyFound, const float th, const int ORBdist)",
                                               "void ORBmatcher::ComputeThreeMaxima(", "int ORBmatcher::DescriptorDistance("]),
        ("orb_object_slam/src/MapPoint.cc", ["float MapPoint::GetMinDistanceInvariance()", "float MapPoint::GetMaxDistanceInvariance()",
                                             "int MapPoint::PredictScale(const float &currentDist, const float &logScaleFactor)"]),
        ("orb_object_slam/src/KeyFrame.cc", ["vector<size_t> KeyFrame::GetFeaturesInArea(const float &x, const float &y, const float &r) const", "bool KeyFrame::IsInImage(const float &x, const float &y) const"]),
        ("orb_object_slam/src/Frame.cc", ["vector<size_t> Frame::GetFeaturesInArea(const float &x, const float &y, const float &r, const int minLevel, const int maxLevel) const"])]


def _cut(text, sig):
    """The definition that starts with `sig`: a statement up to its `;`, or a function up to the brace that closes its body."""
    a = text.index(sig)
    if sig.endswith(";"):
        return text[a:a + len(sig)]
    i = text.index("{", a)
    depth = 0
    while True:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
        if depth == 0:
            return text[a:i]


class FrameIn(C.Structure):
    _fields_ = [("N", C.c_int), ("x", C.c_void_p), ("y", C.c_void_p), ("angle", C.c_void_p), ("octave", C.c_void_p), ("desc", C.c_void_p), ("dynamic", C.c_void_p),
                ("minX", C.c_float), ("maxX", C.c_float), ("minY", C.c_float), ("maxY", C.c_float)]


class PointsIn(C.Structure):
    _fields_ = [("n", C.c_int), ("world_pos", C.c_void_p), ("normal", C.c_void_p), ("min_distance", C.c_void_p), ("max_distance", C.c_void_p), ("skip", C.c_void_p), ("desc", C.c_void_p)]


class CamIn(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("log_sf", C.c_float), ("scale_factors", C.c_void_p), ("n_levels", C.c_int)]


def _keep(keep, a, dtype):
    a = np.ascontiguousarray(a, dtype)
    keep.append(a)
    return a.ctypes.data


def _frame(keep, keys, desc, dynamic=None):
    return FrameIn(len(keys), _keep(keep, keys["x"], np.float32), _keep(keep, keys["y"], np.float32), _keep(keep, keys["angle"], np.float32), _keep(keep, keys["octave"], np.int32),
                   _keep(keep, desc, np.uint8), None if dynamic is None else _keep(keep, dynamic, np.uint8), *[float(b) for b in R.BOUNDS])


def _points(keep, pts, normal=True):
    return PointsIn(len(pts["skip"]), _keep(keep, pts["world_pos"], np.float32), _keep(keep, pts["normal"], np.float32) if normal else None, _keep(keep, pts["min_distance"], np.float32),
                    _keep(keep, pts["max_distance"], np.float32), _keep(keep, pts["skip"], np.uint8), _keep(keep, pts["mp_desc"], np.uint8))


def _fp(a):
    a = np.ascontiguousarray(a, np.float32)
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


def _T44(Rm, t, s=1.0):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = np.float32(s) * np.asarray(Rm, np.float32).reshape(3, 3)
    T[:3, 3] = np.float32(s) * np.asarray(t, np.float32)
    return T


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    d = tmp_path_factory.mktemp("ref_sim3")
    parts = []
    for rel, sigs in WANT:
        text = open(os.path.join(REF, rel)).read()
        parts += [_cut(text, s) for s in sigs]
    (d / "ref_sim3_extracted.inc").write_text("\n\n".join(parts) + "\n")
    so = str(d / "libref_sim3.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-ffp-contract=off", "-fPIC", "-shared", "-I" + str(d), "-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "ref_sim3_standins.cpp")])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def frames(oracle):
    return R.frames(oracle)


@pytest.fixture(scope="module")
def ref_frames(oracle, frames):
    return [R.make_frame(oracle, k, d) for k, d in frames]


INTR = (R.FX, R.FY, R.CX, R.CY)


def _cam(keep):
    return CamIn(*INTR, R.LOG_SF, _keep(keep, R.SF, np.float32), len(R.SF))


def test_cut_takes_whole_definitions():
    text = "int f(int a)\n{\n  if (a) { return 1; }\n  return 0;\n}\nint g() { return 2; }\nconst int K = 3;\n"
    assert _cut(text, "int f(int a)") == "int f(int a)\n{\n  if (a) { return 1; }\n  return 0;\n}" and _cut(text, "int g()") == "int g() { return 2; }" and _cut(text, "const int K = 3;") == "const int K = 3;"


@pytest.mark.parametrize("th,orb_dist,ori,rotated", [(10.0, 100, True, False), (10.0, 100, False, False), (3.0, 64, True, False), (3.0, 64, False, False), (10.0, 100, True, True)])
def test_relocalisation_search(ref, oracle, frames, ref_frames, th, orb_dist, ori, rotated):
    (k1, d1), (k2, d2) = frames
    T, pts, _ = R.projection_case(frames, 100)
    pre, dyn = R.blocked_split(len(k2), 102)
    ang = R.rotated_angles(k1["angle"], 7) if rotated else k1["angle"]
    st = {}
    want, nw, _ = R.search_by_projection_reloc(oracle, ref_frames[1], *T, pts, ang, INTR, R.LOG_SF, R.SF, th, orb_dist, ori, pre | dyn, st)
    keep = []
    tm = np.zeros(len(k2), np.int32)
    a, ap = _fp(ang); Tm, Tp = _fp(_T44(T[0], T[1]))
    inside = _without_outside(oracle, R.RELOC, pts, T, th)
    n = ref.pin_search_by_projection_reloc(C.byref(_frame(keep, k2, d2, dyn)), C.byref(_cam(keep)), Tp, C.byref(_points(keep, inside, False)), ap, pre.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                           C.c_float(th), orb_dist, int(ori), tm.ctypes.data_as(C.POINTER(C.c_int)))
    assert n == nw and np.array_equal(tm, want) and nw >= 50
    if rotated:
        assert st["cut"] >= 10  # a map where the orientation cut removes matches


def _without_outside(oracle, mode, pts, T, th):
    """The reference is undefined for a point whose predicted level is outside mvScaleFactors (it reads past the vector): those points -- which the restatement and the device
    drop -- are handed to the reference as skipped ones."""
    out = dict(pts)
    skip = pts["skip"].copy()
    for i in range(len(skip)):
        if not skip[i]:
            r = R.preamble(mode, pts["world_pos"][i], pts["normal"][i], pts["min_distance"][i], pts["max_distance"][i], T, INTR, R.BOUNDS, R.LOG_SF, R.SF, th)
            skip[i] = r[0] == "outside"
    out["skip"] = skip
    return out


@pytest.mark.parametrize("s", [1.0, 2.0, 0.5])
@pytest.mark.parametrize("th", [10, 40])
def test_sim3_projection_search(ref, oracle, frames, ref_frames, s, th):
    (k1, d1), (k2, d2) = frames
    T, pts, _ = R.projection_case(frames, 200, pre_matched=0.3)
    pre, dyn = R.blocked_split(len(k2), 202, 0.3)
    st = {}
    want, nw, _ = R.search_by_projection_sim3(oracle, ref_frames[1], *T, pts, INTR, R.LOG_SF, R.SF, float(th), pre | dyn, st)
    keep = []
    tm = np.zeros(len(k2), np.int32)
    Sm, Sp = _fp(_T44(T[0], T[1], s))
    n = ref.pin_search_by_projection_sim3(C.byref(_frame(keep, k2, d2, dyn)), C.byref(_cam(keep)), Sp, C.byref(_points(keep, _without_outside(oracle, R.SIM3, pts, T, float(th)))),
                                          pre.ctypes.data_as(C.POINTER(C.c_ubyte)), th, tm.ctypes.data_as(C.POINTER(C.c_int)))
    assert n == nw and np.array_equal(tm, want) and nw >= 100
    if th == 40:
        assert st["contested"] >= 20  # a map where map points compete for a key point


@pytest.mark.parametrize("s", [1.0, 2.0])
@pytest.mark.parametrize("th", [4.0, 8.0])
def test_sim3_fuse_search(ref, oracle, frames, ref_frames, s, th):
    (k1, d1), (k2, d2) = frames
    T, pts, tb = R.projection_case(frames, 300, pre_matched=0.0)
    bi, bd, nw, _ = R.fuse_sim3(oracle, ref_frames[1], *T, pts, INTR, R.LOG_SF, R.SF, th, tb)
    keep = []
    n_pts = len(pts["skip"])
    fmp = np.zeros(n_pts, np.int32); fidx = np.zeros(n_pts, np.int32); nrec = C.c_int()
    Sm, Sp = _fp(_T44(T[0], T[1], s))
    n = ref.pin_fuse_sim3(C.byref(_frame(keep, k2, d2, tb)), C.byref(_cam(keep)), Sp, C.byref(_points(keep, _without_outside(oracle, R.SIM3, pts, T, th))), C.c_float(th),
                          fmp.ctypes.data_as(C.POINTER(C.c_int)), fidx.ctypes.data_as(C.POINTER(C.c_int)), C.byref(nrec))
    fused = np.nonzero(bd <= R.TH_LOW)[0]
    assert n == nw == nrec.value == len(fused) and nw >= 100
    assert np.array_equal(fmp[:n], fused) and np.array_equal(fidx[:n], bi[fused])


@pytest.mark.parametrize("s12", [1.0, 2.0, 0.5])
def test_search_by_sim3(ref, oracle, frames, ref_frames, s12):
    (k1, d1), (k2, d2) = frames
    Ts, p1, p2, tb1, tb2 = R.sim3_case(frames, 400, s12)
    want, nw, _ = R.search_by_sim3(oracle, ref_frames[0], ref_frames[1], *Ts, p1, p2, INTR, R.LOG_SF, R.SF, 7.5, tb1, tb2)
    keep = []
    m12 = np.zeros(len(k1), np.int32)
    R12 = (np.asarray(Ts[4], np.float32) / np.float32(s12)).astype(np.float32)  # sR12 = s12 * R12, exactly
    ptrs = [_fp(x) for x in (Ts[0], Ts[1], Ts[2], Ts[3], R12, Ts[5])]
    q1 = _without_outside(oracle, R.PAIR, p1, (Ts[0], Ts[1], Ts[6], Ts[7]), 7.5)
    q2 = _without_outside(oracle, R.PAIR, p2, (Ts[2], Ts[3], Ts[4], Ts[5]), 7.5)
    n = ref.pin_search_by_sim3(C.byref(_frame(keep, k1, d1, tb1)), C.byref(_frame(keep, k2, d2, tb2)), C.byref(_cam(keep)), ptrs[0][1], ptrs[1][1], ptrs[2][1], ptrs[3][1], C.c_float(s12),
                               ptrs[4][1], ptrs[5][1], C.byref(_points(keep, q1, False)), C.byref(_points(keep, q2, False)), C.c_float(7.5), m12.ctypes.data_as(C.POINTER(C.c_int)))
    assert n == nw and np.array_equal(m12, want) and nw >= 50
