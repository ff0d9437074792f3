"""The judge of the TrackLocalMap GPU tests (tests/track_local_map_restatement.py) against the reference's own text: Frame::isInFrustum (orb_object_slam/src/Frame.cc:346-402) and
Frame::GetFeaturesInArea, Tracking::SearchLocalPoints / UpdateLocalPoints / UpdateLocalKeyFrames (Tracking.cc:2673-2728, :2740-2764, :2766-2874),
ORBmatcher::SearchByProjection(F, vpMapPoints, th), RadiusByViewingCos and Fuse(pKF, vpMapPoints, th), MapPoint::PredictScale with the two distance getters and
KeyFrame::GetFeaturesInArea / IsInImage are cut out of the reference at test time into tmp_path, compiled there around tests/cpp/ref_track_local_map_standins.cpp (our stand-ins
for MapPoint / KeyFrame / Frame / Tracking; oracle/ref_shim/cvshim.hpp for cv::Mat) and run on the inputs of tests/test_track_local_map_gpu.py, built from the same seeds.
Everything must be equal, floats as bit patterns.  Nothing cut or compiled is written inside the repository.

The stand-in key frames of a graph live in one array, so the pointer order of the reference's std::map<KeyFrame *, int> is the index order the library defines.  Where the
reference is undefined (a predicted level outside mvScaleFactors, a projection that is not finite) the point is handed to it as a bad one, which it skips as the restatement drops it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import sim3_restatement as S
from tests import track_local_map_restatement as R
from tests.test_sim3_restatement_pins import _cut, _keep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="the restatement is pinned to the reference's text under /root/reference")

WANT = [("orb_object_slam/src/ORBmatcher.cc", ["const int ORBmatcher::TH_HIGH = 100;", "const int ORBmatcher::TH_LOW = 50;", "const int ORBmatcher::HISTO_LENGTH = 30;",
                                               "int ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint *> &vpMapPoints, const float th)",
                                               "float ORBmatcher::RadiusByViewingCos(const float &viewCos)",
                                               "int ORBmatcher::Fuse(KeyFrame *pKF, const vector<MapPoint *> &vpMapPoints, const float th)", "int ORBmatcher::DescriptorDistance("]),
        ("orb_object_slam/src/MapPoint.cc", ["float MapPoint::GetMinDistanceInvariance()", "float MapPoint::GetMaxDistanceInvariance()",
                                             "int MapPoint::PredictScale(const float &currentDist, const float &logScaleFactor)"]),
        ("orb_object_slam/src/KeyFrame.cc", ["vector<size_t> KeyFrame::GetFeaturesInArea(const float &x, const float &y, const float &r) const", "bool KeyFrame::IsInImage(const float &x, const float &y) const"]),
        ("orb_object_slam/src/Frame.cc", ["bool Frame::isInFrustum(MapPoint *pMP, float viewingCosLimit)",
                                          "vector<size_t> Frame::GetFeaturesInArea(const float &x, const float &y, const float &r, const int minLevel, const int maxLevel) const"]),
        ("orb_object_slam/src/Tracking.cc", ["void Tracking::SearchLocalPoints()", "void Tracking::UpdateLocalPoints()", "void Tracking::UpdateLocalKeyFrames()"])]


class FrameIn(C.Structure):
    _fields_ = [("N", C.c_int), ("x", C.c_void_p), ("y", C.c_void_p), ("angle", C.c_void_p), ("octave", C.c_void_p), ("desc", C.c_void_p), ("dynamic", C.c_void_p),
                ("minX", C.c_float), ("maxX", C.c_float), ("minY", C.c_float), ("maxY", C.c_float)]


class PointsIn(C.Structure):
    _fields_ = [("n", C.c_int), ("world_pos", C.c_void_p), ("normal", C.c_void_p), ("min_distance", C.c_void_p), ("max_distance", C.c_void_p), ("skip", C.c_void_p), ("desc", C.c_void_p)]


class CamIn(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float), ("log_sf", C.c_float), ("scale_factors", C.c_void_p), ("n_levels", C.c_int)]


def _frame(keep, keys, desc, bounds, dynamic=None):
    return FrameIn(len(keys), _keep(keep, keys["x"], np.float32), _keep(keep, keys["y"], np.float32), _keep(keep, keys["angle"], np.float32), _keep(keep, keys["octave"], np.int32),
                   _keep(keep, desc, np.uint8), None if dynamic is None else _keep(keep, dynamic, np.uint8), *[float(b) for b in bounds])


def _points(keep, pts, skip):
    return PointsIn(len(skip), _keep(keep, pts["world_pos"], np.float32), _keep(keep, pts["normal"], np.float32), _keep(keep, pts["min_distance"], np.float32),
                    _keep(keep, pts["max_distance"], np.float32), _keep(keep, skip, np.uint8), _keep(keep, pts["mp_desc"], np.uint8))


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _fp(keep, a):
    a = np.ascontiguousarray(a, np.float32)
    keep.append(a)
    return _ptr(a, C.c_float)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    d = tmp_path_factory.mktemp("ref_tlm")
    parts = []
    for rel, sigs in WANT:
        text = open(os.path.join(REF, rel)).read()
        parts += [_cut(text, s) for s in sigs]
    (d / "ref_track_local_map_extracted.inc").write_text("\n\n".join(parts) + "\n")
    so = str(d / "libref_tlm.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-ffp-contract=off", "-fPIC", "-shared", "-I" + str(d), "-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "ref_track_local_map_standins.cpp")])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def frames(oracle):
    return S.frames(oracle)


@pytest.fixture(scope="module")
def case(oracle, frames):
    T, pts, blocks, tb = R.local_points(frames, 700)
    fr = R.frustum_all(pts, *T, R.INTR, R.BOUNDS, R.LOG_SF, len(R.SF))
    return T, pts, blocks, tb, fr, S.make_frame(oracle, *frames[0])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run_search(ref, keys, desc, bounds, T, pts, blocks, tb_pre, dyn, intr, log_sf, sf, th_sel, undefined):
    keep = []
    n = len(pts["skip"])
    skip = (pts["skip"] != 0) | undefined
    cam = CamIn(*intr, log_sf, _keep(keep, sf, np.float32), len(sf))
    N = len(keys)
    tm = np.zeros(N, np.int32); iv = np.zeros(max(n, 1), np.uint8); pj = np.zeros((max(n, 1), 3), np.float32); lv = np.zeros(max(n, 1), np.int32); vc = np.zeros(max(n, 1), np.float32)
    vis = np.zeros(max(n, 1), np.int32)
    ntm = ref.pin_search_local_points(C.byref(_frame(keep, keys, desc, bounds, dyn)), C.byref(cam), _fp(keep, T[0]), _fp(keep, T[1]), _fp(keep, T[2]), C.byref(_points(keep, pts, skip)),
                                      _ptr(np.ascontiguousarray(blocks, np.uint8), C.c_ubyte), None if tb_pre is None else _ptr(tb_pre, C.c_ubyte), th_sel, _ptr(tm, C.c_int),
                                      _ptr(iv, C.c_ubyte), _ptr(pj, C.c_float), _ptr(lv, C.c_int), _ptr(vc, C.c_float), _ptr(vis, C.c_int))
    return ntm, tm, iv[:n], pj[:n], lv[:n], vc[:n], vis[:n]


@pytest.mark.parametrize("th_sel,th", [(0, 1.0), (1, 3.0), (2, 5.0)])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 3000])
def test_search_local_points(ref, oracle, frames, case, n, th_sel, th):
    T, pts, blocks, _, fr, F = case
    k, d = frames[0]
    pre, dyn = S.blocked_split(len(k), 704, 0.1, 0.05)  # (blocked_keys(len(k), 704, 0.1, 0.05) of local_points is pre | dyn)
    p = {a: b[:n] for a, b in pts.items()}
    f = {a: b[:n] for a, b in fr.items()}
    want = R.search_local_points(oracle, F, *T, p, blocks[:n], R.INTR, R.BOUNDS, R.LOG_SF, R.SF, th, 0.8, pre | dyn, fr=f)
    undefined = np.array([r == "outside" for r in f["reason"]], bool)
    ntm, tm, iv, pj, lv, vc, vis = _run_search(ref, k, d, R.BOUNDS, T, p, blocks[:n], pre, dyn, R.INTR, R.LOG_SF, R.SF, th_sel, undefined)
    assert ntm == want["n_to_match"] and np.array_equal(iv, want["in_view"]) and np.array_equal(vis, want["in_view"].astype(np.int32))
    assert np.array_equal(tm, want["train_match"])
    on = iv != 0  # (a point out of view keeps whatever an earlier frame left on it: only the points in view carry fields)
    assert np.array_equal(lv[on], want["pred_level"][on]) and np.array_equal(_bits(pj[on]), _bits(want["proj"][on])) and np.array_equal(_bits(vc[on]), _bits(want["view_cos"][on]))
    if n == 3000:
        assert int((tm >= 0).sum()) >= 100


def test_exact_cases(ref, oracle, frames):
    k, d = frames[0]
    F = S.make_frame(oracle, k, d, R.EX_BOUNDS)
    for name, log_sf, sf, pts, flags in R.exact_cases():
        blocks = np.ones(len(pts["skip"]), np.uint8)
        fr = R.frustum_all(pts, *R.EX_POSE, R.EX_INTR, R.EX_BOUNDS, log_sf, len(sf))
        want = R.search_local_points(oracle, F, *R.EX_POSE, pts, blocks, R.EX_INTR, R.EX_BOUNDS, log_sf, sf, 1.0, 0.8, None, fr=fr)
        undefined = np.array([r == "outside" for r in fr["reason"]], bool)
        if name == "sf2":
            undefined[12] = True  # PcZ == 0 with u = v = NaN: the reference goes on to casts of NaN
        ntm, tm, iv, pj, lv, vc, vis = _run_search(ref, k, d, R.EX_BOUNDS, R.EX_POSE, pts, blocks, None, None, R.EX_INTR, log_sf, sf, 0, undefined)
        assert iv.tolist() == [w[0] for w in flags] and ntm == want["n_to_match"] and np.array_equal(tm, want["train_match"])
        on = iv != 0
        assert np.array_equal(lv[on], want["pred_level"][on]) and np.array_equal(_bits(pj[on]), _bits(want["proj"][on])) and np.array_equal(_bits(vc[on]), _bits(want["view_cos"][on]))


@pytest.mark.parametrize("total", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_update_local_points(ref, total):
    rng = np.random.default_rng(total)  # (the generator of test_track_local_points_sizes)
    n_points = max(total // 3, 5)
    mp = rng.integers(-1, n_points, total).astype(np.int32)
    n_kf = min(total, 80)
    cuts = np.sort(rng.integers(0, total + 1, max(n_kf - 1, 0)))
    off = np.concatenate([[0], cuts, [total]]).astype(np.int32)
    skip = (rng.uniform(size=n_points) < 0.1).astype(np.uint8)
    out = np.zeros(n_points, np.int32)
    n = ref.pin_update_local_points(n_kf, _ptr(off, C.c_int), _ptr(mp, C.c_int), n_points, _ptr(skip, C.c_ubyte), _ptr(out, C.c_int))
    assert np.array_equal(out[:n], R.update_local_points(off, mp, skip))


@pytest.mark.parametrize("name", R.GRAPHS)
def test_update_local_keyframes(ref, name):
    g = R.graph_case(name)
    want, wmx = R.update_local_keyframes(**g)
    a = {k: np.ascontiguousarray(v, np.uint8 if k in ("mp_skip", "kf_bad") else np.int32) for k, v in g.items()}
    n_kf = len(a["kf_bad"])
    out = np.zeros(max(n_kf, 1), np.int32); mx = C.c_int()
    i = lambda key: _ptr(a[key], C.c_int)
    n = ref.pin_update_local_keyframes(len(a["frame_mp"]), i("frame_mp"), len(a["mp_skip"]), _ptr(a["mp_skip"], C.c_ubyte), i("obs_off"), i("obs_kf"), n_kf, _ptr(a["kf_bad"], C.c_ubyte),
                                       i("cov_off"), i("cov_kf"), i("child_off"), i("child_kf"), i("parent"), _ptr(out, C.c_int), C.byref(mx))
    assert mx.value == wmx
    if want is None:
        assert n == -1
    else:
        assert np.array_equal(out[:n], want)


@pytest.mark.parametrize("th", [3.0, 8.0])
def test_fuse_map(ref, oracle, frames, case, th):
    T, pts, blocks, tb, fr, F = case
    k, d = frames[0]
    rng = np.random.default_rng(5)  # (the key-frame side of test_fuse_map of the GPU tests)
    u_right = np.where(rng.uniform(size=len(k)) < 0.5, k["x"] - rng.uniform(1, 40, len(k)), -1.0).astype(np.float32)
    isg = (1.0 / (R.SF * R.SF)).astype(np.float32)
    ks = (rng.uniform(size=len(k)) < 0.9).astype(np.uint8)
    uv, ur, lv, va, outside = R.fuse_preamble(pts, *T, R.INTR, R.BOUNDS, R.LOG_SF, len(R.SF))
    bi, bd, nw = oracle.fuse(F[2], u_right, isg, uv, ur, np.maximum(lv, 0), va, pts["mp_desc"], R.SF, th, ks)
    undefined = np.zeros(len(va), bool)
    for i in np.nonzero((va == 0) & (pts["skip"] == 0))[0]:
        undefined[i] = S.preamble(S.SIM3, pts["world_pos"][i], pts["normal"][i], pts["min_distance"][i], pts["max_distance"][i], T, R.INTR[:4], R.BOUNDS, R.LOG_SF, R.SF, th)[0] == "outside"
    keep = []
    n_pts = len(va)
    cam = CamIn(*R.INTR, R.LOG_SF, _keep(keep, R.SF, np.float32), len(R.SF))
    fmp = np.zeros(n_pts, np.int32); fidx = np.zeros(n_pts, np.int32); nrec = C.c_int()
    n = ref.pin_fuse_map(C.byref(_frame(keep, k, d, R.BOUNDS, 1 - ks)), C.byref(cam), _fp(keep, T[0]), _fp(keep, T[1]), _fp(keep, T[2]), _ptr(u_right, C.c_float), _ptr(isg, C.c_float),
                         C.byref(_points(keep, pts, (pts["skip"] != 0) | undefined)), C.c_float(th), _ptr(fmp, C.c_int), _ptr(fidx, C.c_int), C.byref(nrec))
    fused = np.nonzero(bd <= R.TH_LOW)[0]
    assert n == nw == nrec.value == len(fused) and nw >= 100
    assert np.array_equal(fmp[:n], fused) and np.array_equal(fidx[:n], bi[fused])
