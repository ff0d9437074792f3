"""The judge of the stereo-search GPU tests (tests/stereo_search_restatement.py) against the reference's own text: ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th,
bMono) (orb_object_slam/src/ORBmatcher.cc:1373-1522) and ORBmatcher::SearchByProjection(F, vpMapPoints, th) (:50-142) with RadiusByViewingCos, DescriptorDistance,
ComputeThreeMaxima, Frame::GetFeaturesInArea and the three thresholds are cut out of the reference at test time into tmp_path, compiled there around
tests/cpp/ref_stereo_search_standins.cpp (our stand-ins for MapPoint / Frame / ORBmatcher; oracle/ref_shim/cvshim.hpp for cv::Mat) and run on every case of
tests/stereo_search_patterns.py and on the window of tests/test_stereo_search_gpu.py, built from the same seeds.  Match vectors, counts and the direction (tlc.z as a bit pattern
and the flag it gives) must be equal.  Nothing cut or compiled is written inside the repository."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import match_patterns as mp
from tests import stereo_search_patterns as SP
from tests import stereo_search_restatement as R
from tests.test_sim3_restatement_pins import _cut, _keep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="the restatement is pinned to the reference's text under /root/reference")

WANT = [("orb_object_slam/src/ORBmatcher.cc", ["const int ORBmatcher::TH_HIGH = 100;", "const int ORBmatcher::TH_LOW = 50;", "const int ORBmatcher::HISTO_LENGTH = 30;",
                                               "int ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint *> &vpMapPoints, const float th)",
                                               "float ORBmatcher::RadiusByViewingCos(const float &viewCos)",
                                               "int ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th, const bool bMono)",
                                               "void ORBmatcher::ComputeThreeMaxima(vector<int> *histo, const int L, int &ind1, int &ind2, int &ind3)", "int ORBmatcher::DescriptorDistance("]),
        ("orb_object_slam/src/Frame.cc", ["vector<size_t> Frame::GetFeaturesInArea(const float &x, const float &y, const float &r, const int minLevel, const int maxLevel) const"])]


class FrameIn(C.Structure):
    _fields_ = [("N", C.c_int), ("x", C.c_void_p), ("y", C.c_void_p), ("angle", C.c_void_p), ("octave", C.c_void_p), ("desc", C.c_void_p), ("dynamic", C.c_void_p),
                ("minX", C.c_float), ("maxX", C.c_float), ("minY", C.c_float), ("maxY", C.c_float)]


class CamIn(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float), ("mb", C.c_float), ("scale_factors", C.c_void_p), ("n_levels", C.c_int)]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    d = tmp_path_factory.mktemp("ref_stereo_search")
    parts = []
    for rel, sigs in WANT:
        text = open(os.path.join(REF, rel)).read()
        parts += [_cut(text, s) for s in sigs]
    (d / "ref_stereo_search_extracted.inc").write_text("\n\n".join(parts) + "\n")
    so = str(d / "libref_stereo_search.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-ffp-contract=off", "-fPIC", "-shared", "-I" + str(d), "-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "ref_stereo_search_standins.cpp")])
    lib = C.CDLL(so)
    lib.pin_search_by_projection_frame.argtypes = [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 8 + [C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.pin_search_local_map.argtypes = [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 6 + [C.c_float, C.c_float, C.c_void_p]
    return lib


def _frame(keep, keys, desc, bounds):
    return FrameIn(len(keys), _keep(keep, keys["x"], np.float32), _keep(keep, keys["y"], np.float32), _keep(keep, keys["angle"], np.float32), _keep(keep, keys["octave"], np.int32),
                   _keep(keep, desc if len(keys) else np.zeros((1, 32), np.uint8), np.uint8), None, *[float(b) for b in bounds])


def _p(keep, a, dtype):
    return _keep(keep, a if len(a) else np.zeros(1, dtype), dtype)


def run_proj(ref, keys, desc, bounds, u_right, world_pos, valid, blocks, mp_desc, last_octave, last_angle, Tcw, Tlw, intr, bf, mb, mono, sf, th, check_ori, tblocked):
    """-> (train_match, nmatches, direction, tlc.z) of the reference's text."""
    keep = []
    F = _frame(keep, keys, desc, bounds)
    cam = CamIn(*[float(a) for a in intr], float(bf), float(mb), _keep(keep, sf, np.float32), len(sf))
    tm = np.zeros(max(len(keys), 1), np.int32); z = C.c_float()
    n = ref.pin_search_by_projection_frame(C.addressof(F), C.addressof(cam), _p(keep, u_right, np.float32), None if tblocked is None else _keep(keep, tblocked, np.uint8), len(valid),
                                           _p(keep, np.asarray(world_pos).reshape(-1), np.float32), _p(keep, valid, np.uint8), _p(keep, blocks, np.uint8),
                                           _p(keep, np.asarray(mp_desc).reshape(-1), np.uint8), _p(keep, last_octave, np.int32), _p(keep, last_angle, np.float32),
                                           _keep(keep, np.asarray(Tcw, np.float32).reshape(-1)[:12], np.float32), _keep(keep, np.asarray(Tlw, np.float32).reshape(-1)[:12], np.float32),
                                           float(th), int(mono), int(check_ori), tm.ctypes.data, C.addressof(z))
    z = np.float32(z.value)
    d = R.NEITHER if mono else R.FORWARD if z > np.float32(mb) else R.BACKWARD if -z > np.float32(mb) else R.NEITHER  # :1393-1394 on the reference's own tlc.z
    return tm[:len(keys)], n, d, z


def run_local(ref, c):
    keep = []
    F = _frame(keep, c.keys, c.desc, mp.BOUNDS)
    cam = CamIn(*SP.INTR, c.bf, c.mb, _keep(keep, c.sf, np.float32), len(c.sf))
    nq = len(c.qxy)
    proj = np.concatenate([c.qxy, c.proj_xr[:, None]], axis=1).astype(np.float32)
    tm = np.zeros(max(len(c.keys), 1), np.int32)
    n = ref.pin_search_local_map(C.addressof(F), C.addressof(cam), _p(keep, c.u_right, np.float32), None if c.tblocked is None else _keep(keep, c.tblocked, np.uint8), nq,
                                 _keep(keep, proj.reshape(-1), np.float32), _keep(keep, np.zeros(nq), np.float32), _keep(keep, c.qlevel, np.int32), _keep(keep, c.valid, np.uint8),
                                 _keep(keep, c.blocks, np.uint8), _keep(keep, c.qdesc.reshape(-1), np.uint8), float(np.float32(c.th / 4.0)), float(np.float32(c.nnratio)), tm.ctypes.data)
    return tm[:len(c.keys)], n


def _check(ref, c):
    want = c.restate()
    if c.kind == "proj":
        tm, n, d, z = run_proj(ref, c.keys, c.desc, mp.BOUNDS, c.u_right, c.world_pos, c.valid, c.blocks, c.qdesc, c.qlevel, c.qangle, c.Tcw, c.Tlw, SP.INTR, c.bf, c.mb, c.mono, c.sf, c.th,
                               c.check_ori, c.tblocked)
        assert z.tobytes() == R.tlc_z(c.Tcw, c.Tlw).tobytes() and d == want[2], c.name
    else:
        tm, n = run_local(ref, c)
    assert np.array_equal(tm, want[0]) and n == want[1], (c.name, tm, want[0])


ALL = SP.designed_cases()


@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_designed_case(ref, case):
    _check(ref, case)


@pytest.mark.parametrize("kind", ["proj", "local"])
def test_equivalence_cases(ref, kind):
    for c in SP.equivalence_cases(kind):
        _check(ref, c)


def test_directions_of_seeded_poses(ref):
    """tlc.z of 200 seeded pose pairs, bit for bit, and the flags around it."""
    c = SP.direction_cases()[0]
    for seed in range(200):
        rng = np.random.default_rng(5000 + seed)
        Tcw, Tlw = SP.pose(Rm=SP._rotation(seed), t=rng.uniform(-3, 3, 3)), SP.pose(Rm=SP._rotation(1000 + seed), t=rng.uniform(-3, 3, 3))
        z = R.tlc_z(Tcw, Tlw)
        for mb in (abs(z), mp.below(abs(z)), mp.above(abs(z))):
            got = run_proj(ref, c.keys, c.desc, mp.BOUNDS, c.u_right, c.world_pos, [0], c.blocks, c.qdesc, c.qlevel, c.qangle, Tcw, Tlw, SP.INTR, c.bf, mb, 0, c.sf, c.th, False, None)
            assert got[3].tobytes() == z.tobytes() and got[2] == R.direction(Tcw, Tlw, mb, 0), seed


def test_window_inputs(ref, oracle):
    """The three pairs of the window test, from the oracle's extractor (the GPU test asserts nothing about the frames: the device's extractor is held to the oracle's elsewhere)."""
    e = oracle.ORBextractor(*mp.STREAM_ORB)
    frames = [e(img) for img in mp.stream_images()]
    c = mp.stream_case(frames, True)
    ur = SP.stream_u_right(frames)
    differs = 0
    for p in range(3):
        k, d = frames[p + 1]
        F = oracle.make_frame(k, d, mp.STREAM_BOUNDS)
        area_fn = lambda x, y, r, lo, hi: [int(i) for i in oracle.get_features_in_area(F, x, y, r, lo, hi)]
        args = (k, d, mp.STREAM_BOUNDS, ur[p], c["world_pos"][p], c["valid"][p], c["blocks"][p], c["mp_desc"][p], frames[p][0]["octave"], frames[p][0]["angle"], c["Tcw"][p], SP.STREAM_TLW[p],
                SP.INTR, SP.BF, SP.MB, 0, c["sf"], c["th"], False)
        want = R.search_by_projection_frame(*args, area_fn=area_fn)
        differs += not np.array_equal(want[0], R.search_by_projection_frame(*args, area_fn=area_fn, stereo_test=False)[0])
        tm, n, dr, _ = run_proj(ref, *args, None)
        assert np.array_equal(tm, want[0]) and n == want[1] and dr == want[2] == SP.STREAM_DIRECTIONS[p]
    assert differs >= 1  # the window's right coordinates change at least one pair's matches
