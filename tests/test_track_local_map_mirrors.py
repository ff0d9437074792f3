"""CPU: (1) the symbols of the TrackLocalMap entries are declared and exported and the Python mirror is importable; (2) the host-only rule of the library --
cs_track_local_keyframes, the walk of cube_slam_amd/csrc/track_local_walk.h -- through the Python mirror and through the C++ mirror (cubeslam::Tracking::UpdateLocalKeyFrames,
cube_slam_amd/host/tracking.hpp) compiled by g++ with nothing of the library (tests/cpp/tracking_mirror.cpp `host`, plain and with -fsanitize=address,undefined, each run as a
child process) gives the restatement's lists on every key-frame graph; (3) the bookkeeping of the Python mirror around the device calls (the frame's own points, the skip and
blocked flags, the statistics loop and the two thresholds) with the device calls replaced by the restatement."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import sim3_restatement as S
from tests import track_local_map_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cs_match_local_map_frustum", "cs_match_fuse_map", "cs_track_local_points", "cs_track_local_keyframes")


def test_symbols_and_declarations():
    import cube_slam_amd
    from cube_slam_amd import _lib, matcher
    assert hasattr(cube_slam_amd, "Tracking") and hasattr(matcher.ORBmatcher, "SearchLocalPoints") and hasattr(matcher.ORBmatcher, "FuseMap")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cubeslam_hip.h")).read(), flags=re.S)
    for name in NAMES:
        assert hasattr(_lib.lib(), name), name
        assert re.search(r"\b%s\s*\(" % name, header), name


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("tracking_mirror")
    base = ["g++", "-std=c++17", "-Wall", "-ffp-contract=off", "-DCUBESLAM_HOST_ONLY", "-I", ROOT, os.path.join(ROOT, "tests", "cpp", "tracking_mirror.cpp")]
    subprocess.check_call(base + ["-O2", "-o", str(d / "mirror")])
    subprocess.check_call(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(d / "mirror_san")])
    return d


def test_gpp_build_of_walk_equals_restatement(exes, tmp_path):
    from cube_slam_amd.tracking import track_local_keyframes
    graphs = [R.graph_case(nm) for nm in R.GRAPHS]
    bad_slot = R.graph_case("random")  # a bad map point in the frame: its slot is cleared (:2785)
    bad_slot["mp_skip"][bad_slot["frame_mp"][5]] = 1
    graphs.append(bad_slot)
    (tmp_path / "in.bin").write_bytes(R.pack([np.asarray([len(graphs)], np.int32)] + [a for g in graphs for a in R.graph_arrays(g)]))
    want = []
    for g in graphs:
        loc, mx = R.update_local_keyframes(**g)
        ploc, pmx = track_local_keyframes(g["frame_mp"], g["mp_skip"], g["obs_off"], g["obs_kf"], g["kf_bad"], g["cov_off"], g["cov_kf"], g["child_off"], g["child_kf"], g["parent"])
        assert pmx == mx and (loc is None) == (ploc is None) and (loc is None or np.array_equal(loc, ploc))
        fm = g["frame_mp"].astype(np.int32).copy()
        has = fm >= 0
        fm[has & (g["mp_skip"][np.where(has, fm, 0)] != 0)] = -1
        want += [np.asarray([-7], np.int32) if loc is None else loc.astype(np.int32), np.asarray([mx], np.int32), fm]
    for exe in ("mirror", "mirror_san"):
        r = subprocess.run([str(exes / exe), str(tmp_path / "in.bin"), str(tmp_path / (exe + ".bin")), "host"], capture_output=True, timeout=120)
        assert r.returncode == 0 and r.stderr == b"", (exe, r.stderr.decode())
        assert (tmp_path / (exe + ".bin")).read_bytes() == R.pack(want), exe


class _FakeMatcher:
    """ORBmatcher.SearchLocalPoints answered by the restatement."""

    def __init__(self, oracle):
        self.oracle, self.mfNNratio = oracle, 0.8

    def set_frame(self, keys, desc, bounds):
        self.frame = S.make_frame(self.oracle, keys, desc, bounds)

    def SearchLocalPoints(self, Rcw, tcw, Ow, wp, nr, mn, mx, skip, blocks, desc, fx, fy, cx, cy, bf, log_sf, sf, th, limit, tb):
        pts = {"world_pos": wp, "normal": nr, "min_distance": mn, "max_distance": mx, "skip": np.asarray(skip, np.uint8), "mp_desc": desc}
        return R.search_local_points(self.oracle, self.frame, Rcw, tcw, Ow, pts, np.asarray(blocks, np.uint8), (fx, fy, cx, cy, bf), R.BOUNDS, log_sf, sf, th, self.mfNNratio, tb, limit)

    def close(self):
        pass


def test_python_mirror_bookkeeping(oracle, monkeypatch):
    from cube_slam_amd import tracking
    frames = S.frames(oracle)
    cm = R.chain_map(frames)
    F0 = S.make_frame(oracle, *frames[0])
    want = R.track_local_map(oracle, F0, cm)
    assert want["ok"] and want["inliers"] >= 100 and len(want["local_kf"]) >= 15 and len(want["local_points"]) >= 1500 and want["search"]["nmatches"] >= 300
    monkeypatch.setattr(tracking, "track_local_points", lambda ctx, off, mp, skip: R.update_local_points(off, mp, skip))
    monkeypatch.setattr(tracking, "PoseOptimization", lambda fr, ctx=None: [oracle.pose_optimization(f["Xw"], f["obs"], f["inv_sigma2"], f["intr"], f["pose"]) for f in fr])
    t = tracking.Tracking.__new__(tracking.Tracking)
    t.ctx = None
    t.mSensor, t.whether_dynamic_object, t.whether_detect_object, t.mbOnlyTracking, t.mMaxFrames = 0, False, False, False, 30
    t.matcher = _FakeMatcher(oracle)
    t.mvpLocalKeyFrames = t.mvpLocalMapPoints = np.zeros(0, np.int32)
    t.mpReferenceKF, t.mnLastRelocFrameId, t.mnMatchesInliers, t.last_search = -1, -10 ** 9, 0, None
    m, F = R.chain_objects(frames, cm)
    ok = t.TrackLocalMap(F, m)
    assert ok == want["ok"] and t.mnMatchesInliers == want["inliers"] and t.mpReferenceKF == want["kf_max"]
    assert np.array_equal(t.mvpLocalKeyFrames, want["local_kf"]) and np.array_equal(t.mvpLocalMapPoints, want["local_points"]) and np.array_equal(F.mvpMapPoints, want["frame_mp"])
    assert np.array_equal(F.mvbOutlier, want["outlier"]) and np.array_equal(F.pose7, want["pose"])
    lp = want["local_points"]
    vis = np.zeros(len(cm["bad"]), np.int64)
    own = cm["frame_mp"][cm["frame_mp"] >= 0]
    np.add.at(vis, own[cm["bad"][own] == 0], 1)
    np.add.at(vis, lp[want["search"]["in_view"] != 0], 1)
    assert np.array_equal(m.visible, vis) and m.found.sum() == int((want["outlier"][want["frame_mp"] >= 0] == 0).sum())
    # just relocalised: th = 5 and the stricter threshold
    t.mnLastRelocFrameId = R.CHAIN_FRAME_ID - 1
    m, F = R.chain_objects(frames, cm)
    t.TrackLocalMap(F, m)
    assert np.array_equal(F.mvpMapPoints, R.track_local_map(oracle, F0, cm, th=5.0)["frame_mp"])
