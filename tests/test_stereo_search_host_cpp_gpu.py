"""GPU: the C++ mirrors of the stereo searches -- cubeslam::ORBmatcher::set_u_right / SearchByProjection(CurrentFrame, LastFrame, th, bMono)
(cube_slam_amd/host/orb_slam_mirrors.hpp) and cubeslam::Tracking::TrackWithMotionModel with the TrackLocalMap that follows it (cube_slam_amd/host/tracking.hpp) -- compiled with g++
against the C-ABI library through tests/cpp/track_motion_model_mirror.cpp: byte-equal to the Python mirror (cube_slam_amd/tracking.py) on the two cases of
tests/test_track_with_motion_model_chain_gpu.py (the first search succeeds; the retry at 2 th runs) -- the last frame's slots and the created points, the matches, outlier flags,
poses, counts, direction, return values, and the local-map search with the mvuRight test."""
import os
import subprocess

import numpy as np
import pytest

from tests import track_local_map_restatement as TL
from tests import track_motion_model_restatement as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    e = str(tmp_path_factory.mktemp("track_motion_model_mirror") / "track_motion_model_mirror")
    lib_dir = os.path.join(ROOT, "cube_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-I", ROOT, os.path.join(ROOT, "tests", "cpp", "track_motion_model_mirror.cpp"), "-o", e, "-L", lib_dir,
                           "-lcubeslam_hip", "-Wl,-rpath," + lib_dir])
    return e


@pytest.mark.parametrize("retry", [False, True], ids=["first_search", "retry_at_2th"])
def test_cpp_mirror_equals_python_mirror(ctx, exe, tmp_path, retry):
    from cube_slam_amd.tracking import LastFrame, Map, TrackedFrame, Tracking
    seq = R.sequence()
    frames, mp, g = seq["frames"], seq["map"], R.graph(seq)
    last_f, cur = frames[1], frames[2]
    ur, _ = R.stereo_of(cur)
    _, depth_last = R.stereo_of(last_f)
    f32, i32 = np.float32, np.int32
    pred = R.predicted(seq, retry)
    arrays = [mp["world_pos"].astype(f32), mp["normal"].astype(f32), mp["min_distance"].astype(f32), mp["max_distance"].astype(f32), mp["mp_desc"].astype(np.uint8), mp["n_obs"].astype(i32),
              g["obs_off"], g["obs_kf"], g["kf_off"], g["kf_mp"], g["kf_bad"], g["cov_off"], g["cov_kf"], g["child_off"], g["child_kf"], g["parent"],
              last_f["keys"], last_f["desc"], seq["last_mp"].astype(i32), depth_last.astype(f32), last_f["Tcw"].astype(f32),
              cur["keys"], cur["desc"], ur.astype(f32), np.asarray(R.BOUNDS, f32), np.asarray(list(R.INTR) + [R.LOG_SF], f32), R.SF.astype(f32), R.ISG.astype(f32),
              pred.astype(f32), R.K4.astype(f32), np.asarray([R.TH_DEPTH], f32), np.asarray([R.FRAME_ID, Tracking.RGBD], i32)]
    (tmp_path / "in.bin").write_bytes(TL.pack(arrays))
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], timeout=60)
    m = Map(world_pos=mp["world_pos"].copy(), normal=mp["normal"].copy(), min_distance=mp["min_distance"].copy(), max_distance=mp["max_distance"].copy(), desc=mp["mp_desc"].copy(),
            bad=np.zeros(seq["n"], np.uint8), n_obs=mp["n_obs"].copy(), **g)
    t = Tracking(ctx=ctx, sensor=Tracking.RGBD)
    last = LastFrame(last_f["keys"], last_f["desc"], seq["last_mp"], last_f["Tcw"], mvDepth=depth_last)
    F = TrackedFrame(R.FRAME_ID, cur["keys"], cur["desc"], R.BOUNDS, np.full(len(cur["keys"]), -1, i32), np.eye(3, dtype=f32), np.zeros(3, f32), np.zeros(3, f32), R.INTR, R.LOG_SF, R.SF,
                     R.ISG, np.zeros(7), u_right=ur)
    ok = t.TrackWithMotionModel(F, last, m, pred, K4=R.K4, mThDepth=R.TH_DEPTH)
    assert ok and t.retried == retry and t.nmatches >= 100 and len(t.mlpTemporalPoints) >= 50
    want = [last.mvpMapPoints.astype(i32), np.asarray(t.mlpTemporalPoints, i32), F.mvpMapPoints.astype(i32), t.last_outliers.astype(np.uint8), F.pose7.astype(np.float64),
            np.asarray([int(ok), t.nmatches, t.nmatchesMap, t.matcher.last_direction, int(t.retried), len(m.bad)], i32),
            np.asarray(F.Rcw, f32).reshape(-1), np.asarray(F.tcw, f32), np.asarray(F.Ow, f32)]
    ok2 = t.TrackLocalMap(F, m)
    s = t.last_search
    t.close()
    assert s["nmatches"] >= 20
    want += [t.mvpLocalKeyFrames.astype(i32), t.mvpLocalMapPoints.astype(i32), s["train_match"].astype(i32), s["in_view"].astype(np.uint8), s["proj"].astype(f32),
             F.mvpMapPoints.astype(i32), F.mvbOutlier.astype(np.uint8), F.pose7.astype(np.float64),
             np.asarray([s["nmatches"], s["n_to_match"], s["outside"], t.mnMatchesInliers, int(ok2), t.mpReferenceKF], i32), m.visible.astype(np.int64), m.found.astype(np.int64),
             m.last_frame_seen.astype(np.int64)]
    assert (tmp_path / "out.bin").read_bytes() == TL.pack(want)
