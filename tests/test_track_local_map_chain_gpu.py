"""GPU: Tracking::TrackLocalMap end to end (reference orb_object_slam/src/Tracking.cc:1356-1416) -- UpdateLocalMap -> SearchLocalPoints -> PoseOptimization -> statistics -- through
the Python mirror (cube_slam_amd/tracking.py) on one seeded synthetic map of 20 key frames, held to the restatement chain (tests/track_local_map_restatement.py, whose pose step is
the CPU oracle's PoseOptimization): local key frames, local points, matches and the inlier count are equal; the pose is within the tolerance tests/test_pose_gpu.py holds the device
PoseOptimization to against the same oracle."""
import numpy as np
import pytest

from cube_slam_amd.tracking import Tracking
from tests import sim3_restatement as S
from tests import track_local_map_restatement as R

pytestmark = pytest.mark.gpu


def test_track_local_map_chain(ctx, oracle):
    frames = S.frames(oracle)
    cm = R.chain_map(frames)
    want = R.track_local_map(oracle, S.make_frame(oracle, *frames[0]), cm)
    assert want["ok"] and want["inliers"] >= 100 and len(want["local_kf"]) >= 15 and len(want["local_points"]) >= 1500 and want["search"]["nmatches"] >= 300
    m, F = R.chain_objects(frames, cm)
    t = Tracking(ctx=ctx)
    ok = t.TrackLocalMap(F, m)
    s, ws = t.last_search, want["search"]
    t.close()
    assert np.array_equal(t.mvpLocalKeyFrames, want["local_kf"]) and t.mpReferenceKF == want["kf_max"]
    assert np.array_equal(t.mvpLocalMapPoints, want["local_points"])
    assert np.array_equal(s["train_match"], ws["train_match"]) and (s["nmatches"], s["n_to_match"], s["outside"]) == (ws["nmatches"], ws["n_to_match"], ws["outside"])
    assert np.array_equal(s["in_view"], ws["in_view"]) and np.array_equal(F.mvpMapPoints, want["frame_mp"])
    assert t.mnMatchesInliers == want["inliers"] and ok == want["ok"]
    assert np.allclose(F.pose7, want["pose"], rtol=0, atol=1e-8)
    assert (F.mvbOutlier != want["outlier"]).sum() <= len(want["outlier"]) // 1000  # (a chi2 on the threshold within round-off, as tests/test_pose_gpu.py allows)
