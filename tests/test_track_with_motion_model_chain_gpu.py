"""GPU: Tracking::TrackWithMotionModel end to end for a depth sensor (reference orb_object_slam/src/Tracking.cc:1276-1354), then TrackLocalMap with the stereo local-map search,
through the Python mirror (cube_slam_amd/tracking.py) on one synthetic RGB-D sequence of three frames (tests/track_motion_model_restatement.py): cs_rgbd_from_keys leaves mvuRight /
mvDepth on the device, UpdateLastFrame creates its close points from there, cs_matcher_set_u_right takes mvuRight from cs_rgbd_device_frame, the stereo search runs at th = 15 (and
again at 30 in the retry variant), PoseOptimization, the outlier loop -- held to the same chain through the restatements: match vectors, outlier flags, nmatches, nmatchesMap and
the return values are equal; the poses are within the bound tests/test_track_local_map_chain_gpu.py holds the device PoseOptimization to against the same oracle (atol 1e-8)."""
import numpy as np
import pytest

from cube_slam_amd.rgbd import RGBDAssociator
from cube_slam_amd.tracking import LastFrame, Map, TrackedFrame, Tracking
from tests import stereo_search_restatement as SR
from tests import track_motion_model_restatement as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def seq():
    return R.sequence()


@pytest.mark.parametrize("retry", [False, True], ids=["first_search", "retry_at_2th"])
def test_track_with_motion_model_chain(ctx, oracle, seq, retry):
    want = R.chain(oracle, seq, retry)
    # the preconditions, on the CPU: the camera moved forward by more than a baseline, UpdateLastFrame created points, the variant takes the branch it is named after
    assert want["direction"] == SR.FORWARD and want["n_created"] >= 50 and want["retried"] == retry and (want["first_nmatches"] < 20) == retry
    assert want["ok"] and want["nmatches"] >= 100 and want["nmatchesMap"] >= 50 and want["ok2"] and want["local_n"] >= 20 and want["local_differs"]
    frames, mp = seq["frames"], seq["map"]
    g = R.graph(seq)
    m = Map(world_pos=mp["world_pos"].copy(), normal=mp["normal"].copy(), min_distance=mp["min_distance"].copy(), max_distance=mp["max_distance"].copy(), desc=mp["mp_desc"].copy(),
            bad=np.zeros(seq["n"], np.uint8), n_obs=mp["n_obs"].copy(), **g)
    a = RGBDAssociator(R.W, R.H, max(len(f["keys"]) for f in frames), 1, ctx=ctx)
    t = Tracking(ctx=ctx, sensor=Tracking.RGBD)
    # the last frame alone on the device: UpdateLastFrame reads its depths there
    a.upload_depth(frames[1]["depth"][None])
    a.from_keys([frames[1]["keys"]], [frames[1]["keys"]], float(R.BF), 1.0)
    last = LastFrame(frames[1]["keys"], frames[1]["desc"], seq["last_mp"], frames[1]["Tcw"], rgbd=a)
    cur = frames[2]
    ur, _ = R.stereo_of(cur)
    F = TrackedFrame(R.FRAME_ID, cur["keys"], cur["desc"], R.BOUNDS, np.full(len(cur["keys"]), -1, np.int32), np.eye(3, dtype=np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32),
                     R.INTR, R.LOG_SF, R.SF, R.ISG, np.zeros(7), u_right=ur)
    # UpdateLastFrame first (it needs the last frame on the handle), then the current frame's mvuRight on a handle of its own
    b = RGBDAssociator(R.W, R.H, len(cur["keys"]), 1, ctx=ctx)
    b.upload_depth(cur["depth"][None])
    b.from_keys([cur["keys"]], [cur["keys"]], float(R.BF), 1.0)
    du, _, _, dn = b.device_frame(0)
    assert dn == len(cur["keys"])
    F.u_right_device = du
    ok = t.TrackWithMotionModel(F, last, m, R.predicted(seq, retry), K4=R.K4, mThDepth=R.TH_DEPTH)
    assert t.matcher.last_direction == want["direction"] and t.retried == want["retried"]
    assert np.array_equal(last.mvpMapPoints, want["last_mp"]) and len(m.bad) == seq["n"] + want["n_created"]
    assert ok == want["ok"] and t.nmatches == want["nmatches"] and t.nmatchesMap == want["nmatchesMap"]
    assert np.array_equal(t.last_outliers, want["outlier"]) and np.array_equal(F.mvpMapPoints, want["frame_mp"])
    assert np.allclose(F.pose7, want["pose"], rtol=0, atol=1e-8)
    ok2 = t.TrackLocalMap(F, m)
    s = t.last_search
    assert np.array_equal(t.mvpLocalKeyFrames, want["local_kf"]) and np.array_equal(t.mvpLocalMapPoints, want["local_points"])
    assert np.array_equal(s["train_match"], want["local_tm"]) and s["nmatches"] == want["local_n"] and s["n_to_match"] == want["n_to_match"]
    assert np.array_equal(F.mvpMapPoints, want["frame_mp2"]) and np.array_equal(F.mvbOutlier, want["outlier2"])
    assert t.mnMatchesInliers == want["inliers"] and ok2 == want["ok2"]
    assert np.allclose(F.pose7, want["pose2"], rtol=0, atol=1e-8)
    t.close(); a.close(); b.close()
