"""GPU chain, one step further than tests/test_gftt_chain_gpu.py, on its small frames: new Harris features on frame 0 (cs_track_new_harris_features), SearchByTrackingHarris
0 -> 1 (cs_match_by_tracking_harris), then the triangulation of every tracked point against the last key frame with a known object motion (cs_triangulate_dynamic_points), and
the dpoints that come out go into cs_ba_dyn_* together with the observation lists of the two key frames.  Every step equals the restatements run through the same steps.

The scene: the camera stands still (gp.TWC), the texture moves by (2, 1) pixels a frame, and the two cuboids (depths gp.CHAIN_DEPTH) move parallel to the image plane by
(2 d / fx, 1 d / fy): the motion that makes a point of the cuboid's depth move by exactly the texture's shift, so the parallax the triangulation sees is the object's own and
x3D comes out at the cuboid's depth, where the point was created."""
import numpy as np
import pytest

from cube_slam_amd.klt import KLTTracker
from tests import gftt_patterns as gp
from tests import klt_patterns as kp
from tests import object_points_restatement as R

pytestmark = pytest.mark.gpu


def _scene():
    """Tcw (12 floats, both key frames), the camera's 7-vector, and the cuboid tables of the two key frames."""
    Twc = gp.TWC.astype(np.float64)
    Rwc, Ow = Twc[:, :3], Twc[:, 3]
    Tcw = np.concatenate([Rwc.T, (-Rwc.T @ Ow)[:, None]], 1)
    w = np.sqrt(1.0 + np.trace(Rwc.T)) / 2  # the rotation turns about z by less than a quarter turn: the trace is positive
    Rcw = Rwc.T
    cam7 = np.array([*Tcw[:, 3], (Rcw[2, 1] - Rcw[1, 2]) / (4 * w), (Rcw[0, 2] - Rcw[2, 0]) / (4 * w), (Rcw[1, 0] - Rcw[0, 1]) / (4 * w), w])
    last, now = [], []
    for d in gp.CHAIN_DEPTH.astype(np.float64):
        centre = Rwc @ np.array([0.0, 0.0, d]) + Ow
        move = Rwc @ np.array([2.0 * d / float(gp.K4[0]), 1.0 * d / float(gp.K4[1]), 0.0])
        last.append([*centre, 0.0, 0.0, 0.0, 1.0]); now.append([*(centre + move), 0.0, 0.0, 0.0, 1.0])
    return Tcw.astype(np.float32).reshape(-1), cam7, np.array(last), np.array(now)


def _triangulation_inputs(f0, step, x3D0):
    Tcw, _, last, now = _scene()
    kept = step["kept"]
    return dict(first=np.array([0, len(kept)], np.int32), Tcw_last=Tcw, Tcw_now=Tcw, K4=gp.K4, cub_first_last=np.array([0, 2], np.int32), cub_pose_last=last,
                cub_first_now=np.array([0, 2], np.int32), cub_pose_now=now, kp1=f0[2][kept], kp2=step["pts"], obj_last=f0[1][kept], obj_now=step["object_id"],
                idx_last=kept.astype(np.int32), world_pos=x3D0[kept], tracklet_last=np.array([11, 12], np.int32), tracklet_now=np.array([11, 12], np.int32))


def _problem(f0, step, x3D0, tri):
    """The two key frames as a dynamic-BA window: one cuboid vertex per (object, key frame), the observation lists of tests/klt_patterns.py with the object of an observation
    mapped to its vertex, PosToObj of the triangulated points from the triangulation and of the others from where they were created (MapPoint::SetWorldPos, the caller's)."""
    _, cam7, last, now = _scene()
    lists = kp.dobs_lists([f0, kp.chain_step(step, f0[0])])
    dp = np.zeros((len(f0[0]), 3))
    for i in range(len(dp)):
        dp[i] = R.se3_map(R.se3_inv(R.se3_load(last[f0[1][i]])), [float(v) for v in x3D0[i]])
    ok = tri["status"] == 0
    dp[f0[0][step["kept"][ok]]] = tri["dpoints"][ok]
    n = len(lists["dobs_cam"])
    K = np.array([[gp.K4[0], 0, gp.K4[2]], [0, gp.K4[1], gp.K4[3]], [0, 0, 1]], np.float64)
    z = np.zeros
    return {"cam_pose": np.stack([cam7, cam7]), "cam_fixed": np.ones(2, np.uint8), "obj_pose": np.concatenate([last, now]), "obj_scale": np.tile([0.6, 0.4, 0.5], (4, 1)),
            "obj_flags": np.full(4, 2 | 8, np.uint8), "vel": z((0, 2)), "points": z((0, 3)), "dpoints": dp, "fix_points": 0, "obs_cam": z(0, np.int32), "obs_point": z(0, np.int32),
            "obs_uv": z((0, 2)), "obs_ur": z(0), "obs_inv_sigma2": z(0), "obs_level": z(0, np.uint8), "fx": float(gp.K4[0]), "fy": float(gp.K4[1]), "cx": float(gp.K4[2]),
            "cy": float(gp.K4[3]), "bf": 40.0, "huber_mono": 5.991 ** 0.5, "huber_stereo": 7.815 ** 0.5, "ulp_info": 10.0, "ulp_scale": np.array([0.6, 0.4, 0.5]), "ulp_ratio": 2.0,
            "dobs_cam": lists["dobs_cam"], "dobs_obj": (2 * lists["dobs_cam"] + lists["dobs_obj"]).astype(np.int32), "dobs_point": lists["dobs_point"], "dobs_uv": lists["dobs_uv"],
            "dobs_inv_sigma2": np.ones(n), "dobs_level": z(n, np.uint8), "K": K, "huber_dyn": 5.991 ** 0.5, "mot_from": z(0, np.int32), "mot_to": z(0, np.int32),
            "mot_vel": z(0, np.int32), "mot_dt": z(0), "mot_info": np.array([0.25, 0.25, 6.25]), "cobs_cam": z(0, np.int32), "cobs_obj": z(0, np.int32), "cobs_bbox": z((0, 4)),
            "cobs_info": z((0, 4)), "cobs_level": z(0, np.uint8), "huber_obj": 30.0, "pc_obj": z(0, np.int32), "pc_offsets": z(1, np.int32), "pc_points": z((0, 3)), "pc_ratio": 2.0}


def test_detect_track_triangulate_feeds_the_dynamic_ba(ctx):
    from cube_slam_amd import object_points as O
    from cube_slam_amd.ba_dynamic import DynamicBundleAdjuster
    c = gp.chain_case()
    frames, masks = c["frames"], c["masks"]
    t = KLTTracker(3, frames.shape[2], frames.shape[1], 256, ctx=ctx)
    try:
        t.set_frames(frames)
        none = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2), np.float32))
        f0, r0 = gp.chain_new_features(frames[0], masks[0], none, lambda p, o: t.new_harris_features([0], masks[0:1], [p], [o], gp.K4, gp.TWC[None], [gp.CHAIN_DEPTH], good_masks=True)[0])
        assert gp.same_harris(r0, c["new0"])
        step = t.search_by_tracking_harris([(0, 1)], [f0[2]], masks[1:2])[0]
        assert kp.same_harris(step, c["step"]) and step["goodmatches"] >= 20
    finally:
        t.close()
    a = _triangulation_inputs(f0, step, r0["x3D"])
    run = lambda cx: O.triangulate_dynamic_points(cx, a["first"], a["Tcw_last"], a["Tcw_now"], a["K4"], a["cub_first_last"], a["cub_pose_last"], a["cub_first_now"], a["cub_pose_now"],
                                                  a["kp1"], a["kp2"], a["obj_last"], a["obj_now"], a["idx_last"], a["world_pos"], a["tracklet_last"], a["tracklet_now"])
    tri = run(ctx)
    # the same steps on the restatements: the chain case's own frame 0 and tracking result, then the restated triangulation
    want = R.triangulate_dynamic_points(_triangulation_inputs(c["per_frame"][0], c["step"], c["new0"]["x3D"]))
    host = run(None)
    for key in ("status", "x3D", "pos_to_obj", "dpoints"):
        assert tri[key].tobytes() == want[key].tobytes() == host[key].tobytes() and tri[key].shape == want[key].shape, key
    ok = tri["status"] == O.TRIANGULATED
    assert int(ok.sum()) >= 20 and set(tri["status"].tolist()) <= {O.TRIANGULATED, O.TRACKLET, O.TOO_FAR}
    # x3D is the point's place in the last key frame: at its cuboid's depth, within the few centimetres a hundredth of a pixel of tracking error is worth there
    assert np.abs(np.linalg.norm(tri["x3D"][ok].astype(np.float64) - a["world_pos"][ok], axis=1)).max() < 0.5
    assert np.array_equal(tri["dpoints"], tri["pos_to_obj"].astype(np.float64))
    d = _problem(f0, step, r0["x3D"], tri)
    assert len(d["dobs_cam"]) == len(f0[0]) + len(step["kept"]) and d["dobs_obj"].max() <= 3 and d["dobs_point"].max() < len(d["dpoints"])
    ba = DynamicBundleAdjuster(d, ctx=ctx)  # cs_ba_dyn_create: no CS_ERR_*
    try:
        st = ba.optimize(5)
        got = ba.read()
    finally:
        ba.close()
    assert np.isfinite(st["chi2_init"]) and np.isfinite(st["chi2_final"]) and st["chi2_final"] <= st["chi2_init"]
    assert got["dpoints"].shape == d["dpoints"].shape and np.isfinite(got["dpoints"]).all() and np.isfinite(got["obj_pose"]).all()
