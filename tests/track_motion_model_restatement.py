"""Judge of Tracking.TrackWithMotionModel (cube_slam_amd/tracking.py; reference orb_object_slam/src/Tracking.cc:1276-1354) followed by TrackLocalMap with the stereo local-map
search: one synthetic RGB-D sequence of three frames and the chain over it through the restatements -- Frame::ComputeStereoFromRGBD and the close-point rule of UpdateLastFrame
(tests/rgbd_restatement.py), the stereo searches (tests/stereo_search_restatement.py) over the oracle's GetFeaturesInArea, the oracle's PoseOptimization, the outlier loop, and
UpdateLocalKeyFrames / UpdateLocalPoints / isInFrustum of tests/track_local_map_restatement.py.  A helper, not a test module.

The sequence: 600 world points 4 - 30 m in front of a camera (KITTI's intrinsics, baseline 0.535 m) that moves 0.7 m forward per frame -- more than a baseline, so the search goes
`forward` -- with a slight yaw.  Frame f holds the projections of the points it sees (0.3 px of noise, levels 0 and 1, a descriptor 5 bits from the point's), in a shuffled order,
and a depth image that carries each key point's depth under its pixel (for 15 % of them twice the true depth).  Frame 0 is the key frame (two key frames hold its points), frame 1 the last frame (it carries the map points
of 60 % of its key points; UpdateLastFrame creates visual-odometry points for the close ones of the rest), frame 2 the current frame."""
import numpy as np

from cube_slam_amd import synth
from cube_slam_amd.orb import KEYPOINT_DTYPE
from tests import rgbd_restatement as rr
from tests import stereo_search_restatement as SR
from tests import track_local_map_restatement as TL

f32, f64 = np.float32, np.float64
INTR, BOUNDS, SF, LOG_SF = TL.INTR, TL.BOUNDS, TL.SF, TL.LOG_SF
K4 = np.array(INTR[:4], np.float32)
BF = f32(INTR[4])
MB = f32(BF / f32(INTR[0]))
TH_DEPTH = 15.0
W, H = int(BOUNDS[1]), int(BOUNDS[3])
ISG = (f32(1.0) / (SF * SF)).astype(f32)
FRAME_ID = 10


def pose_of(f, yaw=0.004, dx=0.0):
    T = np.zeros((3, 4), f32)
    T[:, :3] = synth._rot(1, yaw * f)
    T[:, 3] = (dx, 0.0, -0.7 * f)
    return T


def tcw_of_pose7(p):
    """The 3x4 float pose of (t, qx, qy, qz, qw): what Frame::SetPose receives after PoseOptimization (the quaternion's rotation matrix in double, stored as float)."""
    x, y, z, w = [f64(v) for v in p[3:7]]
    Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], f64)
    return np.concatenate([Rm, np.asarray(p[:3], f64).reshape(3, 1)], axis=1).astype(f32)


def sequence(seed=21, n=600):
    rng = np.random.default_rng(seed)
    z = rng.uniform(4.0, 30.0, n)
    Xw = np.stack([(rng.uniform(40, W - 40, n) - INTR[2]) / INTR[0] * z, (rng.uniform(30, H - 30, n) - INTR[3]) / INTR[1] * z, z], axis=1).astype(f32)
    base = rng.integers(0, 256, (n, 32)).astype(np.uint8)
    level = rng.integers(0, 2, n)
    angle = rng.uniform(0, 360, n).astype(f32)
    frames = []
    for f in range(3):
        T = pose_of(f).astype(f64)
        Pc = Xw.astype(f64) @ T[:, :3].T + T[:, 3]
        u, v = INTR[0] * Pc[:, 0] / Pc[:, 2] + INTR[2], INTR[1] * Pc[:, 1] / Pc[:, 2] + INTR[3]
        vis = np.nonzero((Pc[:, 2] > 1.0) & (u > 20) & (u < W - 20) & (v > 20) & (v < H - 20))[0]
        vis = rng.permutation(vis)
        k = np.zeros(len(vis), KEYPOINT_DTYPE)
        k["x"] = (u[vis] + rng.uniform(-0.3, 0.3, len(vis))).astype(f32); k["y"] = (v[vis] + rng.uniform(-0.3, 0.3, len(vis))).astype(f32)
        k["size"], k["angle"], k["octave"], k["class_id"] = 31.0, angle[vis], level[vis], -1
        d = base[vis].copy()
        for i in range(len(vis)):
            for b in rng.choice(256, 5, replace=False):
                d[i, b // 8] ^= np.uint8(1 << (b % 8))
        depth = np.zeros((H, W), f32)
        zk = Pc[vis, 2].astype(f32)
        zk[rng.uniform(size=len(vis)) < 0.15] *= f32(2.0)  # a sensor that is wrong about every seventh key point: its right coordinate disagrees with the map
        depth[k["y"].astype(int), k["x"].astype(int)] = zk
        frames.append({"keys": k, "desc": d, "point": vis, "depth": depth, "Tcw": pose_of(f)})
    # the map: every world point is a map point; the ones frame 0 sees are observed by key frame 0, every second of them by key frame 1 as well
    seen0 = frames[0]["point"]
    n_obs = np.zeros(n, np.int32); n_obs[seen0] = 1; n_obs[seen0[::2]] = 2
    kf_lists = [seen0.astype(np.int32), seen0[::2].astype(np.int32)]
    obs = [([0] if n_obs[p] >= 1 else []) + ([1] if n_obs[p] == 2 else []) for p in range(n)]
    dist = np.sqrt((Xw.astype(f64) ** 2).sum(1))
    maxd = (dist * 1.2 ** level * 1.1).astype(f32)
    normal = (Xw / dist[:, None]).astype(f32)  # seen from the first camera's centre
    mp = {"world_pos": Xw, "normal": normal, "min_distance": (maxd / f32(1.2 ** 7)).astype(f32), "max_distance": maxd, "mp_desc": base, "n_obs": n_obs, "kf_lists": kf_lists, "obs": obs}
    # the last frame carries the map points of 60 % of its key points (those with observations)
    last = frames[1]
    lm = np.where((rng.uniform(size=len(last["point"])) < 0.6) & (n_obs[last["point"]] > 0), last["point"], -1).astype(np.int64)
    return {"frames": frames, "map": mp, "last_mp": lm, "n": n}


def predicted(seq, retry):
    """mVelocity * mLastFrame.mTcw: the current frame's true pose moved by 2 cm -- or, for the retry variant, yawed by 0.03 rad (about 21 px: outside the windows of 15 and
    18 px, inside those of 30 and 36)."""
    T = pose_of(2, dx=0.02)
    if retry:
        T[:, :3] = synth._rot(1, 0.004 * 2 + 0.03)
    return T


def stereo_of(fr):
    """(mvuRight, mvDepth) of a frame: Frame::ComputeStereoFromRGBD over its depth image (float metres, factor 1; no distortion: mvKeysUn = mvKeys)."""
    u, d, _, _ = rr.compute_stereo_from_rgbd(fr["depth"], 1.0, fr["keys"], fr["keys"], BF)
    return u, d


def _csr(lists):
    off = np.zeros(len(lists) + 1, np.int32)
    off[1:] = np.cumsum([len(l) for l in lists])
    return off, (np.concatenate([np.asarray(l, np.int32) for l in lists]) if off[-1] else np.zeros(0, np.int32)).astype(np.int32)


def graph(seq):
    """The two key frames' tables: each other's covisible, key frame 1 the child of 0."""
    kf_off, kf_mp = _csr(seq["map"]["kf_lists"])
    obs_off, obs_kf = _csr(seq["map"]["obs"])
    cov_off, cov_kf = _csr([[1], [0]])
    child_off, child_kf = _csr([[1], []])
    return dict(kf_off=kf_off, kf_mp=kf_mp, obs_off=obs_off, obs_kf=obs_kf, kf_bad=np.zeros(2, np.uint8), cov_off=cov_off, cov_kf=cov_kf, child_off=child_off, child_kf=child_kf,
                parent=np.array([-1, 0], np.int32))


def chain(oracle, seq, retry):
    """TrackWithMotionModel, then TrackLocalMap with the stereo local-map search, through the restatements -> a dict of everything the GPU test compares."""
    cur, last, mp = seq["frames"][2], seq["frames"][1], seq["map"]
    n = seq["n"]
    ur_cur, _ = stereo_of(cur)
    _, depth_last = stereo_of(last)
    # UpdateLastFrame (:1215-1273): visual-odometry points for the close key points without a map point (or whose point has no observations)
    lm = seq["last_mp"].copy()
    need_new = ((lm < 0) | (mp["n_obs"][np.maximum(lm, 0)] < 1)).astype(np.uint8)
    cp = rr.close_points(depth_last, last["keys"], need_new, last["Tcw"], K4, TH_DEPTH, rr.NEAREST)
    new_idx, new_x3D = np.asarray(cp["new_idx"], np.int64), np.asarray(cp["new_x3D"], f32).reshape(-1, 3)
    lm[new_idx] = n + np.arange(len(new_idx))
    wp = np.concatenate([mp["world_pos"], new_x3D]); desc = np.concatenate([mp["mp_desc"], last["desc"][new_idx]]); n_obs = np.concatenate([mp["n_obs"], np.zeros(len(new_idx), np.int32)])
    Tcw = predicted(seq, retry)
    F = oracle.make_frame(cur["keys"], cur["desc"], BOUNDS)
    area_fn = lambda x, y, r, lo, hi: [int(i) for i in oracle.get_features_in_area(F, x, y, r, lo, hi)]
    has = lm >= 0
    pm = np.where(has, lm, 0)

    def search(th):
        return SR.search_by_projection_frame(cur["keys"], cur["desc"], BOUNDS, ur_cur, wp[pm], has.astype(np.uint8), (n_obs[pm] > 0).astype(np.uint8), desc[pm], last["keys"]["octave"],
                                             last["keys"]["angle"], Tcw, last["Tcw"], INTR[:4], BF, MB, 0, SF, th, True, None, area_fn=area_fn)
    first = search(15.0)  # an RGB-D sensor: th = 15 (:1293-1296), bMono = false
    tm, nmatches, direction, _ = first if first[1] >= 20 else search(30.0)
    out = {"first_nmatches": first[1], "retried": first[1] < 20, "direction": direction, "n_created": len(new_idx), "last_mp": lm}
    frame_mp = np.where(tm >= 0, lm[np.maximum(tm, 0)], -1).astype(np.int64)
    out["search_mp"] = frame_mp.copy()
    if nmatches < 20:
        out.update(ok=False, nmatches=nmatches)
        return out
    pose0 = synth._pose7(Tcw[:, :3].astype(f64), Tcw[:, 3].astype(f64))
    idx = np.nonzero(frame_mp >= 0)[0]
    obs = np.stack([cur["keys"]["x"][idx], cur["keys"]["y"][idx], ur_cur[idx]], axis=1).astype(f64)
    pose, flags, _ = oracle.pose_optimization(wp[frame_mp[idx]].astype(f64), obs, ISG[cur["keys"]["octave"][idx]].astype(f64), np.asarray(INTR, f32).astype(f64), pose0)
    outlier = np.zeros(len(cur["keys"]), np.uint8); outlier[idx] = flags
    nmap = 0
    seen = np.zeros(len(wp), bool)
    for i in idx:  # :1326-1345
        if outlier[i]:
            seen[frame_mp[i]] = True  # pMP->mnLastFrameSeen = mCurrentFrame.mnId (:1338): SearchLocalPoints skips it (:2702)
            frame_mp[i] = -1; nmatches -= 1
        elif n_obs[frame_mp[i]] > 0:
            nmap += 1
    out.update(pose=pose, outlier=outlier, nmatches=nmatches, nmatchesMap=nmap, ok=nmap >= 10, frame_mp=frame_mp.copy())
    # TrackLocalMap (:1356-1416) on the frame as TrackWithMotionModel left it, RGB-D: th = 3, the mvuRight test in the search
    g = graph(seq)
    bad = np.zeros(len(wp), np.uint8)
    obs_off = np.concatenate([g["obs_off"], np.full(len(new_idx), g["obs_off"][-1], np.int32)])
    local_kf, kfmax = TL.update_local_keyframes(frame_mp.astype(np.int32), bad, obs_off, g["obs_kf"], g["kf_bad"], g["cov_off"], g["cov_kf"], g["child_off"], g["child_kf"], g["parent"])
    off, lst = _csr([g["kf_mp"][g["kf_off"][j]:g["kf_off"][j + 1]] for j in local_kf])
    lp = TL.update_local_points(off, lst, bad)
    T2 = tcw_of_pose7(pose)
    Ow = np.array([f32(-sum(f64(T2[k, r]) * f64(T2[k, 3]) for k in range(3))) for r in range(3)], f32)
    seen[frame_mp[frame_mp >= 0]] = True
    pts = {"world_pos": mp["world_pos"][lp], "normal": mp["normal"][lp], "min_distance": mp["min_distance"][lp], "max_distance": mp["max_distance"][lp], "mp_desc": mp["mp_desc"][lp],
           "skip": seen[lp].astype(np.uint8)}
    fr = TL.frustum_all(pts, T2[:, :3], T2[:, 3], Ow, INTR, BOUNDS, LOG_SF, len(SF))
    tb = np.zeros(len(cur["keys"]), np.uint8)
    held = frame_mp >= 0
    tb[held] = n_obs[frame_mp[held]] > 0
    tm2, n2, _, _ = SR.search_local_map(cur["keys"], cur["desc"], BOUNDS, ur_cur, fr["proj"][:, :2], fr["proj"][:, 2], fr["view_cos"], np.maximum(fr["pred_level"], 0), fr["in_view"],
                                        (mp["n_obs"][lp] > 0).astype(np.uint8), pts["mp_desc"], SF, 3.0, 0.8, tb, area_fn=area_fn)
    mono2 = SR.search_local_map(cur["keys"], cur["desc"], BOUNDS, ur_cur, fr["proj"][:, :2], fr["proj"][:, 2], fr["view_cos"], np.maximum(fr["pred_level"], 0), fr["in_view"],
                                (mp["n_obs"][lp] > 0).astype(np.uint8), pts["mp_desc"], SF, 3.0, 0.8, tb, area_fn=area_fn, stereo_test=False)[0]
    got = tm2 >= 0
    frame_mp[got] = lp[tm2[got]]
    idx = np.nonzero(frame_mp >= 0)[0]
    obs = np.stack([cur["keys"]["x"][idx], cur["keys"]["y"][idx], ur_cur[idx]], axis=1).astype(f64)
    pose2, flags2, _ = oracle.pose_optimization(wp[frame_mp[idx]].astype(f64), obs, ISG[cur["keys"]["octave"][idx]].astype(f64), np.asarray(INTR, f32).astype(f64), pose)
    outlier2 = np.zeros(len(cur["keys"]), np.uint8); outlier2[idx] = flags2
    inliers = int(sum(1 for i in idx if not outlier2[i] and n_obs[frame_mp[i]] > 0))
    out.update(local_kf=local_kf, local_points=lp, local_tm=tm2, local_n=n2, local_differs=not np.array_equal(tm2, mono2), n_to_match=int(fr["in_view"].sum()), pose2=pose2,
               outlier2=outlier2, inliers=inliers, ok2=inliers >= 30, frame_mp2=frame_mp.copy())
    return out
